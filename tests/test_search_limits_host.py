"""CPU: the planted trees of tests/search_limits_ref.py.  Every frozen case has the populations its table entry claims
("exact" is a condition: a case that misses it fails here), its tree is what the oracle's own search walks with the case's
head on the CPU, and every region's zoom score lies at least 0.1 from Tz on the side the mask predicts -- no difference
between a BLAS and a device GEMM can move a region across the threshold.  Also the generator's evidence for the limits no
tree reaches ("Search limits")."""
import numpy as np
import pytest

import search_limits_ref as R
from oracle import az_oracle as orc

CASES = R.load_cases()


@pytest.fixture(scope="module")
def pops():
    return {k: R.populations(c["H"], c["W"], c["scale"], 10, 10000,
                             R.mask_of(c["runs"], *R.map_size(c["H"], c["W"], c["scale"])), want_regions=True)
            for k, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_has_the_populations_it_claims(pops, name):
    c, p = CASES[name], pops[name]
    assert c["scale"] == R.default_scale(c["H"], c["W"])
    fh, fw = R.map_size(c["H"], c["W"], c["scale"])
    assert all(0 <= r < fh and 0 <= a < b <= fw for r, a, b in c["runs"])
    for key, want in c["claims"].items():
        if isinstance(want, tuple):
            assert p[key][want[0]] == want[1], (name, key, p[key])
        else:
            assert p[key] == want, (name, key, p[key])
    # consecutive levels agree, and what a level keeps is bounded by what it divides
    for l in range(p["nlev"] - 1):
        assert p["Pn"][l] == p["P"][l + 1] and p["PZ"][l] <= p["P"][l] and p["U"][l] <= p["P"][l]
        assert p["Pn"][l] <= p["CH"][l]


def test_limit_cases_sit_where_the_table_says(pops):
    """The at / past twins: exactly the limit and at most 8 above it, same tree up to the limited level, and nothing else
    of the tree over a limit (so that the limit under test is the only reason a form can hand the search over)."""
    for at, past, lim, lev in (("lv_r_at", "lv_r_past", R.LV_R, 4), ("fl_r_at", "fl_r_past", R.FL_R, 2),
                               ("fl_r_last_at", "fl_r_last_past", R.FL_R, 2)):
        a, b = pops[at], pops[past]
        assert a["Pn"][lev] == lim and lim < b["Pn"][lev] <= lim + 8
        assert (CASES[at]["H"], CASES[at]["W"]) == (CASES[past]["H"], CASES[past]["W"])
        for key in ("P", "U"):
            assert a[key][:lev + 1] == b[key][:lev + 1]
        assert a["PZ"][:lev] == b["PZ"][:lev]
        for p in (a, b):
            assert max(p["P"][:3]) <= R.FL_R and max(p["CH"][:3]) <= R.FL_C
            assert all(p["P"][l] <= R.LV_R and p["U"][l] + 1 <= R.LV_R and p["CH"][l] <= R.LV_C
                       for l in range(3, p["nlev"] - 1))
    assert pops["lv_r_at"]["nlev"] == 6 and pops["fl_r_at"]["nlev"] == 5 and pops["fl_r_last_at"]["nlev"] == 4
    # level 3 of the LV_R twins is under FL_R: k_spec_levels hands over, k_level_geom owns levels 3 and 4
    assert pops["lv_r_past"]["P"][3] <= R.FL_R
    # SPEC_PRE: 3n - 1 children of the root, five children each -> 1 + 6 P1 rows: 49 and 67 straddle 64, 64 itself is
    # not of that form.  (The kernel's second comparison, P1spec <= 64, is implied by the first: the rows include P1.)
    for k in CASES:
        assert pops[k]["spec_rows"] == 1 + 6 * pops[k]["P1"] and (pops[k]["P1"] + 1) % 3 == 0
    assert pops["pre_49"]["spec_rows"] <= R.SPEC_PRE < pops["pre_67"]["spec_rows"]
    # the root's children against FL_R: level 1 of k_spec_levels (P in the loop, P1spec under the deferred root); both
    # trees have five levels (the deferred root needs them) and stay under every other limit
    a, b = pops["p1_254"], pops["p1_257"]
    assert a["P"][1] == a["P1"] == 254 <= R.FL_R < b["P"][1] == b["P1"] == 257 and a["nlev"] == b["nlev"] == 5
    for p in (a, b):
        assert max(p["P"][2:4]) <= R.FL_R and p["P"][4] <= R.LV_R and min(p["P"]) > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_zoom_scores_keep_their_margin_and_the_oracle_walks_the_same_tree(pops, name):
    c, p = CASES[name], pops[name]
    head, fmap, mask = R.case_inputs(c)
    for l, (B, z) in enumerate(p["regions"]):
        zoom = orc.head_forward(head, fmap[0], orc.get_rois_blob(B, c["scale"]))[0].ravel().astype(np.float64)
        want = R.zoom_predicate(B, c["scale"], mask)                # (the root's forced zoom is not a score)
        assert np.all(zoom[want] >= R.TZ + 0.1) and np.all(zoom[~want] <= R.TZ - 0.1), (name, l)
    if name in ("lv_r_at", "fl_r_past", "cap", "p1_257"):                     # the whole search, through the oracle's own loop
        onet = orc.OracleNet(head, feat_fn=lambda d: fmap)
        _, tr = orc.im_propose({"full": onet, "fc": onet}, (c["H"], c["W"]), c["scale"], orc.OracleCfg(Tz=R.TZ),
                               return_trace=True)
        for l, lev in enumerate(tr["levels"]):
            assert lev["B"].shape[0] == p["P"][l] and len(lev["indZ"]) == p["PZ"][l]
            assert sum(f["U"] for f in lev["fwd"]) == p["U"][l]


def test_chunked_dedup_counts_follow_the_batch_size(pops):
    """U of a level is one np.unique per chunk of batch_size regions: at batch == P it is the whole level's, one below it
    the last region forms a chunk of its own."""
    c, p = CASES["lv_r_at"], pops["lv_r_at"]
    for l in (3, 4, 5):
        P = p["P"][l]
        whole = R.case_populations(c, batch=P)["U"][l]
        split = R.case_populations(c, batch=P - 1)["U"][l]
        assert whole == p["U"][l] and whole <= split <= whole + 1


def test_children_tables_do_not_fill_before_the_region_tables(pops):
    """LV_C / FL_C.  Measured, not proved: over the full trees of the shapes below and over every dividing level of every
    frozen case, at most three children share a _sift_dup hash, so a level of CH children keeps at least CH / 3 regions.
    The nearest child counts to LV_C (4095, 4100: multiples of 5) then keep >= 1365 > LV_R, those to FL_C (2045, 2050)
    keep >= 682 > FL_R: the region check of the same level trips too, or -- for 4100 / 2050 -- the child check does, with
    the same flag and the same rerun, and no case can tell them apart."""
    for H, W in ((600, 1000), (800, 1200), (801, 1201), (322, 1598), (300, 1498), (400, 900), (375, 500), (1280, 1920)):
        assert max(R.max_multiplicity(H, W)) <= 3, (H, W)
    for name, p in pops.items():
        for l, (B, z) in enumerate(p["regions"][:-1]):
            m = R.level_multiplicity(B[z])
            assert m <= 3 and (m == 0 or p["Pn"][l] * m >= p["CH"][l]), (name, l, m)
    assert -(-4095 // 3) > R.LV_R and -(-2045 // 3) > R.FL_R


def test_window_predicate_is_roi_pool():
    """zoom_predicate against the oracle's RoIPool on a 0/1 map, for boxes off the grid of any tree."""
    rng = np.random.RandomState(3)
    mask = rng.rand(38, 63) < 0.02
    x1, y1 = rng.uniform(-20, 990, 400), rng.uniform(-20, 590, 400)
    B = np.stack([x1, y1, x1 + rng.uniform(0, 300, 400), y1 + rng.uniform(0, 300, 400)], axis=1)
    pooled = orc.roi_pool(mask.astype(np.float32)[None], orc.get_rois_blob(B, 1.0))
    assert np.array_equal(pooled.max(axis=1) > 0, R.zoom_predicate(B, 1.0, mask))
