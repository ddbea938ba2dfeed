"""CPU: what tests/test_gpu_train_edges.py relies on, asserted on the references alone (the cases are built in
tests/train_edges_ref.py), and the restatement tests/train_ref.py against what the REFERENCE recorded for those cases
(tests/golden/g23_train_roidb_edges.npz, written by tests/gen_golden_train_edges.py).

1. train_ref against g23: the parameter and image-size cases array by array, the large-level cases by counts and SHA-256.
2. Every case's precondition, from train_ref's own `stats` / `trace`: a case that is meant to reach a loop's second pass, a full
   buffer, a limit or a tie proves here that it does, so a changed seed or a changed train_ref cannot turn it into one more
   default-path case.
3. The host layer (az_data_layer.roidb) over train_ref.RefBackend on the cases that go through it."""
import os
import time

import numpy as np
import pytest

import train_edges_ref as E
import train_ref as tr
from oracle import az_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g23_train_roidb_edges.npz")
T0 = time.time()


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def levels():
    """train_ref on every case of group A, once: name -> (boxes, labels, used, summary of its levels, zoomed indices)."""
    out = {}
    for name in E.LEVEL_CASES:
        st = {}
        b, z, u = E.run_level_case(name, st)
        out[name] = (b, z, u, E.level_summary(st), st.get("zoomed", []))
    return out


# ---- 1. train_ref against the reference's record -------------------------------------------------------------------------------
def test_restatement_equals_reference_on_the_parameter_cases(g):
    for name, size, gt, seed, kw in E.param_cases():
        c = E.cfg_of(kw)
        used = int(g["B_%s_used" % name])
        assert np.array_equal(g["B_%s_gt" % name], gt) and tuple(g["B_%s_size" % name]) == size and int(g["B_%s_seed" % name]) == seed
        b, z, u = tr.compute_ex_rois(size, gt, E.noise_of(seed, used + 2), c)
        assert u == used, name
        assert np.array_equal(b, g["B_%s_ex_boxes" % name]) and np.array_equal(z, g["B_%s_zoom_gt" % name]), name
        t = tr.compute_targets(gt, b.astype(np.float32), c)
        ref = g["B_%s_targets" % name]
        assert t.shape == ref.shape and np.array_equal(t, ref) and not np.isnan(ref).any(), name


def test_restatement_equals_reference_on_the_large_levels(g, levels):
    for name, (size, gt, seed, kw, _) in E.LEVEL_CASES.items():
        b, z, u, s, _ = levels[name]
        t = tr.compute_targets(gt, b.astype(np.float32), E.cfg_of(kw))
        for k, v in E.level_digests(size, gt, b, z, u, t, s["levels"]).items():
            assert np.array_equal(v, g["L_%s_%s" % (name, k)]), (name, k)


def test_shared_stream_and_empty_batch_equal_reference(g):
    S = E.SHARED_STREAM
    noise, at = E.noise_of(S["seed"], 8000), 0
    for i, (size, gt) in enumerate(S["images"]):
        st = {}
        b, z, u = tr.compute_ex_rois(size, gt, noise[at:], E.cfg_of(S["kw"]), st)
        at += u
        t = tr.compute_targets(gt, b.astype(np.float32), E.cfg_of(S["kw"]))
        for k, v in E.level_digests(size, gt, b, z, u, t, E.level_summary(st)["levels"]).items():
            assert np.array_equal(v, g["S%d_%s" % (i, k)]), (i, k)
    B = E.EMPTY_BATCH
    noise, at = E.noise_of(B["seed"], 4000), 0
    for i, (size, gt) in enumerate(E.empty_batch_images()):
        b, z, u = tr.compute_ex_rois(size, gt, noise[at:], E.cfg_of(B["kw"]))
        at += u
        assert u == int(g["BE%d_used" % i]) and np.array_equal(b, g["BE%d_ex_boxes" % i]) and np.array_equal(z, g["BE%d_zoom_gt" % i])
        assert np.array_equal(tr.compute_targets(gt, b.astype(np.float32), E.cfg_of(B["kw"])), g["BE%d_targets" % i])


# ---- 2. preconditions ------------------------------------------------------------------------------------------------------------
def test_children_per_parent_is_divide_children(levels):
    rng = np.random.RandomState(5)
    x1, y1 = rng.uniform(0, 500, 300), rng.uniform(0, 500, 300)
    Z = np.stack([x1, y1, x1 + rng.uniform(1, 300, 300), y1 + rng.uniform(1, 300, 300)], 1)
    assert int(tr.children_per_parent(Z).sum()) == orc.divide_children(Z).shape[0]
    assert tr.children_per_parent(np.array([[0., 0., 2099., 11.]])).tolist() == [3 * 350 - 1]


def test_level_preconditions(levels):
    NT, LV = E.NT, E.LV_C
    for name, (_, _, u, s, _) in sorted(levels.items()):
        print("%-16s levels (P, PZ, CH) %s; one parent %d; doubles %d" % (name, s["levels"].tolist(), s["max_parent"], u))
    # 1. children in more than one pass, parents in one
    s = levels["children_passes"][3]
    assert s["max_P"] <= NT and NT < s["max_CH"] <= LV
    assert sum(1 for _, _, ch in s["levels"] if ch > NT) >= 2                     # the sort's and the dedup's passes, twice
    # 2. parents in two passes; in one such level the zoomed regions lie on both sides of index 1024
    b, z, u, s, zoomed = levels["parent_passes"]
    assert s["max_P"] > NT and s["max_CH"] <= LV
    straddle = [(int((zi < NT).sum()), int((zi >= NT).sum())) for (p, pz, _), zi in zip(s["levels"], zoomed) if p > NT and pz > 0]
    assert straddle and any(lo >= 1 and hi >= 1 for lo, hi in straddle), straddle
    print("parent_passes: zoomed regions below / above index 1024: %s" % straddle)
    # (a level with PZ > 1024 cannot fit: every parent has at least 5 children, 5 * 1025 > 4096)
    assert int(tr.children_per_parent(np.array([[0., 0., 9., 9.]]))[0]) == 5 and 5 * (NT + 1) > LV
    # 3. the fullest level and its neighbour
    s, so = levels["level_full"][3], levels["level_over"][3]
    assert 3900 <= s["max_CH"] <= LV and so["max_CH"] > LV
    assert s["max_CH"] == 4095                                                    # one step below: every buffer full but one word
    first_over = [ch for _, _, ch in so["levels"] if ch > LV][0]
    assert all(ch <= LV for _, _, ch in so["levels"][:[c for _, _, c in so["levels"]].index(first_over)])
    # 4. one parent across the passes; the thin image's first level past the limit
    s = levels["thin_parent"][3]
    assert s["max_P"] == 1 and NT < s["max_parent"] == s["max_CH"] <= LV
    so = levels["thin_over"][3]
    assert so["levels"][0][2] > LV
    # 5. super-regions past one pass, 1024 inside an object's rows (or exactly at their end)
    for name, S in (("objects_94", 11), ("objects_120", 11), ("objects_64_s16", 16), ("objects_65_s16", 16)):
        gt = E.LEVEL_CASES[name][1]
        NS = gt.shape[0] * S
        assert NS >= NT and levels[name][3]["max_CH"] <= LV, name
        assert np.array_equal(gt[-1], gt[0]) and gt[-2, 2] == gt[-2, 0] and gt[-2, 3] == gt[-2, 1] and gt[-3, 2] == gt[-3, 0]
    assert (94 * 11) > NT and NT % 11 != 0 and 64 * 16 == NT and 65 * 16 > NT
    # 7. the hash: the first level fits (so the capacity check does not answer first) and a key leaves [0, 2^40)
    size, gt, seed, kw, answer = E.LEVEL_CASES["hash_range"]
    s = levels["hash_range"][3]
    assert answer == "invalid" and s["levels"][0][2] <= LV
    root = np.array([[0., 0., size[1] - 1.0, size[0] - 1.0]])
    keys = np.round(orc.divide_children(root) / kw["min_side"]).astype(np.int64).dot(np.array([1, 10 ** 3, 10 ** 6, 10 ** 9], dtype=np.int64))
    assert keys.min() >= 0 and keys.max() >= (1 << 40)
    assert tr.num_levels(size, kw["min_side"]) <= 16                              # AZ_MAX_LEVELS: the C ABI accepts the image
    for name in ("level_over", "thin_over"):
        assert E.LEVEL_CASES[name][4] == "capacity"


def test_shared_stream_preconditions():
    S = E.SHARED_STREAM
    noise, at, seen = E.noise_of(S["seed"], 8000), 0, []
    for size, gt in S["images"]:
        st = {}
        b, z, u = tr.compute_ex_rois(size, gt, noise[at:], E.cfg_of(S["kw"]), st)
        at += u
        seen.append((E.level_summary(st), b.shape[0], tr.num_levels(size, 10), gt.shape[0]))
    assert seen[0][0]["max_P"] > E.NT and seen[0][0]["max_CH"] <= E.LV_C            # a multi-pass level first
    assert seen[1][3] * 11 > E.NT and seen[1][0]["max_CH"] <= E.LV_C
    assert seen[2][1] == 0 and seen[2][2] <= 0 and seen[2][3] >= 1                  # no level, an object, nothing kept
    assert seen[3][1] > 0 and seen[3][0]["max_P"] <= E.NT


def test_parameter_case_preconditions(g):
    by = {c[0]: c for c in E.param_cases()}
    names = set(by)
    assert {"rep0", "rep1", "rep3", "add1", "add16", "sub1", "sub5", "sub16", "ms5", "ms16", "ms12_5", "zep0", "zep1",
            "emb_01_09", "emb_10_00", "adj0", "adj05", "adj1", "eps14", "eps6", "side_below", "side_min", "side_2min", "wide",
            "tall"} <= names
    for rows in (E.SUB16, E.ADD16):
        r = np.array(rows)
        assert np.all(r[:, 2] > r[:, 0]) and np.all(r[:, 3] > r[:, 1]) and len(set(map(tuple, rows))) == 16
    assert int(g["B_rep0_used"]) == 0 and g["B_rep0_ex_boxes"].shape[0] > 0       # super-regions only
    assert g["B_side_below_ex_boxes"].shape[0] == 0 and by["side_below"][2].shape[0] > 0
    assert tr.num_levels(by["side_below"][1], 10) <= 0 and tr.num_levels(by["side_min"][1], 10) == 1
    assert tr.num_levels(by["side_2min"][1], 10) == 2 and min(by["side_2min"][1]) == 20 and min(by["side_min"][1]) == 10
    assert by["wide"][1][0] < by["wide"][1][1] and by["tall"][1][0] > by["tall"][1][1]
    # adj_thresh 0: every object adjacent, min(S, N) binds at every region, matches won at overlap 0
    name, size, gt, seed, kw = by["adj0"]
    trace = {}
    ex = g["B_adj0_ex_boxes"].astype(np.float32)
    t = tr.compute_targets(gt, ex, E.cfg_of(kw), trace)
    assert gt.shape[0] > 11 and t.shape[0] == 11 * ex.shape[0] and trace["bound"] == ex.shape[0] and trace["zero_rounds"] >= 1
    # adj_thresh 1: only identical boxes (an object's own first super-region)
    t1 = g["B_adj1_targets"]
    assert t1.shape[0] >= 1 and np.all(t1[:, 6] == 1.0)
    assert int(g["B_zep1_used"]) == 5 and g["B_emb_10_00_zoom_gt"].all()          # no objects embedded / all
    B = E.EMPTY_BATCH
    e = [g["BE%d_ex_boxes" % i].shape[0] for i in range(len(B["names"]))]
    assert e[0] == 0 and e[2] == 0 and e[4] == 0 and e[1] > 0 and e[3] > 0
    assert g["BE1_targets"].shape[0] > 0 and g["BE3_targets"].shape[0] > 0


def test_match_case_preconditions():
    for N, S in E.MATCH_SIZES:
        ex, gt, twins = E.match_case(N, S)
        lds = S * N * 8
        assert lds <= E.LDS_MAX and ex.shape[0] <= 36
        seen, zero, ties, bound = [], 0, 0, 0
        for adj in (0.1, 0.0):
            trace = {}
            t = tr.compute_targets(gt, ex, E.cfg_of(E.match_kw(S, adj)), trace)
            seen += trace["argmax"]
            if adj == 0.0:
                assert t.shape[0] == S * ex.shape[0] and trace["zero_rounds"] >= 1    # min(S, N) binds, rounds won at overlap 0
            ties += trace.get("ties", 0)
            bound += trace.get("bound", 0)
        am = np.array(seen)
        ng = (S * N + 63) // 64
        groups, lanes = set((am // 64).tolist()), set((am % 64).tolist())
        print("N=%d S=%d: %d regions, LDS %d bytes, first maxima in %d of %d groups of 64 and %d lanes, %d twins"
              % (N, S, ex.shape[0], lds, len(groups), ng, len(lanes), twins))
        assert 0 in groups and ng - 1 in groups and len(groups) >= 0.95 * ng - 1
        assert am.max() == S * N - 1 and am.min() == 0                             # the first and the very last entry
        if N >= 744:
            assert lanes == set(range(64))
        else:                                                                        # (at most 121 rounds here)
            assert len(lanes) >= 32
        if N >= 129:                                                                 # identical objects > 64 columns apart
            assert twins >= 1 and ties >= 1 and bound >= 1
            same = [(a, a + 70) for a in range(N - 70) if np.array_equal(gt[a], gt[a + 70])]
            assert len(same) == twins
    assert 744 * 88 <= 65536 < 745 * 88 and 1489 * 88 == 131032 and 1024 * 128 == E.LDS_MAX
    for N, S in E.MATCH_OVER:
        assert S * N * 8 > E.LDS_MAX and S * (N - 1) * 8 <= E.LDS_MAX


def test_stats_rows_are_exact_in_any_order():
    for n_sub in E.STATS_NSUB:
        for T in E.STATS_T:
            t = E.stats_exact_rows(n_sub, T, 7 * n_sub + T)
            assert t.shape == (T, 7)
            m, s, tn = E.stats_reference(t, n_sub, 0.0)
            rev = np.ascontiguousarray(t[::-1])
            m2, s2, _ = E.stats_reference(rev, n_sub, 0.0)
            assert np.array_equal(m, m2, equal_nan=True) and np.array_equal(s, s2, equal_nan=True)
            # per class: a power-of-two count, sums that a long-double accumulation reproduces without rounding
            for cls in range(n_sub):
                x = t[t[:, 5] == cls, :4]
                if x.shape[0] == 0:
                    assert np.isnan(m[cls]).all()
                    continue
                assert x.shape[0] & (x.shape[0] - 1) == 0
                assert np.array_equal((x.astype(np.longdouble).sum(0) / x.shape[0]).astype(np.float64), m[cls])
                assert np.array_equal(x * 256, np.round(x * 256)) and np.abs(x).max() <= 4
            inside = (t[:, 5] >= 0) & (t[:, 5] < n_sub) & (t[:, 5] == np.floor(t[:, 5]))
            assert np.array_equal(tn[~inside], t[~inside])                          # rows of no class: untouched
            if T > n_sub * 2:
                assert (~inside).sum() == T - inside.sum() and (s[0] == 0).all()    # class 0: identical rows
            if T >= 4097 and T % 2 == 1:
                assert {-1.0, float(n_sub), 1e9, 2.5, -0.5} & set(t[~inside, 5].tolist())
    # a class with one row: std 0, its normalised row nan, as NumPy has it
    t = E.stats_exact_rows(11, 1, 3)
    m, s, tn = E.stats_reference(t, 11, 0.0)
    assert (s[0] == 0).all() and np.isnan(tn[0, :4]).all() and np.isnan(m[1:]).all()


def test_ref_backend_takes_any_n_sub():
    be = tr.RefBackend()
    for n_sub in E.STATS_NSUB:
        t = E.stats_random_rows(n_sub, 300, n_sub)
        m, s = be.train_target_stats(n_sub, 1e-14, t.copy(), False)
        assert m.shape == (n_sub, 4) and np.isfinite(s).all()


# ---- 3. the host layer -------------------------------------------------------------------------------------------------------------
class LimitBackend(tr.RefBackend):
    """RefBackend with the device's level limit: a level past LV_C is AZ_ERR_CAPACITY without `.needed`."""

    def train_ex_rois(self, tp, sizes, gt_list, noise, cap=None):
        from aznet_hip import ffi
        at = 0
        for size, gt in zip(sizes, gt_list):
            st = {}
            at += tr.compute_ex_rois(size, gt, noise[at:], self._cfg(tp), st)[2]
            if st.get("max_children", 0) > E.LV_C:
                raise ffi.AzError(ffi.AZ_ERR_CAPACITY, "a level holds more than %d children" % E.LV_C)
        return tr.RefBackend.train_ex_rois(self, tp, sizes, gt_list, noise, cap)


@pytest.fixture()
def rdl():
    from az_data_layer import roidb as m
    yield m
    m.set_backend(None)


def test_host_layer_surfaces_the_level_overflow(rdl):
    rdl.set_backend(LimitBackend())
    E.host_overflow(rdl)


def test_host_layer_on_mixed_images(rdl, monkeypatch):
    rdl.set_backend(tr.RefBackend())
    E.check_mixed(*E.host_mixed(rdl, monkeypatch), in_err_ulps=0)


def test_zz_time():
    print("tests/test_train_edges_host.py: %.1f s" % (time.time() - T0))
