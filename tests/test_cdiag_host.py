"""CPU: the NumPy restatement of az_coco_diag_eval (tests/cdiag_ref.py) held to what already exists -- the COCOeval
restatement (coco_eval_ref) for variant 0, the TP claims and the ignored rows -- and to a hand-worked set; the binding's
argument checks, the header, and detect.diagnose_det's COCO packing, host tables and text with the restatement as the device."""
import os
import re
import sys

import numpy as np
import pytest

import cdiag_ref as C
import coco_cases
import coco_eval_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
# a perfect curve in accumulate's arithmetic: tp / (tp + np.spacing(1)) is 1.0 from two TPs on (2 + 2^-52 rounds to 2), and
# with ONE object it is 1 / (1 + 2^-52) = 1 - 2^-52 at every recall threshold
ONE_TP = 1.0 / (1.0 + np.spacing(1))


def _sets():
    out = [(name, c, None) for name, c in sorted(coco_cases.CASES.items())]
    for seed in range(12):
        c = coco_cases.random_set(seed)
        out.append(("seed %d" % seed, c, np.arange(c["n_classes"]) // 2))
    return out


@pytest.fixture(scope="module")
def diagnosed():
    return [(name, c, R.coco_eval(*C.args(c)), C.diag(*C.args(c), class_group=g)) for name, c, g in _sets()]


def test_variant_0_is_the_coco_evaluation(diagnosed):
    for name, c, ref, d in diagnosed:
        assert np.array_equal(d["prec_fix"][0], ref["precision"][:, :, :, 0, 2]), name
        assert np.array_equal(d["recall_fix"][0], ref["recall"][:, :, 0, 2]), name


def test_tp_rows_claims_and_ignored_rows_are_the_coco_matching(diagnosed):
    seen = set()
    for name, c, ref, d in diagnosed:
        m, ig, ty = ref["dt_match"][0], ref["dt_ignore"][0], d["type"]
        assert np.array_equal(ty == -1, ig == -1), name
        assert np.array_equal(ty == C.IGN, ig == 1), name
        assert np.array_equal(ty == C.TP, (m >= 0) & (ig == 0)), name
        seg0 = np.repeat(c["gt_off"][:-1], np.diff(c["det_off"]))           # each detection's segment's first box
        for t in range(C.T):
            tp = np.nonzero(ty[t] == C.TP)[0]
            assert np.array_equal(d["gt_claim"][t, seg0[tp] + m[t, tp]], tp), name
            assert (d["gt_claim"][t] >= 0).sum() == tp.size, name
            assert (d["gt_claim"][t, c["gt_crowd"] != 0] == -1).all(), name
        seen |= set(np.unique(ty).tolist())
        assert np.array_equal(d["type_table"][:, :, C.TP] + d["miss"], np.repeat(d["npos"][:, None], C.T, 1)), name
        assert not (d["loc_fixed"] & (ty != C.LOC)).any(), name
    assert seen == set(range(-1, 7))


def test_variant_7_is_a_perfect_curve(diagnosed):
    some = 0
    for name, c, ref, d in diagnosed:
        p7 = d["prec_fix"][7]                                               # [T, R, K]
        npig = d["type_table"][:, :, C.TP] + np.array([[d["loc_fixed"][t, c["det_off"][k * c["n_images"]]:
                                                                       c["det_off"][(k + 1) * c["n_images"]]].sum()
                                                         for t in range(C.T)] for k in range(c["n_classes"])])
        for k in range(c["n_classes"]):
            for t in range(C.T):
                want = -1.0 if npig[k, t] == 0 else (ONE_TP if npig[k, t] == 1 else 1.0)
                assert (p7[t, :, k] == want).all(), (name, k, t)
                assert d["recall_fix"][7, t, k] == (-1.0 if npig[k, t] == 0 else 1.0), (name, k, t)
                some += npig[k, t] > 1
        # variant 6 divides by the objects found: its recall is 1 wherever anything was found
        r6 = d["recall_fix"][6]
        assert ((r6 == 1.0) | (r6 == -1.0)).all(), name
    assert some > 50


def test_hand_worked_set():
    from aznet_hip import ffi
    d = C.diag(*C.args(C.HAND), class_group=C.HAND_GROUP)
    idx = np.array(C.HAND_INDEX)
    assert d["npos"].tolist() == [3, 1, 1]
    for t in (0, 5):
        assert d["type"][t, idx].tolist() == C.HAND_TYPES[t], t
        assert np.nonzero(d["loc_fixed"][t, idx])[0].tolist() == C.HAND_FIXED[t], t
        assert d["gt_claim"][t, :4].tolist() == [idx[r] if r >= 0 else -1 for r in C.HAND_CLAIM[t]], t
        assert d["type"][t, 12] == C.TP and d["gt_claim"][t, 4] == 12 and d["gt_claim"][t, 5] == -1
    # d1 turns from DUP to LOC above its IoU .8; from .85 B is free again and d2, the first LOC row on it, is fixed
    assert d["type"][:, idx[1]].tolist() == [C.DUP] * 7 + [C.LOC] * 3
    assert d["type"][:, idx[4]].tolist() == [C.DUP] * 3 + [C.TP] * 4 + [C.LOC] * 3
    assert d["loc_fixed"][:, idx[2]].tolist() == [0] * 7 + [1] * 3 and d["loc_fixed"][:, idx[4]].sum() == 0
    assert d["ov_same"][idx].tolist() == [1.0, 0.8, 0.625, 0.5, 0.8, 0.0, 0.0, 0.0, 0.0, 0.2, 0.4, 0.25]
    assert d["arg_same"][idx].tolist() == [0, 0, 1, 1, 1, -1, -1, -1, -1, 0, 3, 3]      # d9 meets A and B alike: the first
    assert d["ov_other"][idx[6]] == 1.0 and d["ov_other"][idx[7]] == 0.5
    assert d["other_class"][idx].tolist() == [-1] * 6 + [1, 2] + [-1] * 4
    assert d["type_table"][0, 0].tolist() == [1, 2, 3, 3, 1, 1, 1] and d["type_table"][0, 5].tolist() == [1, 2, 1, 5, 1, 1, 1]
    assert d["miss"][0, [0, 5]].tolist() == [1, 1] and d["miss"][2].tolist() == [1] * 10
    means = ffi.coco_diag_means(d["prec_fix"])
    for (t, v), want in C.HAND_AP.items():
        # the fractions are exact; accumulate's np.spacing(1) moves a precision by at most 2^-52
        assert abs(means["ap_fix"][0, t, v] - float(want)) < 1e-12, (t, v, means["ap_fix"][0, t, v], float(want))
    assert means["ap_fix"].shape == (3, 10, 8) and means["stats_fix"].shape == (8, 3)
    assert np.array_equal(means["stats_fix"][0], R.summarize(R.coco_eval(*C.args(C.HAND))["precision"], -np.ones((10, 3, 4, 3)))[:3])
    # category 2 has an object and no detection: 0 under every variant that keeps its npig, -1 where nothing is left
    assert (d["prec_fix"][:6, :, :, 2] == 0).all() and (d["prec_fix"][6:, :, :, 2] == -1).all()
    assert np.isnan(means["ap_fix"][2, :, 6:]).all()


def test_bg_overlap_is_inclusive_and_the_cap_hides_a_true_positive():
    c = C.bg_edge_case()
    at = C.diag(*C.args(c), bg_overlap=0.1)
    above = C.diag(*C.args(c), bg_overlap=np.nextafter(0.1, 1.0))
    assert at["ov_same"][0] == 0.1 and at["ov_other"][1] == 0.1
    assert at["type"][0].tolist() == [C.LOC, C.OTH] and above["type"][0].tolist() == [C.BG, C.BG]
    for n in (99, 100, 101, 165):
        c = C.cap_case(n)
        d = C.diag(*C.args(c))
        assert (d["type"][0] == -1).sum() == max(0, n - 100) and d["type"][0, n - 1] == C.TP
        # box 1's only detection scores lowest: past the cap it is not evaluated and the box counts as missed
        assert d["type"][0, 0] == (C.TP if n <= 100 else -1) and d["miss"][0, 0] == (0 if n <= 100 else 1)
        assert d["gt_claim"][0].tolist() == [n - 1, 0 if n <= 100 else -1]
    d = C.diag(*C.args(C.loc_case()))
    assert d["type"][0].tolist() == [C.LOC, C.TP, C.TP, C.LOC, C.LOC] and d["loc_fixed"][0].tolist() == [0, 0, 0, 1, 0]
    assert d["type"][3].tolist() == [C.LOC, C.LOC, C.TP, C.LOC, C.LOC] and d["loc_fixed"][3].tolist() == [0, 1, 0, 1, 0]


def test_case_builders_hold_what_they_promise():
    for same in (True, False):
        c, group = C.tie_case(same)
        d = C.diag(*C.args(c), class_group=group)
        n = len(C.TIE_PAIRS)
        first = np.array([a for a, _ in C.TIE_PAIRS])
        assert (63, 64) in C.TIE_PAIRS and sorted(a for a, _ in C.TIE_PAIRS) == list(range(64))
        if same:
            assert np.array_equal(d["arg_same"][:n], first) and (d["ov_same"][:n] == 0.25).all() and (d["type"][:, :n] == C.LOC).all()
        else:
            assert (d["other_class"][:n] == 1).all() and (d["ov_other"][:n] == 0.25).all()
            assert set(d["type"][0, :n].tolist()) == {C.SIM}
    c, crowd = C.crowd_case()
    d = C.diag(*C.args(c))
    assert (d["type"][:, :10] == C.IGN).all() and (d["gt_claim"][:, list(crowd)] == -1).all()
    assert not np.isin(d["arg_same"], list(crowd)).any()
    assert d["arg_same"][10] == 31 and d["type"][0, 10] == C.LOC and d["type"][0, 11] == C.BG and d["ov_other"][11] == 0.0
    for n_own, before, after in ((63, 0, 0), (1, 62, 1), (65, 63, 2)):
        c = C.wave_case(n_own, before, after, crowd_at=(0, n_own - 1) if n_own > 2 else ())
        assert c["gt_off"][2] - c["gt_off"][1] == n_own and c["gt_off"][-1] == n_own + before + after
        d = C.diag(*C.args(c), class_group=np.array([0, 0, 1], np.int32))
        assert all((d["type"][0] == t).any() for t in (C.TP, C.LOC, C.BG))
    c = C.class_count_case(5)
    none, one = C.diag(*C.args(c)), C.diag(*C.args(c), class_group=np.zeros(5, np.int32))
    assert np.array_equal(none["type"] == C.OTH, one["type"] == C.SIM) and (none["type"] == C.OTH).any()
    assert all((none["type"][0] == t).any() for t in range(7) if t != C.SIM)


def test_binding_checks_its_arguments_without_a_device():
    from aznet_hip import ffi
    assert "az_coco_diag_eval" in ffi.SYMBOLS
    ctx = ffi.AzContext.__new__(ffi.AzContext)           # no az_create: the checks come before the library is touched
    base = dict(zip(C.KEYS, C.args(C.HAND)), class_group=C.HAND_GROUP)
    for key in ("det_off", "gt_off", "det_box", "det_score", "gt_box", "gt_area", "gt_crowd", "class_group"):
        with pytest.raises(ffi.AzError) as e:
            ctx.coco_diag_eval(**dict(base, **{key: base[key][:-1]}))
        assert e.value.code == ffi.AZ_ERR_INVALID, key


def test_header_and_makefile_declare_the_entry():
    header = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    m = re.search(r"\bint az_coco_diag_eval\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 25
    for word in ("bg_overlap", "class_group", "type_out", "loc_fixed_out", "gt_claim_out", "prec_fix_out", "recall_fix_out",
                 "kernel_ms_out"):
        assert word in m.group(1)
    mk = open(os.path.join(REPO, "az-net_amd", "csrc", "Makefile")).read()
    assert "az_cdiag.o" in mk


# ------------------------------------------------------------------------------------------------------------- Python
class _StubCtx(object):
    """Answers coco_diag_eval with the restatement (and det_diag_eval with the VOC one)."""

    def __init__(self):
        self.calls = []

    def coco_diag_eval(self, *a, **kw):
        from aznet_hip import ffi
        self.calls.append((a, kw))
        out = C.diag(*a, **kw)
        out.update(ffi.coco_diag_means(out["prec_fix"]))
        return out

    def det_diag_eval(self, *a, **kw):
        import ddiag_ref
        return ddiag_ref.diag_flat(*a, **kw)


def _all_boxes(db, seed=5):
    """test_net-style all_boxes near the devkit's ground truth (as test_gpu_coco_eval.py builds them)."""
    rng = np.random.RandomState(seed)
    roidb = db.gt_roidb()
    out = [[[] for _ in range(db.num_images)] for _ in range(db.num_classes)]
    for i, e in enumerate(roidb):
        for b, k in zip(e["boxes"].astype(np.float32), e["gt_classes"]):
            d = np.zeros((2, 5), np.float32)
            d[:, :4] = b + rng.normal(0, 2, (2, 4)).astype(np.float32)
            d[:, 2:4] = np.maximum(d[:, 2:4], d[:, 0:2] + 1)
            d[:, 4] = rng.rand(2)
            out[k][i] = d if isinstance(out[k][i], list) else np.vstack([out[k][i], d])
        k = 1 + rng.randint(db.num_classes - 1)
        if isinstance(out[k][i], list):
            out[k][i] = np.array([[5, 5, 60, 70, 0.3]], np.float32)
    return out


def test_a_coco_imdb_is_packed_as_evaluation_packs_it(tmp_path):
    import json
    from datasets import coco_eval
    from datasets.coco import coco
    from detect import diagnose_det as DD
    devkit = coco_cases.make_devkit(tmp_path / "kit")
    db = coco("val", "2014", devkit)
    all_boxes = _all_boxes(db)
    ctx = _StubCtx()
    d = DD.diagnose(db, all_boxes, ctx=ctx, protocol="coco")
    # the arguments are those of evaluate_detections' results file, read back
    path = db._write_coco_results_file(all_boxes, str(tmp_path))
    want = coco_eval.pack(db._coco[0], json.load(open(path)))
    (a, kw), = ctx.calls
    for got, key in zip(a, C.KEYS):
        assert np.array_equal(got, want[key]), key
    assert kw["bg_overlap"] == 0.1 and kw["class_group"].tolist() == [0] * 80          # one supercategory: one group
    ref = R.coco_eval(*C.args(want))
    assert np.array_equal(d["stats_fix"][0], ref["stats"][:3]) and d["protocol"] == "coco"
    assert np.array_equal(d["dap_stats"], d["stats_fix"][1:] - d["stats_fix"][0]) and d["dap_stats"].shape == (7, 3)
    assert np.array_equal(d["dap"], d["ap_fix"][:, :, 1:] - d["ap_fix"][:, :, :1], equal_nan=True) and d["dap"].shape == (80, 10, 7)
    assert d["gt_by_size"].shape == (80, 3) and d["miss_by_size"].shape == (80, 10, 3) and d["confusion"].shape == (80, 80)
    counts = (want["gt_crowd"] == 0)
    assert d["gt_by_size"].sum() == counts.sum() == d["npos"].sum()
    assert np.array_equal(d["miss_by_size"].sum(2), d["miss"])
    ty0 = d["type"][0]
    assert d["confusion"].sum() == ((ty0 == C.SIM) | (ty0 == C.OTH)).sum() and not (d["type"] == C.OTH).any()
    assert "fp_at" not in d and "cuts" not in d
    # categories without a supercategory: every class on its own; a dict of groups still applies
    for c in db._coco[0].dataset["categories"][:3]:
        del c["supercategory"]
    assert DD.diagnose(db, all_boxes, ctx=_StubCtx(), protocol="coco")["class_group"] is None
    g = DD.diagnose(db, all_boxes, ctx=_StubCtx(), protocol="coco", groups={"person": "x", "bicycle": "x"})["class_group"]
    assert g[0] == g[1] and len(set(g.tolist())) == 79
    lines = DD.summary_lines(d)
    text = "\n".join(lines)
    assert "IoU .50:.95" in text and "at IoU 0.50" in text and "at IoU 0.75" in text and "Missed objects by size" in text
    assert "Confusions" in text and "top-ranked" not in text
    assert lines[2].split()[2] == "%.1f" % (100 * ref["stats"][0]) and len(lines[2].split()) == 10
    with pytest.raises(ValueError):
        DD.diagnose(coco("test", "2014", devkit), all_boxes, ctx=_StubCtx(), protocol="coco")
    with pytest.raises(ValueError):
        DD.diagnose(db, all_boxes, ctx=_StubCtx(), protocol="tide")


def test_the_synthetic_imdb_is_packed_from_gt_roidb():
    from datasets.factory import get_imdb
    from detect import diagnose_det as DD
    imdb = get_imdb("synthetic_375x500_4")
    roidb = imdb.gt_roidb()
    K, N = imdb.num_classes - 1, imdb.num_images
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(N)] for _ in range(K + 1)]
    n_obj = 0
    for i, e in enumerate(roidb):
        for b, k in zip(e["boxes"].astype(np.float32), e["gt_classes"]):
            all_boxes[k][i] = np.vstack([all_boxes[k][i], np.r_[b, 0.9].astype(np.float32)[None]])
            n_obj += 1
    b0, k0 = roidb[0]["boxes"][0].astype(np.float64), int(roidb[0]["gt_classes"][0])
    free = next(k for k in range(1, K + 1) if k not in roidb[0]["gt_classes"].tolist())
    all_boxes[free][0] = np.r_[b0, 0.4].astype(np.float32)[None]                       # another class on an object: OTH
    ctx = _StubCtx()
    d = DD.diagnose(imdb, all_boxes, ctx=ctx, protocol="coco")
    (a, kw), = ctx.calls
    assert a[0] == K and a[1] == N and kw["class_group"] is None and not a[7].any()
    first = int(a[8][(k0 - 1) * N])                                                     # class k0, image 0: its first box
    assert a[5][first].tolist() == [b0[0], b0[1], b0[2] - b0[0] + 1, b0[3] - b0[1] + 1]
    assert np.array_equal(a[6], a[5][:, 2] * a[5][:, 3]) and a[5].shape[0] == n_obj
    assert (d["type"] == C.TP).sum() == 10 * n_obj and (d["type"] == C.OTH).sum() == 10 and d["miss"].sum() == 0
    assert d["confusion"][free - 1, k0 - 1] == 1 and d["confusion"].sum() == 1
    has = d["npos"] > 0
    assert np.isin(d["prec_fix"][7][:, :, has], (1.0, ONE_TP)).all() and (d["prec_fix"][:, :, :, ~has] == -1).all()
    # (the OTH row is of a class without objects: its curves are -1 and it costs no AP)
    assert d["stats_fix"][7, 0] > 0.999999 and (d["dap_stats"] >= 0).all()
    assert len(DD.summary_lines(d)) > 10


def test_the_voc_protocol_returns_todays_keys():
    from datasets.factory import get_imdb
    from detect import diagnose_det as DD
    imdb = get_imdb("synthetic_375x500_4")
    all_boxes = [[[] for _ in range(imdb.num_images)] for _ in range(imdb.num_classes)]
    all_boxes[1][0] = np.array([[10, 10, 80, 90, 0.5]], np.float32)
    d = DD.diagnose(imdb, all_boxes, ctx=_StubCtx())
    e = DD.diagnose(imdb, all_boxes, ctx=_StubCtx(), protocol="voc")
    keys = {"type", "ov_same", "arg_same", "ov_other", "other_class", "loc_fixed", "gt_claim", "type_table", "miss", "fp_at",
            "npos", "ap_fix", "cuts", "classes", "class_group", "imdb", "num_images", "metric_07", "min_overlap", "bg_overlap",
            "area_edges", "det_off", "gt_off", "gt_box", "gt_difficult", "gt_by_size", "miss_by_size", "confusion", "dap",
            "mean_dap"}
    assert set(d) == keys == set(e)
    assert any("top-ranked" in l for l in DD.summary_lines(d))


def test_tool_parser_takes_the_protocol():
    sys.path.insert(0, os.path.abspath(TOOLS))
    try:
        tool = __import__("diagnose_det")
    finally:
        sys.path.pop(0)
    p = tool.build_parser()
    assert p.parse_args(["d.pkl"]).protocol == "voc" and p.parse_args(["d.pkl", "--protocol", "coco"]).protocol == "coco"
    with pytest.raises(SystemExit):
        p.parse_args(["d.pkl", "--protocol", "tide"])
    assert "det_diagnosis_coco.pkl" in tool.__doc__ and "ten thresholds" in tool.__doc__ and "coco" in p.format_help()
