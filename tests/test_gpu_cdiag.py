"""GPU: az_coco_diag_eval ("Detection diagnosis, COCO protocol") against the NumPy restatement
tests/cdiag_ref.py -- every per-detection, per-box and table output equal and prec_fix / recall_fix bit for bit -- at the
kernels' wave, chunk, cap, class-count and threshold edges, against az_coco_eval on the same inputs, its refusals, and
tools/diagnose_det.py --protocol coco beside tools/eval_det.py."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import cdiag_ref as C
import coco_cases
import coco_eval_ref as R
from coco_cases import CASES

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
ONE_TP = 1.0 / (1.0 + np.spacing(1))                     # a perfect precision with one object (test_cdiag_host.py)


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def _check(ctx, case, what="", **kw):
    got = ctx.coco_diag_eval(*C.args(case), **kw)
    C.same(got, C.diag(*C.args(case), **kw), what)
    return got


# -------------------------------------------------------------------------------------------------------- small sets
def test_hand_cases_equal_the_restatement(ctx):
    for name in sorted(CASES):
        _check(ctx, CASES[name], name)
    d = _check(ctx, C.HAND, "hand-worked", class_group=C.HAND_GROUP)
    idx = np.array(C.HAND_INDEX)
    for t in (0, 5):
        assert d["type"][t, idx].tolist() == C.HAND_TYPES[t] and np.nonzero(d["loc_fixed"][t, idx])[0].tolist() == C.HAND_FIXED[t]
    for (t, v), want in C.HAND_AP.items():
        assert abs(d["ap_fix"][0, t, v] - float(want)) < 1e-12, (t, v)
    # a category with detections and no ground truth: -1, left out of the means
    d = ctx.coco_diag_eval(*C.args(CASES["no_gt_class"]))
    assert (d["prec_fix"][:, :, :, 1] == -1).all() and np.isnan(d["ap_fix"][1]).all() and (d["type"][:, 1] == C.OTH).all()
    assert np.array_equal(d["stats_fix"][0], R.coco_eval(*C.args(CASES["no_gt_class"]))["stats"][:3])


def test_forty_random_sets_equal_the_restatement(ctx):
    seen = set()
    for seed in range(40):
        c = coco_cases.random_set(seed)
        d = _check(ctx, c, "seed %d" % seed, class_group=np.arange(c["n_classes"]) // 2, bg_overlap=(0.1, 0.25)[seed % 2])
        seen |= set(np.unique(d["type"]).tolist())
    assert seen == set(range(-1, 7))


def test_iou_exactly_on_the_thresholds(ctx):
    d = _check(ctx, CASES["iou_edges"], "iou edges")
    assert d["ov_same"].tolist() == [0.75, 0.5]
    assert d["type"][:, 0].tolist() == [C.TP] * 6 + [C.LOC] * 4           # IoU .75 is a match at the threshold .75
    assert d["type"][:, 1].tolist() == [C.DUP] + [C.LOC] * 9              # IoU .5, the box taken: DUP at .50 only
    assert d["loc_fixed"][:, 0].tolist() == [0] * 6 + [1] * 4 and d["loc_fixed"][:, 1].sum() == 0
    c = C.bg_edge_case()
    up = np.nextafter(0.1, 1.0)
    want = {0.1: [C.LOC, C.OTH], up: [C.BG, C.BG], 0.0: [C.LOC, C.OTH], 0.5: [C.BG, C.BG]}
    for bg, types in want.items():
        d = _check(ctx, c, "bg_overlap %r" % bg, bg_overlap=bg)
        assert d["ov_same"][0] == 0.1 and d["ov_other"][1] == 0.1 and d["type"][0].tolist() == types, bg
    d = _check(ctx, CASES["iou_edges"], "bg_overlap 0.5", bg_overlap=0.5)
    assert d["type"][:, 1].tolist() == [C.DUP] + [C.LOC] * 9              # ov_same .5 >= bg_overlap .5


def test_the_fix_rule(ctx):
    d = _check(ctx, C.loc_case(), "loc")
    # row 0's box is claimed by the lower-ranked row 2; rows 3 and 4 share an unclaimed box; row 1 is TP at .50 and LOC from .65
    assert d["type"][0].tolist() == [C.LOC, C.TP, C.TP, C.LOC, C.LOC] and d["loc_fixed"][0].tolist() == [0, 0, 0, 1, 0]
    assert d["type"][3].tolist() == [C.LOC, C.LOC, C.TP, C.LOC, C.LOC] and d["loc_fixed"][3].tolist() == [0, 1, 0, 1, 0]
    assert d["gt_claim"][0].tolist() == [2, -1, 1] and d["gt_claim"][3].tolist() == [2, -1, -1]


# -------------------------------------------------------------------------------------------------------- wave edges
@pytest.mark.parametrize("n_own,before,after", [(63, 0, 0), (64, 0, 0), (65, 0, 0), (130, 0, 0), (1, 62, 0), (1, 62, 1), (1, 63, 1),
                                                (10, 60, 60), (65, 63, 2), (64, 1, 65)])
def test_segment_and_image_sizes_round_the_wave(ctx, n_own, before, after):
    crowd = tuple(p for p in (0, 31, 62, 63, 64, n_own - 1) if 0 < n_own - 1 and p < n_own)
    c = C.wave_case(n_own, before, after, crowd_at=crowd)
    assert c["gt_off"][2] - c["gt_off"][1] == n_own and c["gt_off"][-1] == n_own + before + after
    d = _check(ctx, c, "wave", class_group=np.array([0, 0, 1], np.int32))
    assert (d["gt_claim"][:, c["gt_crowd"] != 0] == -1).all()
    assert all((d["type"][0] == t).any() for t in (C.TP, C.BG))


@pytest.mark.parametrize("same", [True, False], ids=["same_class", "other_class"])
def test_the_first_maximum_wins_in_every_lane_and_across_box_64(ctx, same):
    c, group = C.tie_case(same)
    d = _check(ctx, c, "tie", class_group=group)
    n = len(C.TIE_PAIRS)
    if same:
        assert d["arg_same"][:n].tolist() == [a for a, _ in C.TIE_PAIRS] and (d["ov_same"][:n] == 0.25).all()
    else:
        assert (d["other_class"][:n] == 1).all() and (d["ov_other"][:n] == 0.25).all() and (d["type"][:, :n] == C.SIM).all()


def test_crowd_boxes_before_between_and_past_position_63(ctx):
    c, crowd = C.crowd_case()
    d = _check(ctx, c, "crowd")
    assert (d["type"][:, :10] == C.IGN).all()                                  # each crowd box matched twice
    assert not np.isin(d["arg_same"], list(crowd)).any() and (d["gt_claim"][:, list(crowd)] == -1).all()
    assert d["arg_same"][10] == 31 and d["type"][0, 10] == C.LOC and d["type"][0, 11] == C.BG


@pytest.mark.parametrize("n", [99, 100, 101, 165])
def test_the_cap_of_100_detections(ctx, n):
    d = _check(ctx, C.cap_case(n), "cap %d" % n)
    assert (d["type"] == -1).sum() == 10 * max(0, n - 100) and (d["type"][:, n - 1] == C.TP).all()
    assert d["type"][0, 0] == (C.TP if n <= 100 else -1) and d["miss"][0].tolist() == [0 if n <= 100 else 1] * 10
    assert d["gt_claim"][0].tolist() == [n - 1, 0 if n <= 100 else -1]


# ----------------------------------------------------------------------------------------------------------- classes
@pytest.mark.parametrize("K", [1, 2, 80, 300])
def test_class_counts_and_groups(ctx, K):
    c = C.class_count_case(K)
    none = _check(ctx, c, "own groups")
    one = _check(ctx, c, "one group", class_group=np.zeros(K, np.int32))
    _check(ctx, c, "several groups", class_group=np.arange(K) % 3)
    assert not (none["type"] == C.SIM).any() and not (one["type"] == C.OTH).any()
    assert np.array_equal(none["type"] == C.OTH, one["type"] == C.SIM)
    if K == 1:
        assert (none["other_class"] == -1).all()
    else:
        assert all((none["type"][0] == t).any() for t in (C.TP, C.DUP, C.LOC, C.OTH, C.BG))


def test_empty_segments_sets_and_classes(ctx):
    box = [0.0, 0.0, 10.0, 10.0]
    cases = {"no_detections": C.pack(3, 2, [], [(0, 0, box, 100.0, 0), (2, 1, box, 100.0, 1)]),
             "no_boxes": C.pack(3, 2, [(0, 0, box, .5), (2, 1, box, .25), (2, 1, box, .75)], []),
             "nothing": C.pack(2, 3, [], []),
             "no_images": dict(zip(C.KEYS, (3, 0, np.zeros((0, 4)), np.zeros(0), np.zeros(1, np.int64), np.zeros((0, 4)),
                                            np.zeros(0), np.zeros(0, np.uint8), np.zeros(1, np.int64))))}
    for name, c in cases.items():
        d = _check(ctx, c, name)
        if name != "no_detections":
            assert (d["prec_fix"] == -1).all() and (d["stats_fix"] == -1).all()
    d = ctx.coco_diag_eval(*C.args(cases["no_detections"]))
    assert d["npos"].tolist() == [1, 0, 0] and (d["prec_fix"][:6, :, :, 0] == 0).all() and (d["prec_fix"][6:] == -1).all()
    assert ctx.coco_diag_eval(0, 5, np.zeros((0, 4)), np.zeros(0), [0], np.zeros((0, 4)), np.zeros(0), np.zeros(0), [0])["ap_fix"].shape == (0, 10, 8)


def test_twenty_thousand_segments(ctx):
    c = C.many_segments_case()
    assert c["n_classes"] * c["n_images"] == 20000
    d = _check(ctx, c, "20000 segments", class_group=np.array([0, 0, 1, 1], np.int32))
    assert all((d["type"][0] == t).any() for t in range(7)) and d["loc_fixed"].any()


def test_a_joint_call_is_the_per_image_calls(ctx):
    c = coco_cases.random_set(3, K=4, N=3)
    group = np.array([0, 0, 1, 2], np.int32)
    whole = _check(ctx, c, "joint", class_group=group)
    tab, miss, npos = np.zeros_like(whole["type_table"]), np.zeros_like(whole["miss"]), np.zeros_like(whole["npos"])
    for i in range(3):
        sub, dr, gr = C.sub_image(c, i)
        one = ctx.coco_diag_eval(*C.args(sub), class_group=group)
        tab += one["type_table"]; miss += one["miss"]; npos += one["npos"]
        for k in ("arg_same", "other_class"):
            assert np.array_equal(one[k], whole[k][dr]), (i, k)
        for k in ("type", "loc_fixed"):
            assert np.array_equal(one[k], whole[k][:, dr]), (i, k)
        for k in ("ov_same", "ov_other"):
            assert np.array_equal(one[k].view(np.uint64), whole[k][dr].view(np.uint64)), (i, k)
        assert np.array_equal(np.where(one["gt_claim"] >= 0, dr[np.maximum(one["gt_claim"], 0)], -1), whole["gt_claim"][:, gr]), i
    assert np.array_equal(tab, whole["type_table"]) and np.array_equal(miss, whole["miss"]) and np.array_equal(npos, whole["npos"])


def test_a_small_call_after_a_large_one_reads_no_stale_scratch(ctx):
    from aznet_hip import ffi
    large, small = C.many_segments_case(), coco_cases.random_set(9, K=3, N=2)
    kw = dict(class_group=np.array([0, 0, 1], np.int32))
    fresh = ffi.AzContext(0)
    try:
        want = fresh.coco_diag_eval(*C.args(small), **kw)
    finally:
        fresh.close()
    for _ in range(2):
        ctx.coco_diag_eval(*C.args(large))
        C.same(ctx.coco_diag_eval(*C.args(small), **kw), want, "after a large call")


# ---------------------------------------------------------------------------------------------- against az_coco_eval
def test_the_plain_variant_is_az_coco_eval_which_keeps_its_bits(ctx):
    for seed in (1, 4, 7):
        c = coco_cases.random_set(seed)
        a = C.args(c)
        before = ctx.coco_eval(*a, want_matches=True)
        got = ctx.coco_diag_eval(*a)
        after = ctx.coco_eval(*a, want_matches=True)
        for k in ("precision", "recall", "stats"):
            assert np.array_equal(before[k].view(np.uint64), after[k].view(np.uint64)), k
        assert np.array_equal(before["dt_match"], after["dt_match"]) and np.array_equal(before["dt_ignore"], after["dt_ignore"])
        assert np.array_equal(got["prec_fix"][0].view(np.uint64), np.ascontiguousarray(before["precision"][:, :, :, 0, 2]).view(np.uint64))
        assert np.array_equal(got["recall_fix"][0].view(np.uint64), np.ascontiguousarray(before["recall"][:, :, 0, 2]).view(np.uint64))
        assert np.array_equal(got["stats_fix"][0], before["stats"][:3])
        m, ig = before["dt_match"][0], before["dt_ignore"][0]
        assert np.array_equal(got["type"] == C.IGN, ig == 1) and np.array_equal(got["type"] == -1, ig == -1)
        assert np.array_equal(got["type"] == C.TP, (m >= 0) & (ig == 0))
        seg0 = np.repeat(c["gt_off"][:-1], np.diff(c["det_off"]))
        for t in range(10):
            tp = np.nonzero(got["type"][t] == C.TP)[0]
            assert np.array_equal(got["gt_claim"][t, seg0[tp] + m[t, tp]], tp) and (got["gt_claim"][t] >= 0).sum() == tp.size


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(ctx):
    from aznet_hip import ffi
    L, h = ctx.L, ctx.h
    c = coco_cases.random_set(2, K=2, N=2)
    K, N, D, G = 2, 2, int(c["det_off"][-1]), int(c["gt_off"][-1])
    db, ds = np.ascontiguousarray(c["det_box"]), np.ascontiguousarray(c["det_score"])
    gb, ga, gc = np.ascontiguousarray(c["gt_box"]), np.ascontiguousarray(c["gt_area"]), np.ascontiguousarray(c["gt_crowd"])
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    u8p, i8p, i64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(ctypes.c_int64)
    outs = [(np.zeros(D), dp), (np.zeros(D, np.int32), ip), (np.zeros(D), dp), (np.zeros(D, np.int32), ip),
            (np.zeros((10, D), np.int8), i8p), (np.zeros((10, D), np.uint8), u8p), (np.zeros((10, G), np.int32), ip),
            (np.zeros(K, np.int64), i64p), (np.zeros((K, 10, 7), np.int64), i64p), (np.zeros((K, 10), np.int64), i64p),
            (np.zeros((8, 10, 101, K)), dp), (np.zeros((8, 10, K)), dp)]
    ms = ctypes.c_float(-7.0)

    def call(nc=K, ni=N, det_off=c["det_off"], gt_off=c["gt_off"], bg=0.1, null=False):
        for a, _ in outs:
            a.view(np.uint8)[...] = 0x5a
        ms.value = -7.0
        do, go = np.asarray(det_off, np.int32), np.asarray(gt_off, np.int32)
        ptrs = [None if null else a.ctypes.data_as(t) for a, t in outs]
        return L.az_coco_diag_eval(h, nc, ni, db.ctypes.data_as(dp), ds.ctypes.data_as(dp), do.ctypes.data_as(ip),
                                   gb.ctypes.data_as(dp), ga.ctypes.data_as(dp), gc.ctypes.data_as(u8p), go.ctypes.data_as(ip),
                                   bg, None, *ptrs, None if null else ctypes.byref(ms))

    def untouched():
        return all((a.view(np.uint8) == 0x5a).all() for a, _ in outs) and ms.value == -7.0

    assert call() == ffi.AZ_OK and not untouched() and ms.value >= 0.0
    assert np.array_equal(outs[4][0], C.diag(*C.args(c))["type"])
    assert call(null=True) == ffi.AZ_OK and untouched()                      # every output may be NULL
    shift, desc = c["det_off"].copy(), c["det_off"].copy()
    shift[0] = 1
    desc[1], desc[2] = desc[2] + 1, desc[1]
    refused = [(dict(det_off=shift), ffi.AZ_ERR_INVALID), (dict(det_off=desc), ffi.AZ_ERR_INVALID),
               (dict(gt_off=np.r_[1, c["gt_off"][1:]]), ffi.AZ_ERR_INVALID), (dict(nc=-1), ffi.AZ_ERR_INVALID),
               (dict(nc=1 << 16, ni=1 << 15), ffi.AZ_ERR_CAPACITY), (dict(bg=float("nan")), ffi.AZ_ERR_INVALID),
               (dict(bg=-0.01), ffi.AZ_ERR_INVALID), (dict(bg=np.nextafter(0.5, 1.0)), ffi.AZ_ERR_INVALID)]
    for kw, code in refused:
        assert call(**kw) == code and untouched(), kw
    assert call(bg=0.5) == ffi.AZ_OK and not untouched()                    # the context is still usable
    with pytest.raises(ffi.AzError) as e:
        ctx.coco_diag_eval(*C.args(c), bg_overlap=0.6)
    assert e.value.code == ffi.AZ_ERR_INVALID and "bg_overlap" in str(e.value)


# ------------------------------------------------------------------------------------------------------- front door
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


def test_the_tool_reports_the_ap_eval_det_prints(ctx, tmp_path):
    from datasets import coco_eval
    from datasets.coco import coco
    devkit = coco_cases.make_devkit(tmp_path / "data" / "COCO")
    db = coco("val", "2014", devkit)
    pkl = tmp_path / "detections.pkl"
    with open(str(pkl), "wb") as f:
        pickle.dump(_all_boxes(db), f, pickle.HIGHEST_PROTOCOL)
    runs = {}
    for tool, extra in (("diagnose_det.py", ["--protocol", "coco"]), ("eval_det.py", [])):
        # the factory's devkit is <ROOT_DIR>/data/COCO; a fresh process with ROOT_DIR at tmp_path
        argv = [tool, str(pkl), "--imdb", "coco_2014_val", "--no-nms", "--out", str(tmp_path / tool[:-3])] + extra
        code = ("import _init_paths, sys, runpy, datasets; datasets.ROOT_DIR = %r; sys.argv = %r;"
                "runpy.run_path(%r, run_name='__main__')" % (str(tmp_path), argv, os.path.join(TOOLS, tool)))
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=TOOLS, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        runs[tool] = p.stdout
    assert "IoU .50:.95" in runs["diagnose_det.py"] and "wrote" in runs["diagnose_det.py"]
    assert os.listdir(str(tmp_path / "diagnose_det")) == ["det_diagnosis_coco.pkl"]          # and no results file
    with open(str(tmp_path / "diagnose_det" / "det_diagnosis_coco.pkl"), "rb") as f:
        d = pickle.load(f)
    # eval_det.py's numbers: its results file evaluated as it evaluated it, and the three lines it printed
    r = coco_eval.evaluate_results_file(db._coco[0], str(tmp_path / "eval_det" / "instances_val2014_results.json"), ctx=ctx)
    assert np.array_equal(d["stats_fix"][0].view(np.uint64), r["stats"][:3].view(np.uint64))
    assert 0 < d["stats_fix"][0, 0] < 1 and d["protocol"] == "coco" and d["type"].shape[0] == 10
    lines = [ln for ln in runs["eval_det.py"].splitlines() if ln.startswith(" Average Precision")]
    assert lines[:3] == coco_eval.summary_lines(np.r_[d["stats_fix"][0], np.zeros(9)])[:3]


def test_the_tool_diagnoses_the_synthetic_imdb_without_files(tmp_path):
    from datasets.factory import get_imdb
    imdb = get_imdb("synthetic_375x500_4")
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(imdb.num_images)] for _ in range(imdb.num_classes)]
    for i, e in enumerate(imdb.gt_roidb()):
        for b, k in zip(e["boxes"].astype(np.float32), e["gt_classes"]):
            all_boxes[k][i] = np.vstack([all_boxes[k][i], np.r_[b, 0.9].astype(np.float32)[None],
                                         np.r_[b[0] + 30, b[1], b[2] + 30, b[3], 0.5].astype(np.float32)[None]])
    pkl = tmp_path / "detections.pkl"
    with open(str(pkl), "wb") as f:
        pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(TOOLS, "diagnose_det.py"), str(pkl), "--imdb",
                        "synthetic_375x500_4", "--no-nms", "--protocol", "coco", "--out", str(tmp_path / "out")], cwd=TOOLS,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "IoU .50:.95" in p.stdout and "Detections by type at IoU 0.75" in p.stdout and "top-ranked" not in p.stdout
    with open(str(tmp_path / "out" / "det_diagnosis_coco.pkl"), "rb") as f:
        d = pickle.load(f)
    n_obj = sum(len(e["gt_classes"]) for e in imdb.gt_roidb())
    assert d["npos"].sum() == n_obj and (d["type"][0] == C.TP).sum() == n_obj and d["miss"].sum() == 0
    assert d["stats_fix"][7, 0] > 0.999999 and (d["type"][0] != C.TP).sum() == n_obj
