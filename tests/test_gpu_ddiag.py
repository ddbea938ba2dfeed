"""GPU: az_det_diag_eval ("Detection diagnosis") against the NumPy restatement tests/ddiag_ref.py -- every
integer output and both overlaps bit for bit, ap_fix bit for bit under the 11-point metric and to 1e-12 under the area
metric (the bound test_gpu_voc_eval.py holds ap_auc to) -- at the kernels' wave, chunk, class-count, threshold and cut
edges, against az_voc_eval on the same inputs, its refusals, and detect.diagnose_det / tools/diagnose_det.py end to end."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import ddiag_ref as R
import eval_edges_cases as E
import voc_cases

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
INT_KEYS = ("type", "arg_same", "other_class", "loc_fixed", "gt_claim", "type_table", "miss", "fp_at", "npos")
PERFECT_11 = voc_cases._sum11([1.0] * 11)


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, m07, what=""):
    for k in INT_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    for k in ("ov_same", "ov_other"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)
    if m07:
        assert np.array_equal(got["ap_fix"], want["ap_fix"], equal_nan=True), (what, got["ap_fix"], want["ap_fix"])
    else:
        assert np.array_equal(np.isnan(got["ap_fix"]), np.isnan(want["ap_fix"])), what
        np.testing.assert_allclose(got["ap_fix"], want["ap_fix"], rtol=1e-12, atol=0, equal_nan=True, err_msg=what)


def _check(ctx, case, what="", metrics=(True, False), **kw):
    out = None
    for m07 in metrics:
        got = ctx.det_diag_eval(*case, metric_07=m07, **kw)
        _same(got, R.diag_flat(*case, metric_07=m07, **kw), m07, what)
        out = got
    return out


# ------------------------------------------------------------------------------------------------------------ layout
def test_a_joint_call_is_the_per_image_calls(ctx):
    case = R.random_case(4, 3, 11, n_det=(1, 7))
    group, cuts = np.array([0, 0, 1, 2], np.int32), (0.5, 1, 2)
    # cuts count rows of the whole class: the tables of the cuts are not additive, every other table is
    whole = _check(ctx, case, "joint", class_group=group, cuts=cuts)
    tab, miss, npos = np.zeros_like(whole["type_table"]), np.zeros_like(whole["miss"]), np.zeros_like(whole["npos"])
    for i in range(3):
        sub, dr, gr = R.sub_image(case, i)
        one = ctx.det_diag_eval(*sub, class_group=group)
        tab += one["type_table"]; miss += one["miss"]; npos += one["npos"]
        for k in ("type", "arg_same", "other_class", "loc_fixed"):
            assert np.array_equal(one[k], whole[k][dr]), (i, k)
        for k in ("ov_same", "ov_other"):
            assert np.array_equal(_bits(one[k]), _bits(whole[k][dr])), (i, k)
        claim = whole["gt_claim"][gr]
        assert np.array_equal(np.where(one["gt_claim"] >= 0, dr[np.maximum(one["gt_claim"], 0)], -1), claim), i
    assert np.array_equal(tab, whole["type_table"]) and np.array_equal(miss, whole["miss"]) and np.array_equal(npos, whole["npos"])


def test_empty_sets_classes_and_a_class_without_positives(ctx):
    box = R.grid_box(0)
    cases = {
        "no_detections": R.pack(3, 2, [], [(0, 0, box, 0), (2, 1, box, 1)]),
        "no_boxes": R.pack(3, 2, [(0, 0, box, 0.5), (2, 1, box, 0.25), (2, 1, box, 0.75)], []),
        "nothing": R.pack(2, 3, [], []),
        "no_images": (3, 0, np.zeros((0, 4)), np.zeros(0), np.zeros(1, np.int64), np.zeros((0, 4)), np.zeros(0, np.uint8),
                      np.zeros(1, np.int64)),
        # class 1 empty; class 2 has only difficult boxes (npos = 0) and detections on and off them
        "npos0": R.pack(4, 2, [(0, 0, box, 0.9), (2, 0, box, 0.8), (2, 1, R.shifted(box, 0.6), 0.7), (2, 1, R.grid_box(7), 0.6),
                               (3, 1, box, 0.5)],
                        [(0, 0, box, 0), (2, 0, box, 1), (2, 1, box, 1), (3, 0, box, 0)]),
    }
    for name, case in cases.items():
        got = _check(ctx, case, name, cuts=(0.0, 1.0, 3.0))
        if name in ("no_detections", "nothing", "no_images"):
            assert got["type_table"].sum() == 0 and got["fp_at"].sum() == 0 and not np.isnan(got["ap_fix"]).any()
    got = ctx.det_diag_eval(*cases["npos0"], metric_07=False)
    assert got["npos"].tolist() == [1, 0, 0, 1] and got["type_table"][2].tolist() == [1, 0, 0, 1, 0, 0, 1]
    assert got["loc_fixed"].sum() == 0 and np.isnan(got["ap_fix"][2]).all()
    assert ctx.det_diag_eval(0, 5, np.zeros((0, 4)), np.zeros(0), [0], np.zeros((0, 4)), np.zeros(0), [0])["ap_fix"].shape == (0, 8)


# -------------------------------------------------------------------------------------------------------- wave edges
@pytest.mark.parametrize("n_det,n_gt", [(1, 65), (63, 65), (64, 65), (65, 65), (129, 65), (65, 1), (65, 63), (65, 64), (65, 130)])
def test_segment_and_image_sizes_round_the_wave(ctx, n_det, n_gt):
    case = R.wave_case(n_det, n_gt)
    got = _check(ctx, case, "wave", class_group=np.array([0, 0, 1], np.int32), cuts=(0.5, 2.0))
    assert int(np.diff(case[4])[1]) == n_det and int(case[7][-1]) == n_gt
    if n_det >= 63 and n_gt >= 63:
        assert all((got["type"] == t).any() for t in (R.TP, R.LOC, R.BG)) and ((got["type"] == R.SIM) | (got["type"] == R.OTH)).any()


@pytest.mark.parametrize("same", [True, False], ids=["same_class", "other_class"])
def test_the_first_maximum_wins_in_every_lane_and_across_box_64(ctx, same):
    case, group, keep = R.tie_case(same)
    assert (63, 64) in keep and (5, 69) in keep and len(keep) == len(R.TIE_PAIRS)
    got = _check(ctx, case, "tie", class_group=group)
    k = np.arange(len(keep))
    first = np.array([a for a, _ in keep])
    if same:
        assert np.array_equal(got["arg_same"][k], first) and set(got["type"][k].tolist()) == {R.TP, R.IGN}
        assert np.array_equal(np.sort(got["arg_same"][len(keep):]), np.setdiff1d(np.arange(130), np.array(keep).ravel()))
    else:
        assert np.array_equal(got["other_class"][k], 1 + first) and set(got["type"][k].tolist()) == {R.SIM, R.OTH}


# ----------------------------------------------------------------------------------------------------------- classes
@pytest.mark.parametrize("C", [1, 2, 21, 256, 300])
def test_class_counts_and_groups(ctx, C):
    case = R.class_count_case(C)
    none = _check(ctx, case, "own groups", metrics=(True,), cuts=(1.0,))
    one = _check(ctx, case, "one group", metrics=(True,), class_group=np.zeros(C, np.int32))
    assert not (none["type"] == R.SIM).any() and not (one["type"] == R.OTH).any()
    assert np.array_equal(none["type"] == R.OTH, one["type"] == R.SIM)
    if C == 1:
        assert (none["other_class"] == -1).all() and not (none["type"] == R.OTH).any()
    else:
        assert (none["type"] == R.OTH).any() and all((none["type"] == t).any() for t in (R.TP, R.DUP, R.LOC, R.BG))
    if C > 2:
        assert (none["type"] == R.IGN).any()


def test_voc_groups_and_the_lower_class_wins_a_tie(ctx):
    case = R.random_case(20, 3, 5, n_det=(0, 4), n_gt=(0, 2))
    got = _check(ctx, case, "voc groups", class_group=R.VOC_GROUPS)
    assert (got["type"] == R.SIM).any() and (got["type"] == R.OTH).any()
    tie = _check(ctx, R.other_tie_case(), "other tie")
    assert tie["other_class"].tolist() == [1, -1, 3, 1]


# -------------------------------------------------------------------------------------------------------- thresholds
def test_overlaps_exactly_on_the_thresholds(ctx):
    case = R.threshold_case()
    up5, up1 = np.nextafter(0.5, 1.0), np.nextafter(0.1, 1.0)
    want = {(0.5, 0.1): [R.TP, R.LOC, R.OTH, R.BG], (up5, 0.1): [R.LOC, R.LOC, R.OTH, R.BG], (0.5, up1): [R.TP, R.BG, R.BG, R.BG],
            (0.5, 0.0): [R.TP, R.LOC, R.OTH, R.BG], (0.5, 0.5): [R.TP, R.BG, R.BG, R.BG], (0.1, 0.1): [R.TP, R.TP, R.OTH, R.BG]}
    for (mo, bg), types in want.items():
        got = _check(ctx, case, "thresholds %r %r" % (mo, bg), min_overlap=mo, bg_overlap=bg)
        assert got["type"].tolist() == types, (mo, bg)
        assert got["ov_same"][:2].tolist() == [0.5, 0.1] and got["ov_other"][2] == 0.1
        if bg == mo:
            assert not (got["type"] == R.LOC).any()


def test_difficult_boxes(ctx):
    got = _check(ctx, R.difficult_case(), "difficult")
    assert got["type"].tolist() == [R.IGN, R.LOC, R.OTH] and got["loc_fixed"].tolist() == [0, 0, 0]
    assert got["gt_claim"].tolist() == [-1, -1] and got["miss"].tolist() == [0, 0]


def test_claims_across_chunks_of_64_detections(ctx):
    got = _check(ctx, R.chunk_case(), "chunks")
    assert got["type"][[3, 70, 5, 69, 2, 100]].tolist() == [R.TP, R.DUP, R.LOC, R.LOC, R.LOC, R.TP]
    assert got["loc_fixed"][[5, 69, 2]].tolist() == [1, 0, 0] and got["loc_fixed"].sum() == 1
    assert got["gt_claim"].tolist() == [3, -1, 100, -1] and got["miss"].tolist() == [2]


def test_tied_nan_and_infinite_confidences(ctx):
    _check(ctx, R.score_case(), "scores", cuts=(0.5, 1.0))
    _check(ctx, E.voc_score_edge_case(), "voc score edges", cuts=(0.5, 1.0))


# -------------------------------------------------------------------------------------------------------------- cuts
def test_cuts(ctx):
    case = R.cuts_case()
    got = _check(ctx, case, "cut edges", cuts=R.CUTS_EDGE)
    assert got["fp_at"][0].sum(1).tolist() == [0, 2, 2, 4, 9, 10, 10, 10]
    assert np.array_equal(got["fp_at"][0, -1], got["type_table"][0])
    assert _check(ctx, case, "no cuts")["fp_at"].shape == (1, 0, 7)
    got = _check(ctx, R.random_case(3, 4, 16), "16 cuts", cuts=np.linspace(0.0, 3.0, 16))
    assert got["fp_at"].shape == (3, 16, 7) and (np.diff(got["fp_at"].sum(2), axis=1) >= 0).all()


# ----------------------------------------------------------------------------------------------------- many segments
def test_twenty_thousand_segments(ctx):
    case = R.many_segments_case()
    got = _check(ctx, case, "20000 segments", metrics=(True,), class_group=np.array([0, 0, 1, 1], np.int32), cuts=(0.5, 1.0))
    assert case[0] * case[1] == 20000 and all((got["type"] == t).any() for t in range(7)) and got["loc_fixed"].any()


# ---------------------------------------------------------------------------------------------- against az_voc_eval
@pytest.mark.parametrize("name", ["random", "curves"])
def test_the_plain_variant_is_az_voc_eval(ctx, name):
    case = R.random_case(4, 6, 3) if name == "random" else E.voc_class_curve_case()
    for m07 in (True, False):
        before = ctx.voc_eval(*case, min_overlap=0.5, metric_07=m07)
        got = ctx.det_diag_eval(*case, metric_07=m07, cuts=(1.0,))
        after = ctx.voc_eval(*case, min_overlap=0.5, metric_07=m07)
        for k in ("match", "npos"):
            assert np.array_equal(before[k], after[k])
        for k in ("rec", "prec", "ap", "ap_auc"):
            assert np.array_equal(_bits(before[k]), _bits(after[k])), k
        assert np.array_equal(R.to_match(got["type"]), before["match"]) and np.array_equal(got["npos"], before["npos"])
        if m07:
            assert np.array_equal(_bits(got["ap_fix"][:, 0]), _bits(before["ap"]))
        else:
            np.testing.assert_allclose(got["ap_fix"][:, 0], before["ap"], rtol=1e-12, atol=0, equal_nan=True)
    if name == "curves":
        _same(ctx.det_diag_eval(*case, cuts=(1.0,)), R.diag_flat(*case, cuts=(1.0,)), True, "curves")


def test_a_small_call_after_a_large_one_reads_no_stale_scratch(ctx):
    from aznet_hip import ffi
    large, small = R.many_segments_case(), R.random_case(3, 2, 9)
    kw = dict(class_group=np.array([0, 0, 1], np.int32), cuts=(0.5, 1.0, 2.0))
    fresh = ffi.AzContext(0)
    try:
        want = fresh.det_diag_eval(*small, **kw)
    finally:
        fresh.close()
    for _ in range(2):
        ctx.det_diag_eval(*large, cuts=(1.0,))
        got = ctx.det_diag_eval(*small, **kw)
        for k in INT_KEYS:
            assert np.array_equal(got[k], want[k]), k
        for k in ("ov_same", "ov_other", "ap_fix"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(ctx):
    from aznet_hip import ffi
    L, h = ctx.L, ctx.h
    C, N, db, dc, doff, gb, gd, goff = R.random_case(2, 2, 1)
    D, G = int(doff[-1]), int(goff[-1])
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    u8p, i64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)
    outs = {"type": np.zeros(D, np.int8), "ov_same": np.zeros(D), "arg_same": np.zeros(D, np.int32), "ov_other": np.zeros(D),
            "other_class": np.zeros(D, np.int32), "loc_fixed": np.zeros(D, np.uint8), "gt_claim": np.zeros(G, np.int32),
            "type_table": np.zeros((C, 7), np.int64), "miss": np.zeros(C, np.int64), "fp_at": np.zeros((C, 16, 7), np.int64),
            "npos": np.zeros(C, np.int64), "ap_fix": np.zeros((C, 8))}
    ms = ctypes.c_float(-7.0)

    def call(nc=C, ni=N, det_off=doff, gt_off=goff, mo=0.5, bg=0.1, cuts=(0.5, 1.0), n_cuts=None, null=False):
        for a in outs.values():
            a.view(np.uint8)[...] = 0x5a
        ms.value = -7.0
        do, go = np.asarray(det_off, np.int32), np.asarray(gt_off, np.int32)
        ct = np.asarray(cuts, np.float64)
        ptr = (lambda a, t: None) if null else (lambda a, t: a.ctypes.data_as(t))
        return L.az_det_diag_eval(
            h, nc, ni, db.ctypes.data_as(dp), dc.ctypes.data_as(dp), do.ctypes.data_as(ip), gb.ctypes.data_as(dp),
            gd.ctypes.data_as(u8p), go.ctypes.data_as(ip), mo, bg, 1, None, ct.ctypes.data_as(dp),
            ct.size if n_cuts is None else n_cuts, ptr(outs["type"], ctypes.POINTER(ctypes.c_int8)), ptr(outs["ov_same"], dp),
            ptr(outs["arg_same"], ip), ptr(outs["ov_other"], dp), ptr(outs["other_class"], ip), ptr(outs["loc_fixed"], u8p),
            ptr(outs["gt_claim"], ip), ptr(outs["type_table"], i64p), ptr(outs["miss"], i64p), ptr(outs["fp_at"], i64p),
            ptr(outs["npos"], i64p), ptr(outs["ap_fix"], dp), None if null else ctypes.byref(ms))

    def untouched():
        return all((a.view(np.uint8) == 0x5a).all() for a in outs.values()) and ms.value == -7.0

    assert call() == ffi.AZ_OK and not untouched() and ms.value >= 0.0
    assert np.array_equal(outs["type"], R.diag_flat(C, N, db, dc, doff, gb, gd, goff)["type"])
    assert call(null=True) == ffi.AZ_OK and untouched()                      # every output may be NULL
    nan = float("nan")
    shift, desc = doff.copy(), doff.copy()
    shift[0] = 1
    desc[1], desc[2] = desc[2] + 1, desc[1]
    refused = [
        (dict(det_off=shift), ffi.AZ_ERR_INVALID), (dict(det_off=desc), ffi.AZ_ERR_INVALID),
        (dict(gt_off=np.r_[1, goff[1:]]), ffi.AZ_ERR_INVALID), (dict(nc=-1), ffi.AZ_ERR_INVALID),
        (dict(nc=65536, ni=65536), ffi.AZ_ERR_CAPACITY),
        (dict(mo=nan), ffi.AZ_ERR_INVALID), (dict(bg=nan), ffi.AZ_ERR_INVALID), (dict(bg=-0.01), ffi.AZ_ERR_INVALID),
        (dict(bg=np.nextafter(0.5, 1.0)), ffi.AZ_ERR_INVALID), (dict(cuts=np.linspace(0, 1, 17)), ffi.AZ_ERR_INVALID),
        (dict(cuts=(-0.5, 1.0)), ffi.AZ_ERR_INVALID), (dict(cuts=(0.5, nan)), ffi.AZ_ERR_INVALID),
        (dict(cuts=(0.5, float("inf"))), ffi.AZ_ERR_INVALID),
        (dict(cuts=(1.0, 0.5)), ffi.AZ_ERR_INVALID), (dict(n_cuts=-1), ffi.AZ_ERR_INVALID),
    ]
    for kw, code in refused:
        assert call(**kw) == code and untouched(), kw
    assert call(bg=0.5, cuts=(1.0, 1.0)) == ffi.AZ_OK and not untouched()    # the context is still usable; equal cuts ascend
    with pytest.raises(ffi.AzError) as e:
        ctx.det_diag_eval(C, N, db, dc, doff, gb, gd, goff, bg_overlap=0.6)
    assert e.value.code == ffi.AZ_ERR_INVALID and "bg_overlap" in str(e.value)


# ------------------------------------------------------------------------------------------------------- front door
def _planted(imdb):
    """all_boxes of the synthetic imdb: the ground truth itself at score 0.9 and, at lower scores, for every object
    whose class is alone in its image the same box moved right by 60 % of its width (LOC), for every image a copy of
    an object under a class the image does not hold (OTH: the synthetic classes are each on their own) and a far-away
    box (BG).  -> (gt only, with the plants, the plants' (class, image, row, type))."""
    roidb = imdb.gt_roidb()
    nc, ni = imdb.num_classes, imdb.num_images
    only = [[np.zeros((0, 5), np.float32) for _ in range(ni)] for _ in range(nc)]
    for i, e in enumerate(roidb):
        for b, k in zip(e["boxes"].astype(np.float32), e["gt_classes"]):
            only[k][i] = np.vstack([only[k][i], np.r_[b, 0.9].astype(np.float32)[None]])
    full = [[a.copy() for a in row] for row in only]
    plants = []

    def add(k, i, box, score, ty):
        plants.append((k, i, full[k][i].shape[0], ty))
        full[k][i] = np.vstack([full[k][i], np.r_[box, score].astype(np.float32)[None]])
    for i, e in enumerate(roidb):
        cls = e["gt_classes"].tolist()
        for b, k in zip(e["boxes"].astype(np.float64), cls):
            if cls.count(k) == 1:
                s = round(0.6 * (b[2] - b[0] + 1))
                add(k, i, [b[0] + s, b[1], b[2] + s, b[3]], 0.5, R.LOC)
        free = next(k for k in range(1, nc) if k not in cls)
        add(free, i, e["boxes"][0].astype(np.float64), 0.4, R.OTH)
        add(cls[0], i, [5000.0, 5000.0, 5050.0, 5050.0], 0.3, R.BG)
    return only, full, plants


def test_diagnose_on_the_synthetic_imdb_with_planted_detections(ctx):
    from datasets.factory import get_imdb
    from detect import diagnose_det as DD
    imdb = get_imdb("synthetic_375x500_4")
    only, full, plants = _planted(imdb)
    d = DD.diagnose(imdb, only, ctx=ctx)
    n_obj = sum(len(e["gt_classes"]) for e in imdb.gt_roidb())
    assert d["type"].size == n_obj and (d["type"] == R.TP).all() and d["miss"].sum() == 0 and d["npos"].sum() == n_obj
    has = d["npos"] > 0
    assert (d["ap_fix"][has] == PERFECT_11).all() and (d["ap_fix"][~has, 0] == 0).all() and d["miss_by_size"].sum() == 0
    d = DD.diagnose(imdb, full, ctx=ctx)
    N = imdb.num_images
    assert any(p[3] == R.LOC for p in plants) and d["type"].size == n_obj + len(plants)
    for k, i, row, ty in plants:
        assert d["type"][d["det_off"][(k - 1) * N + i] + row] == ty, (k, i, row, ty)
    assert (d["type"] == R.TP).sum() == n_obj and d["confusion"].sum() == N and d["loc_fixed"].sum() == 0
    assert d["class_group"] is None and len(DD.summary_lines(d)) > 30


def test_the_tool_reports_the_ap_eval_det_prints(tmp_path):
    import scipy.io as sio
    from datasets.factory import get_imdb
    imdb = get_imdb("synthetic_375x500_4")
    _, full, _ = _planted(imdb)
    det = tmp_path / "detections.pkl"
    with open(det, "wb") as f:
        pickle.dump(full, f, pickle.HIGHEST_PROTOCOL)
    runs = {}
    for tool in ("diagnose_det.py", "eval_det.py"):
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(TOOLS, tool), str(det), "--imdb",
                            "synthetic_375x500_4", "--no-nms", "--out", str(tmp_path / tool[:-3])], cwd=TOOLS,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        runs[tool] = p.stdout
    assert "Detections by type" in runs["diagnose_det.py"] and "wrote" in runs["diagnose_det.py"]
    with open(tmp_path / "diagnose_det" / "det_diagnosis.pkl", "rb") as f:
        d = pickle.load(f)
    lines = [ln for ln in runs["eval_det.py"].splitlines() if ln.startswith("!!! class")]
    assert len(lines) == 20 == len(d["classes"])
    for k, c in enumerate(d["classes"]):
        assert lines[k].split()[1] == c and lines[k].split()[3] == "%.4f" % d["ap_fix"][k, 0]
        saved = float(sio.loadmat(str(tmp_path / "eval_det" / (c + "_pr.mat")))["ap"][0, 0])
        assert saved == d["ap_fix"][k, 0], c
    assert (d["ap_fix"][:, 0] > 0).any() and (d["ap_fix"][:, 0] < 1).any()
