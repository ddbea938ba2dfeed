"""CPU: the detection diagnosis off the device -- the NumPy restatement (tests/ddiag_ref.py) against the VOC evaluation's
restatement and against a hand-worked set whose answers are written out here, the binding's argument checks, the header,
the tool's parser, and detect.diagnose_det's host-side tables on a stub context."""
import os
import re
import sys
from fractions import Fraction as Fr

import numpy as np
import pytest

import ddiag_ref as R
import voc_cases
import voc_eval_ref as V
from helpers import GOLDEN

REPO = os.path.dirname(os.path.dirname(GOLDEN))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
# a perfect 11-point AP in VOCevaldet's arithmetic (ap = ap + p / 11, eleven times): 1 + 2^-52, as voc_cases has it
PERFECT_11 = voc_cases._sum11([1.0] * 11)


def _flat(gt, dets):
    """A voc_cases case (one class) in the flat layout."""
    return R.pack(1, len(gt), [(0, i, b, s) for i, s, b in dets], [(0, i, b, d) for i, g in enumerate(gt) for b, d in g])


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _same_as_voc(case, **kw):
    for m07 in (True, False):
        ref = V.evaluate_flat(*case, metric_07=m07, **{k: v for k, v in kw.items() if k == "min_overlap"})
        got = R.diag_flat(*case, metric_07=m07, **kw)
        assert np.array_equal(R.to_match(got["type"]), ref["match"])
        assert np.array_equal(got["npos"], ref["npos"])
        assert np.array_equal(_bits(got["ap_fix"][:, 0]), _bits(ref["ap"]))
        # the plain claims are the evaluation's: a box is claimed exactly when one TP names it
        tp = np.nonzero(got["type"] == R.TP)[0]
        assert sorted(got["gt_claim"][got["gt_claim"] >= 0].tolist()) == sorted(tp.tolist())


@pytest.mark.parametrize("name", [c[0] for c in voc_cases.CASES])
def test_variant_0_and_the_types_are_the_voc_evaluation_on_its_cases(name):
    _, gt, dets, want = next(c for c in voc_cases.CASES if c[0] == name)
    case = _flat(gt, dets)
    _same_as_voc(case)
    got = R.diag_flat(*case)
    assert R.to_match(got["type"]).tolist() == want["match"] and int(got["npos"][0]) == want["npos"]


@pytest.mark.parametrize("seed", range(6))
def test_variant_0_and_the_types_are_the_voc_evaluation_on_random_sets(seed):
    case = R.random_case(4, 6, seed)
    _same_as_voc(case, class_group=np.array([0, 0, 1, 1]), cuts=(0.5, 1, 2))
    _same_as_voc(case, min_overlap=0.3, bg_overlap=0.3)
    got = R.diag_flat(*case, class_group=np.array([0, 0, 1, 1]))
    assert all((got["type"] == t).any() for t in range(7)) and got["loc_fixed"].any() and got["miss"].all()
    assert np.array_equal(got["type_table"].sum(1), np.diff(case[4][::6]))


@pytest.mark.parametrize("seed", range(6))
def test_variant_7_is_a_perfect_ap(seed):
    case = R.random_case(4, 6, seed, p_diff=0.1)
    for m07 in (True, False):
        got = R.diag_flat(*case, metric_07=m07)
        for c in range(4):
            tps = int(got["type_table"][c, R.TP])
            lo, hi = case[4][c * 6], case[4][(c + 1) * 6]
            if tps + int(got["loc_fixed"][lo:hi].sum()) == 0:
                continue
            # precision 1 at every recall: the area is exactly 1.0, the 11-point sum VOCevaldet's own value of eleven 1 / 11
            assert got["ap_fix"][c, 7] == (PERFECT_11 if m07 else 1.0), (c, m07)
            assert got["ap_fix"][c, 6] >= got["ap_fix"][c, 0] or tps == 0


def test_hand_worked_set():
    """3 classes x 2 images, 12 detections (ddiag_ref.hand_case draws the boxes); every number below is worked by hand."""
    case, group = R.hand_case()
    s11 = voc_cases._sum11
    for m07 in (True, False):
        got = R.diag_flat(*case, metric_07=m07, class_group=group, cuts=(0.5, 1, 2))
        #                              d0  d1  d2  d3  d4  d5  d6  d7  d8  d9 d10 d11
        assert got["type"].tolist() == [1, 2, 0, 3, 3, 4, 5, 6, 1, 5, 3, 1]
        assert got["loc_fixed"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0]
        assert got["arg_same"].tolist() == [0, 0, 1, 2, 2, -1, -1, -1, 0, -1, 0, 0]
        assert got["other_class"].tolist() == [-1, -1, -1, -1, -1, 1, 2, -1, -1, 2, -1, -1]
        assert got["ov_same"].tolist() == [1.0, 1.0, 1.0, 50.0 / 150.0, 40.0 / 160.0, 0.0, 0.0, 0.0, 0.5, 0.0, 60.0 / 140.0, 1.0]
        assert got["ov_other"].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
        # boxes: A, B (difficult), E | G0 | C | F | H (difficult)
        assert got["gt_claim"].tolist() == [0, -1, -1, 8, -1, 11, -1]
        assert got["npos"].tolist() == [3, 1, 1] and got["miss"].tolist() == [1, 1, 0]
        #                                      IGN TP DUP LOC SIM OTH BG
        assert got["type_table"].tolist() == [[1, 2, 1, 2, 1, 2, 1], [0, 0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0]]
        # class 0 in rank order: d8 d0 d1 d2 d3 d4 ...; its cuts hold floor(1.5) = 1, 3 and 6 rows
        assert got["fp_at"][0].tolist() == [[0, 1, 0, 0, 0, 0, 0], [0, 2, 1, 0, 0, 0, 0], [1, 2, 1, 2, 0, 0, 0]]
        assert got["fp_at"][1].tolist() == [[0] * 7, [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0]]
        assert got["fp_at"][2].tolist() == [[0] * 7, [0, 1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0]]
        ap = got["ap_fix"]
        if m07:
            # class 0: recall 2/3 at precision 1; with E found by d3 recall 1 at precision 3/4 (d1 is still a false positive)
            c0 = s11([1.0] * 7 + [0.0] * 4)
            want = [[c0, c0, s11([1.0] * 7 + [0.75] * 4), c0, c0, c0, PERFECT_11, PERFECT_11],
                    [0.0, 0.0, PERFECT_11, 0.0, 0.0, 0.0, 0.0, PERFECT_11],      # class 1: one LOC; no TP: variant 6 selects 0
                    [PERFECT_11] * 8]
            assert ap.tolist() == want
            assert abs(ap[0, 2] - float(Fr(10, 11))) < 1e-15 and abs(ap[0, 0] - float(Fr(7, 11))) < 1e-15
        else:
            want = [[Fr(2, 3), Fr(2, 3), Fr(11, 12), Fr(2, 3), Fr(2, 3), Fr(2, 3), Fr(1), Fr(1)],
                    [Fr(0), Fr(0), Fr(1), Fr(0), Fr(0), Fr(0), None, Fr(1)],     # no TP: 0 / 0 recall, NaN
                    [Fr(1)] * 8]
            for c in range(3):
                for v in range(8):
                    if want[c][v] is None:
                        assert np.isnan(ap[c, v])
                    else:
                        assert abs(ap[c, v] - float(want[c][v])) <= 2.0 ** -52, (c, v)


def test_case_builders_hold_what_they_promise():
    c = R.diag_flat(*R.chunk_case())
    assert c["type"][[3, 70, 5, 69, 2, 100]].tolist() == [R.TP, R.DUP, R.LOC, R.LOC, R.LOC, R.TP]
    assert c["loc_fixed"][[5, 69, 2]].tolist() == [1, 0, 0] and c["miss"].tolist() == [2] and c["gt_claim"].tolist() == [3, -1, 100, -1]
    t = R.threshold_case()
    up5, up1 = np.nextafter(0.5, 1.0), np.nextafter(0.1, 1.0)
    a = R.diag_flat(*t)
    assert a["ov_same"][:2].tolist() == [0.5, 0.1] and a["ov_other"][2] == 0.1
    assert a["type"].tolist() == [R.TP, R.LOC, R.OTH, R.BG]
    assert R.diag_flat(*t, min_overlap=up5)["type"].tolist() == [R.LOC, R.LOC, R.OTH, R.BG]
    assert R.diag_flat(*t, bg_overlap=up1)["type"].tolist() == [R.TP, R.BG, R.BG, R.BG]
    assert R.diag_flat(*t, bg_overlap=0.0)["type"].tolist() == [R.TP, R.LOC, R.OTH, R.BG]
    assert R.diag_flat(*t, bg_overlap=0.5)["type"].tolist() == [R.TP, R.BG, R.BG, R.BG]
    d = R.diag_flat(*R.difficult_case())
    assert d["type"].tolist() == [R.IGN, R.LOC, R.OTH] and d["loc_fixed"].tolist() == [0, 0, 0]
    for same in (True, False):
        case, group, keep = R.tie_case(same)
        got = R.diag_flat(*case, class_group=group)
        for k, (a_, b_) in enumerate(keep):
            if same:                                   # the first of the two copies decides: difficult or not
                assert got["arg_same"][k] == a_ and got["type"][k] == (R.TP if k % 2 == 0 else R.IGN)
            else:
                assert got["other_class"][k] == 1 + a_ and got["type"][k] == (R.SIM if k % 2 == 0 else R.OTH)
    o = R.diag_flat(*R.other_tie_case())
    assert o["other_class"].tolist() == [1, -1, 3, 1] and o["type"].tolist() == [R.OTH, R.TP, R.IGN, R.OTH]
    cc = R.diag_flat(*R.cuts_case(), cuts=R.CUTS_EDGE)
    assert cc["fp_at"][0].sum(1).tolist() == [0, 2, 2, 4, 9, 10, 10, 10] and cc["npos"].tolist() == [4]
    s = R.score_case()
    assert np.isnan(s[3]).sum() == 2 and np.isinf(s[3]).sum() == 4


def test_binding_checks_its_arguments_without_a_device():
    from aznet_hip import ffi
    assert "az_det_diag_eval" in ffi.SYMBOLS
    ctx = ffi.AzContext.__new__(ffi.AzContext)           # no az_create: the checks come before the library is touched
    case, group = R.hand_case()
    C, N, db, dc, doff, gb, gd, goff = case
    bad = [dict(det_off=doff[:-1]), dict(gt_off=goff[1:]), dict(det_box=db[:-1]), dict(det_conf=dc[:-1]),
           dict(gt_box=gb[:-1]), dict(gt_difficult=gd[:-1]), dict(class_group=group[:-1])]
    base = dict(n_classes=C, n_images=N, det_box=db, det_conf=dc, det_off=doff, gt_box=gb, gt_difficult=gd, gt_off=goff,
                class_group=group)
    bad += [dict(cuts=(0.5, np.inf)), dict(cuts=(np.nan,))]             # inf * (npos = 0) has no row count
    for b in bad:
        with pytest.raises(ffi.AzError) as e:
            ctx.det_diag_eval(**dict(base, **b))
        assert e.value.code == ffi.AZ_ERR_INVALID
    with pytest.raises(ValueError):                                      # the restatement refuses them too
        R.diag_flat(*case, cuts=(0.5, np.inf))


def test_header_declares_the_entry():
    header = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    m = re.search(r"\bint az_det_diag_eval\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 28
    for word in ("bg_overlap", "class_group", "loc_fixed_out", "gt_claim_out", "fp_at_out", "ap_fix_out", "kernel_ms_out"):
        assert word in m.group(1)
    mk = open(os.path.join(REPO, "az-net_amd", "csrc", "Makefile")).read()
    assert "az_ddiag.o" in mk and "az_eval_dev.h" in mk


def _tool(name):
    sys.path.insert(0, os.path.abspath(TOOLS))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_tool_parser():
    p = _tool("diagnose_det").build_parser()
    a = p.parse_args(["d.pkl"])
    assert (a.dets, a.imdb_name, a.no_nms, a.bg_overlap, a.output_dir, a.cfg_file) == ("d.pkl", "voc_2007_test", False, 0.1, None, None)
    a = p.parse_args(["d.pkl", "--imdb", "synthetic_375x500_4", "--cfg", "c.yml", "--no-nms", "--bg-overlap", "0.2", "--out", "o",
                      "--soft-nms", "gaussian", "--bbox-vote"])
    assert (a.imdb_name, a.cfg_file, a.no_nms, a.bg_overlap, a.output_dir) == ("synthetic_375x500_4", "c.yml", True, 0.2, "o")
    # the post-processing flags are eval_det.py's
    e = _tool("eval_det").build_parser().parse_args(["d.pkl", "--soft-nms", "gaussian", "--bbox-vote"])
    post = [k for k in vars(e) if k not in ("dets", "imdb_name", "output_dir", "no_nms", "comp_mode", "cfg_file", "gpu_id")]
    assert post and all(getattr(a, k) == getattr(e, k) for k in post)


class _StubImdb(object):
    name = "stub"

    def __init__(self, classes, roidb):
        self.classes = ["__background__"] + list(classes)
        self.num_classes = len(self.classes)
        self._roidb = roidb
        self.num_images = len(roidb)

    def gt_roidb(self):
        return self._roidb


class _StubCtx(object):
    """Answers det_diag_eval with the restatement, after planting what the caller asks for."""

    def __init__(self, plant=None):
        self.plant, self.calls = plant or {}, []

    def det_diag_eval(self, C, N, db, dc, doff, gb, gd, goff, **kw):
        self.calls.append(dict(kw, C=C, N=N, det_box=db, det_conf=dc, gt_box=gb))
        out = R.diag_flat(C, N, db, dc, doff, gb, gd, goff, **kw)
        out.update(self.plant)
        return out


def test_diagnose_builds_the_segments_and_the_host_tables():
    from detect import diagnose_det as DD
    # 3 classes x 2 images; 0-based boxes as a roidb holds them: areas 400 (small), 2500 (medium), 10000 (large)
    roidb = [{"boxes": np.array([[0, 0, 19, 19], [100, 0, 149, 49], [200, 0, 299, 99]], np.uint16),
              "gt_classes": np.array([1, 2, 3], np.int32)},
             {"boxes": np.array([[0, 0, 19, 19], [50, 50, 69, 69]], np.uint16), "gt_classes": np.array([1, 1], np.int32)}]
    imdb = _StubImdb(["a", "b", "c"], roidb)
    e = np.zeros((0, 5), np.float32)
    all_boxes = [[[], []],
                 [np.array([[0, 0, 19, 19, 0.9004], [100.04, 0, 149, 49, 0.8], [200, 0, 299, 99, 0.7]], np.float32), e],
                 [[], np.array([[0, 0, 19, 19, 0.6]], np.float32)],
                 [e, []]]
    ctx = _StubCtx()
    d = DD.diagnose(imdb, all_boxes, groups={"a": "x", "b": "x"}, ctx=ctx)
    call = ctx.calls[0]
    assert (call["C"], call["N"], call["metric_07"], call["min_overlap"], call["bg_overlap"]) == (3, 2, True, 0.5, 0.1)
    assert call["class_group"].tolist() == [0, 0, 1] and tuple(call["cuts"]) == DD.DEFAULT_CUTS
    # rounded as a results file holds them: '%.3f' scores, '%.1f' of x + 1
    assert call["det_conf"].tolist() == [0.9, 0.8, 0.7, 0.6] and call["det_box"][1].tolist() == [101.0, 1.0, 150.0, 50.0]
    assert call["gt_box"][0].tolist() == [1.0, 1.0, 20.0, 20.0]
    assert d["type"].tolist() == [R.TP, R.SIM, R.OTH, R.SIM]
    assert d["gt_by_size"].tolist() == [[3, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert d["miss_by_size"].tolist() == [[2, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert d["confusion"].tolist() == [[0, 1, 1], [1, 0, 0], [0, 0, 0]]
    # (class b's one detection is a SIM row: with it removed no row counts, and VOCevaldet's max over no finite precision is NaN)
    assert np.isnan(d["ap_fix"][1, 3]) and np.isnan(d["dap"][1, 2])
    assert np.array_equal(d["dap"], d["ap_fix"][:, 1:] - d["ap_fix"][:, :1], equal_nan=True) and d["mean_dap"].shape == (7,)
    # planted device answers: the host tables follow them, not the boxes
    plant = {"gt_claim": np.array([5, -1, 7, -1, 9], np.int32), "type": np.array([R.SIM, R.BG, R.OTH, R.TP], np.int8),
             "other_class": np.array([2, -1, 1, -1], np.int32),
             "ap_fix": np.array([[0.5, 0.5, 0.75, 0.5, 0.5, 0.5, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, np.nan, 1.0],
                                 [0.25] * 8])}
    d = DD.diagnose(imdb, all_boxes, area_edges=(401, 2500), ctx=_StubCtx(plant))
    # the boxes in class-major order: class a's (image 0, image 1 x 2), b's, c's -> claims 5, -1, 7 | -1 | 9
    assert d["gt_by_size"].tolist() == [[3, 0, 0], [0, 0, 1], [0, 0, 1]]
    assert d["miss_by_size"].tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 0]]
    assert d["confusion"].tolist() == [[0, 1, 1], [0, 0, 0], [0, 0, 0]]
    # the mean leaves a NaN entry out: variant 6 over classes a and c only
    assert d["mean_dap"].tolist() == [0.0, 0.25 / 3, 0.0, 0.0, 0.0, 0.5 / 2, 1.5 / 3]
    assert d["class_group"] is None
    lines = DD.summary_lines(d)
    text = "\n".join(lines)
    assert "n/a" in text and "Missed objects by size" in text and "a on c" in text
    with pytest.raises(ValueError):
        DD.diagnose(imdb, all_boxes, groups=[0, 1], ctx=_StubCtx())


def test_only_a_pascal_voc_imdb_takes_the_xml_records(tmp_path, monkeypatch):
    """A coco imdb carries _devkit_path, _year, _image_set and _data_path as pascal_voc does (datasets/coco.py): it must go
    through gt_roidb like any other imdb, and nothing may be written into its data tree."""
    from datasets import voc_eval
    from datasets.pascal_voc import pascal_voc
    from detect import diagnose_det as DD
    roidb = [{"boxes": np.array([[0, 0, 19, 19]], np.uint16), "gt_classes": np.array([1], np.int32)}]
    imdb = _StubImdb(["a", "b"], roidb)
    imdb._devkit_path, imdb._year, imdb._image_set = str(tmp_path / "COCO"), "2014", "val"
    imdb._data_path, imdb.image_index = str(tmp_path / "COCO" / "images"), [397133]
    used = []
    monkeypatch.setattr(voc_eval, "load_records", lambda db: used.append("xml") or [[]])
    real = voc_eval.roidb_records
    monkeypatch.setattr(voc_eval, "roidb_records", lambda db: used.append("roidb") or real(db))
    all_boxes = [[[]], [np.array([[0, 0, 19, 19, 0.9]], np.float32)], [[]]]
    d = DD.diagnose(imdb, all_boxes, ctx=_StubCtx())
    assert used == ["roidb"] and d["metric_07"] is True and d["type"].tolist() == [R.TP] and d["npos"].tolist() == [1, 0]
    assert list(tmp_path.iterdir()) == []
    # a pascal_voc imdb, and only that class, reads its XML records (2012: the area metric)
    voc = pascal_voc.__new__(pascal_voc)
    voc.__dict__.update(imdb.__dict__, _year="2012", _classes=imdb.classes, _image_index=[397133])
    del used[:]
    monkeypatch.setattr(voc_eval, "load_records", lambda db: used.append("xml") or [[("a", [1.0, 1.0, 20.0, 20.0], 1)]])
    d = DD.diagnose(voc, all_boxes, ctx=_StubCtx())
    assert used == ["xml"] and d["metric_07"] is False and d["type"].tolist() == [R.IGN] and d["npos"].tolist() == [0, 0]


def test_default_groups_are_hoiems_sets_for_the_voc_names_only():
    from detect import diagnose_det as DD
    assert np.array_equal(DD.default_groups(list(R.VOC_CLASSES)) == DD.default_groups(list(R.VOC_CLASSES))[:, None],
                          R.VOC_GROUPS == R.VOC_GROUPS[:, None])
    g = DD.default_groups(list(R.VOC_CLASSES))
    names = list(R.VOC_CLASSES)
    assert g[names.index("car")] == g[names.index("boat")] and g[names.index("cat")] == g[names.index("bird")]
    assert g[names.index("sofa")] == g[names.index("pottedplant")] and g[names.index("person")] != g[names.index("cat")]
    assert (g == g[names.index("tvmonitor")]).sum() == 1 and (g == g[names.index("bottle")]).sum() == 1
    assert DD.default_groups(["class%d" % k for k in range(1, 21)]) is None and DD.default_groups(names[:19]) is None


def test_summary_lines_on_empty_tables():
    from detect import diagnose_det as DD
    imdb = _StubImdb(["a", "b"], [{"boxes": np.zeros((0, 4), np.uint16), "gt_classes": np.zeros(0, np.int32)}])
    d = DD.diagnose(imdb, [[[]], [[]], [[]]], ctx=_StubCtx())
    assert d["type_table"].sum() == 0 and d["ap_fix"].tolist() == [[0.0] * 8] * 2
    with np.errstate(all="raise"):
        lines = DD.summary_lines(d)
    assert any("n/a" in l for l in lines) and any(l.startswith("Confusions") and l.endswith(": 0") for l in lines)
