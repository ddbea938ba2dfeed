"""CPU: Soft-NMS and box voting off the device -- the restatement (tests/postproc_ref.py) against the oracle's nms and on
hand-derived cases, the configuration keys and the tools' flags, the two entries in header / binding / library, the routing
of detect.test.postprocess_detections with the context stubbed, and the conditions on the generated gaussian cases that
tests/test_gpu_postproc.py compares with the float64 restatement in order."""
import ctypes
import os
import re

import numpy as np
import pytest

import postproc_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
f32 = np.float32


def oracle_nms(dets, thresh):
    """oracle.az_oracle.nms; with tied scores its argsort's order is NumPy's choice, so the visiting order the header states
    (a stable ascending sort reversed: the higher index first) is handed to the same C restatement."""
    import oracle.az_oracle as orc
    dets = np.ascontiguousarray(dets, np.float32)
    if np.unique(dets[:, 4]).size == dets.shape[0]:
        return orc.nms(dets, thresh)
    order = np.ascontiguousarray(np.argsort(dets[:, 4], kind="stable")[::-1], dtype=np.int64)
    keep = np.zeros(dets.shape[0], np.int64)
    n = orc.lib().orc_nms(orc._fp(dets), dets.shape[0], orc._lp(order), float(thresh), orc._lp(keep))
    return [int(k) for k in keep[:n]]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", [0.0, 0.3, 0.5, 1.0])
def test_hard_restatement_equals_the_oracle_nms(thresh):
    for n in (1, 2, 3, 17, 64, 100, 257, 600):
        for kind, d in (("random", P.random_group(n, n)), ("clustered", P.clustered_group(n + 1, n)),
                        ("duplicates", P.with_duplicates(P.clustered_group(n + 2, n), n)),
                        ("equal scores", P.equal_scores(P.clustered_group(n + 3, n)))):
            keep, sc = P.soft_nms_ref(d, "hard", thresh, min_score=P.hard_min_score(d))
            assert keep.tolist() == oracle_nms(d, thresh), (kind, n, thresh)
            assert sc.dtype == np.float32 and np.array_equal(sc, d[keep, 4])
    assert P.soft_nms_ref(np.zeros((0, 5), f32), "hard", thresh)[0].size == 0


A, B, C = [0, 0, 3, 3], [0, 0, 3, 1], [0, 2, 3, 3]            # areas 16, 8, 8; IoU(A, B) = IoU(A, C) = 8 / 16, IoU(B, C) = 0


def rows(boxes, scores):
    return np.hstack((np.array(boxes, f32), np.array(scores, f32)[:, None]))


def test_two_boxes_by_hand():
    d = rows([A, B], [0.8, 0.6])
    assert P.iou_row(d[:, :4], P._areas(d[:, :4], f32(1)), 0).tolist() == [1.0, 0.5]
    for dt in (np.float32, np.float64):
        keep, sc = P.soft_nms_ref(d, "linear", 0.3, min_score=0.001, dtype=dt)
        assert keep.tolist() == [0, 1] and sc.tolist() == [dt(f32(0.8)), dt(f32(0.6)) * dt(0.5)] and sc.dtype == dt
    # the comparison is >=: at thresh = IoU the score decays, just above it does not
    assert P.soft_nms_ref(d, "linear", 0.5)[1].tolist() == [f32(0.8), f32(0.6) * f32(0.5)]
    assert P.soft_nms_ref(d, "linear", 0.5000001)[1].tolist() == [f32(0.8), f32(0.6)]
    assert P.soft_nms_ref(d, "hard", 0.5)[0].tolist() == [0] and P.soft_nms_ref(d, "hard", 0.5000001)[0].tolist() == [0, 1]
    # hard with min_score 0: the suppressed box stays in the pool with score 0 and is emitted last
    keep, sc = P.soft_nms_ref(d, "hard", 0.5, min_score=0.0)
    assert keep.tolist() == [0, 1] and sc.tolist() == [f32(0.8), 0.0]
    # gaussian: w = exp(-0.25 / 0.5), whatever thresh is
    for t in (0.0, 0.9):
        keep, sc = P.soft_nms_ref(d, "gaussian", t, sigma=0.5, dtype=np.float64)
        assert keep.tolist() == [0, 1] and abs(sc[1] - float(f32(0.6)) * np.exp(-0.5)) < 1e-15
    sc32 = P.soft_nms_ref(d, "gaussian", 0.3, sigma=0.5)[1]
    assert sc32.dtype == np.float32 and abs(float(sc32[1]) / (float(f32(0.6)) * np.exp(-0.5)) - 1) < 3e-7
    # the order follows the CURRENT scores: B decays below a third box that does not touch A
    far = [100, 100, 103, 103]
    keep, sc = P.soft_nms_ref(rows([A, B, far], [0.8, 0.6, 0.5]), "linear", 0.3)
    assert keep.tolist() == [0, 2, 1] and sc.tolist() == [f32(0.8), f32(0.5), f32(0.6) * f32(0.5)]


def test_three_boxes_by_hand():
    d = rows([A, B, C], [1.0, 0.75, 0.5])
    keep, sc = P.soft_nms_ref(d, "linear", 0.3, min_score=0.001)
    assert keep.tolist() == [0, 1, 2] and sc.tolist() == [1.0, 0.375, 0.25]          # B and C do not overlap: C decays once
    # dropped when s < min_score, kept when s == min_score
    assert P.soft_nms_ref(d, "linear", 0.3, min_score=0.25)[0].tolist() == [0, 1, 2]
    assert P.soft_nms_ref(d, "linear", 0.3, min_score=0.2500001)[0].tolist() == [0, 1]
    assert P.soft_nms_ref(d, "linear", 0.3, min_score=0.5)[0].tolist() == [0]
    assert P.soft_nms_ref(d, "hard", 0.3)[0].tolist() == [0]
    # equal scores: the higher original index first
    keep, sc = P.soft_nms_ref(rows([A, B, C], [0.5, 0.5, 0.5]), "linear", 0.3)
    assert keep.tolist() == [2, 1, 0] and sc.tolist() == [0.5, 0.5, 0.125]            # A decays twice, by 1 - 0.5 each time
    # min_score above every score: the first pick is still emitted (a box is dropped only after a decay)
    assert P.soft_nms_ref(d, "linear", 0.3, min_score=2.0)[0].tolist() == [0]


def test_voting_by_hand():
    k, lo, hi, far = [10, 10, 20, 20], [9, 9, 19, 19], [11, 11, 21, 21], [100, 100, 110, 110]
    d = rows([k, lo, hi, far], [0.5, 0.25, 0.25, 1.0])
    assert P.iou_row(d[:, :4], P._areas(d[:, :4], f32(1)), 0)[1] == f32(100) / f32(142)
    for form in (True, False):
        v = P.box_vote_ref(d, [0, 3], 0.5, loop=form)
        assert v.dtype == np.float32 and v.tolist() == [k, far]              # symmetric voters: the box's own coordinates
    # IoU(lo, hi) = 81 / 161 is below 0.6: lo is voted on by k and itself, (0.5 * 10 + 0.25 * 9) / 0.75, rounded once to float32
    assert P.box_vote_ref(d, [1], 0.6).tolist() == [[float(f32(7.25 / 0.75))] * 2 + [float(f32(14.75 / 0.75))] * 2]
    assert P.box_vote_ref(d, [1], 0.5).tolist() == [k]                      # ... at 0.5 by all three: k's coordinates
    assert P.box_vote_ref(d, [0], 0.75).tolist() == [k]                     # above the neighbours' IoU: the self vote alone
    assert P.box_vote_ref(d, [0], 1.0).tolist() == [k] and P.box_vote_ref(d, [0], 1.5).tolist() == [k]    # (no voter: as it was)
    # weights are the rows' scores as given: a heavier upper neighbour pulls the box up
    d2 = rows([k, lo, hi], [0.5, 0.25, 0.75])
    assert P.box_vote_ref(d2, [0], 0.5).tolist() == [[float(f32((5 + 2.25 + 8.25) / 1.5))] * 2 + [float(f32((10 + 4.75 + 15.75) / 1.5))] * 2]
    # voters of score 0 carry no weight; sw == 0 leaves the box as it was
    assert P.box_vote_ref(rows([k, lo, hi], [0.5, 0.0, 0.0]), [0], 0.5).tolist() == [k]
    assert P.box_vote_ref(rows([k, lo, hi], [0.0, 0.0, 0.0]), [0, 1], 0.5).tolist() == [k, lo]
    assert P.box_vote_ref(np.zeros((0, 5), f32), [], 0.5).shape == (0, 4)


def test_voting_forms_agree_and_whole_number_cases_are_exact():
    for n in (1, 40, 257):
        d = P.clustered_group(7 + n, n)
        keep = P.soft_nms_ref(d, "linear", 0.3)[0]
        for vt in (0.0, 0.5, 0.8):
            assert np.array_equal(P.box_vote_ref(d, keep, vt, loop=True), P.box_vote_ref(d, keep, vt, loop=False)), (n, vt)
        w = P.whole_number_group(n, n)
        keep = P.soft_nms_ref(w, "hard", 0.5, min_score=P.hard_min_score(w))[0]
        for vt in (0.0, 0.5):
            assert np.array_equal(P.box_vote_ref(w, keep, vt), P.box_vote_exact(w, keep, vt)), (n, vt)


# ---- the conditions on the generated cases -------------------------------------------------------------------------------
def test_gaussian_cases_have_the_gap_and_order_alike_in_both_precisions():
    """What lets tests/test_gpu_postproc.py hold the device to the float64 restatement's indices: no pick and no drop of a
    gaussian case is decided by less than GAP (relative), and the float32 restatement picks the same boxes in the same order."""
    assert sorted(P.GAUSS_SEEDS) == sorted(P.GAUSS_SIZES) and 100 in P.GAUSS_SIZES and 257 in P.GAUSS_SIZES and P.GAP == 1e-4
    for n in P.GAUSS_SIZES:
        d = P.gaussian_case(n)
        info = {}
        k64, s64 = P.soft_nms_ref(d, "gaussian", dtype=np.float64, info=info, **P.GAUSS)
        k32, s32 = P.soft_nms_ref(d, "gaussian", dtype=np.float32, **P.GAUSS)
        print("  gaussian case, %3d boxes (seed %d): %3d picked, gap %.3e, margin to min_score %.3e, float32 vs float64 %.2e"
              % (n, P.GAUSS_SEEDS[n], k64.size, info["gap"], info["margin"], np.max(np.abs(s32 - s64) / s64)))
        assert info["gap"] >= P.GAP and info["margin"] >= P.GAP, n
        assert np.array_equal(k32, k64), n
        assert (k64.size < n or n == 2) and k64.size >= 2                      # the drop does bind, and boxes do survive
        assert P.gaussian_ok(d)[0] and P.gaussian_seed(n) == P.GAUSS_SEEDS[n]    # ... and the seed is the search's first


# ---- configuration, tools, ABI -------------------------------------------------------------------------------------------
KEYS = dict(NMS_METHOD="hard", SOFT_NMS_SIGMA=0.5, SOFT_NMS_MIN_SCORE=0.001, BBOX_VOTE=False, BBOX_VOTE_THRESH=0.8)


@pytest.fixture
def test_cfg(monkeypatch):
    from detect.config import cfg
    for k in KEYS:
        monkeypatch.setattr(cfg.TEST, k, cfg.TEST[k])                           # (put back afterwards)
    return cfg


def test_cfg_keys_defaults_and_yaml(tmp_path, test_cfg):
    from detect import config
    T = config.cfg.TEST
    for k, v in KEYS.items():
        assert T[k] == v and type(T[k]) is type(v), k
    assert config.nms_method() == "hard" and config.NMS_METHODS == ("hard", "linear", "gaussian")
    y = tmp_path / "pp.yml"
    y.write_text("TEST:\n  NMS_METHOD: gaussian\n  SOFT_NMS_SIGMA: 0.25\n  SOFT_NMS_MIN_SCORE: 0.01\n  BBOX_VOTE: True\n"
                 "  BBOX_VOTE_THRESH: 0.7\n")
    config.cfg_from_file(str(y))
    assert (T.NMS_METHOD, T.SOFT_NMS_SIGMA, T.SOFT_NMS_MIN_SCORE, T.BBOX_VOTE, T.BBOX_VOTE_THRESH) == ("gaussian", 0.25, 0.01, True, 0.7)
    assert config.nms_method() == "gaussian"
    for bad in ("soft", "Linear", "", 1):
        T.NMS_METHOD = bad
        with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
            config.nms_method()
    with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
        config.nms_method("none")
    y.write_text("TEST:\n  BBOX_VOTE: 1\n")
    with pytest.raises(ValueError):
        config.cfg_from_file(str(y))
    text = open(os.path.join(REPO, "az-net_amd", "lib", "detect", "config.py")).read()
    for k in ("NMS_METHOD='hard'", "SOFT_NMS_SIGMA=0.5", "SOFT_NMS_MIN_SCORE=0.001", "BBOX_VOTE=False", "BBOX_VOTE_THRESH=0.8"):
        assert re.search(re.escape(k) + r"[,)]\s+# \(not in the reference\)", text), k


def test_flags_of_the_three_tools(monkeypatch, test_cfg, tmp_path, capsys):
    """The two detection tools get the flags from tools/_cli.py (build_parser adds them to a tool that declares --comp, parse
    applies them), eval_det.py adds and applies them itself; a flag wins over a --cfg file read afterwards."""
    from detect import config
    monkeypatch.syspath_prepend(TOOLS)
    import _cli
    import eval_det
    import test_det_net
    import test_shared
    import train_det_net
    tables = [[_cli.COMMON, test_det_net.FLAGS], [_cli.COMMON, _cli.THRESH, test_shared.FLAGS]]
    parsers = [_cli.build_parser("t", t) for t in tables] + [eval_det.build_parser()]
    lead = [["--net", "synthetic", "--prop", "p.pkl"], ["--tz", "0.5"], ["d.pkl"]]
    try:
        for p, first in zip(parsers, lead):
            a = p.parse_args(first)
            assert a.soft_nms is None and a.bbox_vote is False
            _cli.set_postproc(a)
            assert test_cfg.TEST.NMS_METHOD == "hard" and test_cfg.TEST.BBOX_VOTE is False      # no flag: the cfg as it stands
            for m in ("linear", "gaussian"):
                a = p.parse_args(first + ["--soft-nms", m, "--bbox-vote"])
                assert a.soft_nms == m and a.bbox_vote is True
                _cli.set_postproc(a)
                assert test_cfg.TEST.NMS_METHOD == m and test_cfg.TEST.BBOX_VOTE is True
                config.cfg_clear_cli()
                test_cfg.TEST.NMS_METHOD, test_cfg.TEST.BBOX_VOTE = "hard", False
            for bad in (["--soft-nms", "hard"], ["--soft-nms"], ["--bbox-vote", "1"]):
                with pytest.raises(SystemExit):
                    p.parse_args(first + bad)
        # the tools that evaluate no detections do not take them
        with pytest.raises(SystemExit):
            _cli.build_parser("t", [train_det_net.COMMON, train_det_net.FLAGS]).parse_args(["--bbox-vote"])
        with pytest.raises(SystemExit):
            _cli.build_parser("t", [_cli.COMMON, _cli.THRESH]).parse_args(["--soft-nms", "linear"])
        # through parse, as the two tools call it; the --cfg file they read AFTERWARDS does not take the flag's value back
        y = tmp_path / "pp.yml"
        y.write_text("TEST:\n  NMS_METHOD: gaussian\n  BBOX_VOTE_THRESH: 0.7\n")
        monkeypatch.setattr("sys.argv", ["test_det_net.py", "--net", "synthetic", "--prop", "p.pkl", "--soft-nms", "linear", "--cfg", str(y)])
        a = _cli.parse("t", tables[0])
        assert a.soft_nms == "linear" and test_cfg.TEST.NMS_METHOD == "linear" and test_cfg.TEST.BBOX_VOTE is False
        config.cfg_from_file(a.cfg_file)
        assert test_cfg.TEST.NMS_METHOD == "linear" and test_cfg.TEST.BBOX_VOTE_THRESH == 0.7
        config.cfg_clear_cli()
        # no flag: the file's value stays
        monkeypatch.setattr("sys.argv", ["test_shared.py", "--tz", "0.5", "--cfg", str(y)])
        a = _cli.parse("t", tables[1])
        config.cfg_from_file(a.cfg_file)
        assert test_cfg.TEST.NMS_METHOD == "gaussian" and test_cfg.TEST.BBOX_VOTE is False
        with pytest.raises(KeyError):
            config.cfg_set_cli("TEST", "NO_SUCH_KEY", 1)
        with pytest.raises(KeyError):
            config.cfg_set_cli("TEST", "BBOX_VOTE", "yes")
    finally:
        config.cfg_clear_cli()
    src = open(os.path.join(TOOLS, "eval_det.py")).read()
    assert "postprocess_detections(all_boxes)" in src and "apply_nms" not in src


def test_header_binding_and_library_agree_on_the_entries():
    from aznet_hip import ffi
    header = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    L = ffi.load_library()
    for name, nargs in (("az_soft_nms_batched", 11), ("az_box_vote_batched", 8)):
        assert name in ffi.SYMBOLS
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == nargs
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    for const, val in (("AZ_NMS_HARD", ffi.AZ_NMS_HARD), ("AZ_NMS_LINEAR", ffi.AZ_NMS_LINEAR), ("AZ_NMS_GAUSSIAN", ffi.AZ_NMS_GAUSSIAN),
                       ("AZ_SOFT_NMS_MAX", ffi.AZ_SOFT_NMS_MAX)):
        assert int(re.search(r"#define\s+" + const + r"\s+(\d+)", header).group(1)) == val
    assert ffi.NMS_METHODS == {"hard": 0, "linear": 1, "gaussian": 2} and ffi.AZ_SOFT_NMS_MAX == 4096
    L.az_soft_nms_batched.argtypes[4:8] == [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    for word in ("the higher original index", "(double)ovr >= thresh", "expf(-(ovr * ovr) / (float)sigma)", "ascending j",
                 "AZ_ERR_CAPACITY", "uses `>`"):
        assert word in header, word
    makefile = open(os.path.join(REPO, "az-net_amd", "csrc", "Makefile")).read()
    assert "az_postproc.o" in makefile and "-ffp-contract=off" in makefile


def test_wrappers_check_dtype_and_shape_as_nms_does():
    from utils import cython_nms
    d = P.random_group(1, 4)
    for fn in (lambda x: cython_nms.soft_nms(x), lambda x: cython_nms.box_vote(x, [0])):
        with pytest.raises(ValueError, match="dtype mismatch"):
            fn(d.astype(np.float64))
        with pytest.raises(ValueError, match="wrong number of dimensions"):
            fn(d.ravel())
        with pytest.raises(ValueError, match="wrong number of dimensions"):
            fn(d.tolist())
    import inspect
    assert str(inspect.signature(cython_nms.soft_nms)) == "(dets, method='linear', thresh=0.3, sigma=0.5, min_score=0.001)"
    assert str(inspect.signature(cython_nms.box_vote)) == "(dets, keep, vote_thresh=0.8)"


# ---- the routing of postprocess_detections -----------------------------------------------------------------------------------
class StubContext(object):
    """The three context calls through the restatement, each call noted."""

    def __init__(self):
        self.calls = []

    def nms_batched(self, sets, thresh):
        self.calls.append(("nms_batched", len(sets), thresh))
        return [P.soft_nms_ref(d, "hard", thresh, min_score=P.hard_min_score(d))[0] for d in sets]

    def soft_nms_batched(self, sets, method, thresh, sigma, min_score):
        self.calls.append(("soft_nms_batched", len(sets), method, thresh, sigma, min_score))
        return [P.soft_nms_ref(d, method, thresh, sigma, min_score) for d in sets]

    def box_vote_batched(self, sets, keeps, vote_thresh):
        self.calls.append(("box_vote_batched", len(sets), vote_thresh))
        return [P.box_vote_ref(d, k, vote_thresh) for d, k in zip(sets, keeps)]


def same(a, b):
    return len(a) == len(b) and all(
        len(x) == len(y) and all((isinstance(u, list) and u == [] and isinstance(v, list) and v == []) or
                                 (not isinstance(u, list) and not isinstance(v, list) and u.dtype == v.dtype and np.array_equal(u, v))
                                 for u, v in zip(x, y)) for x, y in zip(a, b))


def test_defaults_route_to_apply_nms(monkeypatch, test_cfg):
    from aznet_hip import ffi
    from detect import test as T
    stub = StubContext()
    monkeypatch.setattr(ffi, "default_context", lambda device=None: stub)
    boxes = P.front_door_boxes()
    want = T.apply_nms(boxes, test_cfg.TEST.NMS)
    assert stub.calls == [("nms_batched", 8, 0.5)]
    got = T.postprocess_detections(boxes)
    assert stub.calls == [("nms_batched", 8, 0.5)] * 2 and same(got, want)       # the same one call, the same bits
    seen = []
    monkeypatch.setattr(T, "apply_nms", lambda ab, th: seen.append((ab is boxes, th)) or "handed on")
    assert T.postprocess_detections(boxes) == "handed on" and seen == [(True, 0.5)]
    src = open(os.path.join(REPO, "az-net_amd", "lib", "detect", "test.py")).read()
    assert "nms_dets = postprocess_detections(all_boxes)" in src and src.index("pickle.dump(all_boxes") < src.index("nms_dets = postprocess")


@pytest.mark.parametrize("method, vote", [("hard", True), ("linear", False), ("linear", True), ("gaussian", False), ("gaussian", True)])
def test_settings_route_to_one_batched_call_each(monkeypatch, test_cfg, method, vote):
    from aznet_hip import ffi
    from detect import test as T
    stub = StubContext()
    monkeypatch.setattr(ffi, "default_context", lambda device=None: stub)
    test_cfg.TEST.NMS_METHOD, test_cfg.TEST.BBOX_VOTE = method, vote
    test_cfg.TEST.SOFT_NMS_SIGMA, test_cfg.TEST.BBOX_VOTE_THRESH = 0.25, 0.7
    boxes = P.front_door_boxes()
    got = T.postprocess_detections(boxes)
    first = ("nms_batched", 8, 0.5) if method == "hard" else ("soft_nms_batched", 8, method, 0.5, 0.25, 0.001)
    assert stub.calls == [first] + ([("box_vote_batched", 8, 0.7)] if vote else [])
    assert same(got, P.postprocess_ref(boxes, method, 0.5, 0.25, 0.001, vote, 0.7))
    assert got[0] == [[], [], [], []] and sum(not isinstance(g, list) for cls in got for g in cls) == 6
    test_cfg.TEST.NMS_METHOD = "soft"
    with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
        T.postprocess_detections(boxes)
