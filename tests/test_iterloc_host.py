"""CPU: iterative box localisation off the device -- the restatement (tests/iterloc_ref.py) on bias-only heads against
hand-derived answers, its ordering, threshold, cap and early end, _Detections.add with and without the later rounds' rows,
the configuration keys, the tools' flags and the two entries in header / binding / library."""
import ctypes
import heapq
import os
import re

import numpy as np
import pytest

import det_infer_ref as D
import iterloc_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
f32 = np.float32
H, W, SCALE = R.IMAGE
ANCHORS = np.array([[100, 100, 164, 132], [200, 150, 264, 182]], np.float64)     # 64 x 32 at eps = 0


def by_head(head, eps=0.0, dedup=0.0, batch=10000, calls=None):
    def fn(boxes):
        if calls is not None:
            calls.append(len(boxes))
        return D.detect_ref(boxes, SCALE, dedup, batch, (H, W), eps, D.bias_rows(head))
    return fn


def table(scores, calls=None):
    """A detect_fn that answers a call of P rows with the table's rows (repeated past its end) and boxes that name their
    row and class."""
    scores = np.asarray(scores, f32)

    def fn(boxes):
        P, K = len(boxes), scores.shape[1]
        if calls is not None:
            calls.append(P)
        b = np.zeros((P, K, 4))
        b[:, :, 0] = np.arange(P)[:, None]
        b[:, :, 1] = np.arange(K)[None, :]
        b[:, :, 2:] = np.asarray(boxes)[:, None, :2] + 1000
        return scores[np.arange(P) % len(scores)], b.reshape(P, 4 * K)
    return fn


def probs(head):
    return D.bias_rows(head)(np.arange(1), None)[0][0]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_every_round_shifts_a_class_box_by_its_own_delta():
    head = R.shift_head(3)
    p = probs(head)
    s, b, ex = R.iter_ref(by_head(head), ANCHORS, 4, 0.0, 100)
    shift = lambda j, t: t * np.array([j, -j / 4.0, j, -j / 4.0])     # noqa: E731
    assert np.array_equal(s, np.tile(p, (2, 1)))
    assert np.array_equal(b, np.hstack([ANCHORS + shift(j, 1) for j in range(3)]))
    # class-major: (class 1, row 0), (class 1, row 1), (class 2, row 0), (class 2, row 1); class 0 is never a source
    assert ex["count"].tolist() == [4, 4, 4]
    assert ex["cls"].tolist() == [1, 1, 2, 2] * 3
    assert ex["src"].tolist() == [0, 1, 0, 1] + [0, 1, 2, 3] * 2      # the proposal row, then the position in the last list
    assert ex["round"].tolist() == [2] * 4 + [3] * 4 + [4] * 4
    for t in (2, 3, 4):
        want = np.array([ANCHORS[i] + shift(j, t) for j in (1, 2) for i in (0, 1)])
        assert np.array_equal(ex["box"][4 * (t - 2):4 * (t - 1)], want), t
    assert np.array_equal(ex["score"], np.tile(p[[1, 1, 2, 2]], 3)) and ex["score"].dtype == f32
    assert ex["box"].dtype == np.float64 and ex["cls"].dtype == np.int32 and ex["src"].dtype == np.int32


def test_only_the_source_class_column_is_taken():
    # class 2's refined box is shifted by class 2's delta again, never by class 1's: the boxes of the two classes part
    head = R.shift_head(3)
    _, _, ex = R.iter_ref(by_head(head), ANCHORS[:1], 2, 0.0, 10)
    assert ex["box"].tolist() == [[102, 99.5, 166, 131.5], [104, 99, 168, 131]]


def test_threshold_is_a_float32_comparison_with_equality_kept():
    head = R.shift_head(3, bc=[0.0, 1.0, 0.5])
    p = probs(head)
    assert p[1] > p[2] and p.dtype == f32
    run = lambda ms: R.iter_ref(by_head(head), ANCHORS, 2, ms, 100)[2]      # noqa: E731
    assert run(float(p[1]))["cls"].tolist() == [1, 1]                        # equal: kept
    assert run(float(np.nextafter(p[1], f32(2))))["count"].tolist() == [0]   # the score one float32 below: dropped
    assert run(float(p[2]))["cls"].tolist() == [1, 1, 2, 2]
    assert run(float(np.nextafter(p[2], f32(2))))["cls"].tolist() == [1, 1]
    # a double between p[1] and the next float32 that rounds to p[1]: the comparison is made in float32
    up = float(np.nextafter(p[1], f32(2)))
    ms = float(p[1]) + (up - float(p[1])) * 0.25
    assert ms > float(p[1]) and f32(ms) == p[1]
    assert run(ms)["cls"].tolist() == [1, 1]


def test_cap_keeps_the_lowest_f_among_equal_scores_in_ascending_f():
    sc = np.full((3, 3), 0.5, f32)
    _, _, ex = R.iter_ref(table(sc), np.zeros((3, 4)), 2, 0.0, 4)
    assert ex["count"].tolist() == [4]
    assert list(zip(ex["cls"].tolist(), ex["src"].tolist())) == [(1, 0), (1, 1), (1, 2), (2, 0)]
    # one higher score at the very end: it is kept, with the lowest f of the rest -- and still in ascending f
    sc[2, 2] = 0.75
    _, _, ex = R.iter_ref(table(sc), np.zeros((3, 4)), 2, 0.0, 4)
    assert list(zip(ex["cls"].tolist(), ex["src"].tolist())) == [(1, 0), (1, 1), (1, 2), (2, 2)]
    # the cut between two distinct scores, the lower ones first in f
    sc = np.array([[9, 0.1, 0.2], [9, 0.3, 0.4], [9, 0.5, 0.6]], f32)
    _, _, ex = R.iter_ref(table(sc), np.zeros((3, 4)), 2, 0.0, 3)
    assert list(zip(ex["cls"].tolist(), ex["src"].tolist())) == [(1, 2), (2, 1), (2, 2)]
    assert R.select([0.5, 0.5, 0.7, 0.5], 0.5, 2).tolist() == [0, 2]
    assert R.select([0.5, 0.5, 0.7, 0.5], 0.5, 4).tolist() == [0, 1, 2, 3]
    assert R.select([0.4, np.nan, 0.7], 0.5, 4).tolist() == [2]


def test_later_rounds_select_among_the_previous_rounds_extras_alone():
    # a call of n rows answers with rows 0 .. n-1 of the table: round 2 has 3 sources, whose own-class scores are
    # (row 0, class 1) = 0.9, (row 1, class 2) = 0.1, (row 2, class 2) = 0.8 -> round 3 takes positions 0 and 2
    sc = np.array([[0, 0.9, 0.2], [0, 0.3, 0.1], [0, 0.2, 0.8]], f32)
    calls = []
    _, _, ex = R.iter_ref(table(sc, calls), np.zeros((3, 4)), 3, 0.5, 100)
    assert ex["count"].tolist() == [2, 1] and calls == [3, 2, 1]
    assert ex["cls"].tolist() == [1, 2, 1] and ex["src"].tolist() == [0, 2, 0]
    assert ex["score"].tolist() == [f32(0.9), f32(0.1), f32(0.9)]


def test_early_end_and_one_round():
    head = R.shift_head(3)
    calls = []
    s, b, ex = R.iter_ref(by_head(head, calls=calls), ANCHORS, 5, 0.99, 100)
    assert calls == [2] and ex["count"].tolist() == [0, 0, 0, 0] and ex["cls"].size == 0 and ex["box"].shape == (0, 4)
    calls = []
    s1, b1, ex1 = R.iter_ref(by_head(head, calls=calls), ANCHORS, 1, 0.0, 100)
    assert calls == [2] and ex1["count"].size == 0 and ex1["score"].size == 0
    assert np.array_equal(s, s1) and np.array_equal(b, b1)


def test_the_dedup_inside_a_round_merges_and_restores_rows():
    # class 1 and 2 of one anchor land in one 1/16 cell: the merged row is decoded from the first one's box (test.py:215-218)
    head = R.shift_head(3)
    anchor = np.array([[101, 100, 165, 132]], np.float64)
    _, _, a = R.iter_ref(by_head(head, dedup=1. / 16.), anchor, 2, 0.0, 10)
    _, _, b = R.iter_ref(by_head(head, dedup=0.0), anchor, 2, 0.0, 10)
    assert a["count"].tolist() == [2] and np.array_equal(a["box"][0], b["box"][0])
    assert b["box"][1].tolist() == [105, 99, 169, 131]
    assert a["box"][1].tolist() == [104, 99.25, 168, 131.25]       # class 1's box (102, 99.75, ...) moved by class 2's delta


# ---- _Detections.add ---------------------------------------------------------------------------------------------------------
def old_add(self, i, scores, boxes):
    """_Detections.add as it was before the `extra` argument."""
    for j in range(1, self.num_classes):
        inds = np.where((scores[:, j] > self.thresh[j]))[0]
        cls_scores = scores[inds, j]
        cls_boxes = boxes[inds, j * 4:(j + 1) * 4]
        top_inds = np.argsort(-cls_scores)[:self.max_per_image]
        cls_scores = cls_scores[top_inds]
        cls_boxes = cls_boxes[top_inds, :]
        top = self.top_scores[j]
        for val in cls_scores:
            heapq.heappush(top, val)
        if len(top) > self.max_per_set:
            while len(top) > self.max_per_set:
                heapq.heappop(top)
            self.thresh[j] = top[0]
        self.all_boxes[j][i] = np.hstack((cls_boxes, cls_scores[:, np.newaxis])).astype(np.float32, copy=False)


def test_detections_add_with_and_without_extra():
    from detect.test import _Detections
    rng = np.random.RandomState(0)
    K, n = 4, 3
    a, b, c = _Detections(K, n), _Detections(K, n), _Detections(K, n)
    for i in range(n):
        s = rng.rand(150, K)
        bx = rng.rand(150, 4 * K) * 100
        a.add(i, s, bx)
        b.add(i, s, bx, None)
        old_add(c, i, s, bx)
    for j in range(1, K):
        for i in range(n):
            assert a.all_boxes[j][i].tobytes() == c.all_boxes[j][i].tobytes() == b.all_boxes[j][i].tobytes()
            assert a.all_boxes[j][i].dtype == np.float32
        assert a.thresh[j] == c.thresh[j] and a.top_scores[j] == c.top_scores[j]
    # with extra: class j's candidates are the base rows followed by its extra rows; threshold, top 100, heap on all of them
    d = _Detections(3, 1)
    s = np.array([[0.1, 0.5, 0.2], [0.1, 0.4, 0.3]])
    bx = np.arange(24, dtype=np.float64).reshape(2, 12)
    extra = dict(cls=np.array([2, 1, 2], np.int32), src=np.array([0, 1, 0], np.int32), round=np.array([2, 2, 3], np.int32),
                 score=np.array([0.9, 0.45, 0.25], f32), box=np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.float64))
    d.add(0, s, bx, extra)
    assert d.all_boxes[1][0].tolist() == [[4, 5, 6, 7, f32(0.5)], [5, 6, 7, 8, f32(0.45)], [16, 17, 18, 19, f32(0.4)]]
    assert d.all_boxes[2][0].tolist() == [[1, 2, 3, 4, f32(0.9)], [20, 21, 22, 23, f32(0.3)], [9, 10, 11, 12, f32(0.25)],
                                          [8, 9, 10, 11, f32(0.2)]]
    assert sorted(d.top_scores[2]) == [0.2, float(f32(0.25)), 0.3, float(f32(0.9))]
    # an empty extra is the base rows alone
    e, g = _Detections(3, 1), _Detections(3, 1)
    none = dict(cls=np.zeros(0, np.int32), score=np.zeros(0, f32), box=np.zeros((0, 4)))
    e.add(0, s, bx, none)
    g.add(0, s, bx)
    assert all(e.all_boxes[j][0].tobytes() == g.all_boxes[j][0].tobytes() for j in (1, 2))
    # the top 100 per image count the extras
    h = _Detections(2, 1)
    many = dict(cls=np.ones(150, np.int32), score=np.linspace(0.5, 0.9, 150).astype(f32), box=np.zeros((150, 4)))
    h.add(0, np.full((10, 2), 0.95), np.ones((10, 8)), many)
    got = h.all_boxes[1][0]
    assert got.shape == (100, 5) and np.all(got[:10, 4] == f32(0.95)) and np.all(got[10:, :4] == 0)


# ---- configuration, tools, ABI -------------------------------------------------------------------------------------------
KEYS = dict(ITER_LOC=1, ITER_LOC_SCORE=0.05, ITER_LOC_MAX=1000)


@pytest.fixture
def test_cfg(monkeypatch):
    from detect.config import cfg
    for k in list(KEYS) + ["SCALES"]:
        monkeypatch.setattr(cfg.TEST, k, cfg.TEST[k])
    return cfg


def test_cfg_keys_defaults_checks_and_yaml(tmp_path, test_cfg):
    from detect import config
    T = config.cfg.TEST
    for k, v in KEYS.items():
        assert T[k] == v and type(T[k]) is type(v), k
    assert config.iter_loc() == (1, 0.05, 1000)
    y = tmp_path / "il.yml"
    y.write_text("TEST:\n  ITER_LOC: 3\n  ITER_LOC_SCORE: 0.2\n  ITER_LOC_MAX: 64\n")
    config.cfg_from_file(str(y))
    assert config.iter_loc() == (3, 0.2, 64)
    assert config.iter_loc(8, 0, 4096) == (8, 0.0, 4096)
    for bad in (0, 9, -1, 2.0, "2", True):
        with pytest.raises(ValueError, match="ITER_LOC = "):
            config.iter_loc(rounds=bad)
    for bad in (float("nan"), float("inf"), "0.1", True):
        with pytest.raises(ValueError, match="ITER_LOC_SCORE"):
            config.iter_loc(score=bad)
    for bad in (0, 4097, 10.0, "7"):
        with pytest.raises(ValueError, match="ITER_LOC_MAX"):
            config.iter_loc(max_rows=bad)
    T.ITER_LOC = 9
    with pytest.raises(ValueError):
        config.iter_loc()
    y.write_text("TEST:\n  ITER_LOC: 2.5\n")
    with pytest.raises(ValueError):
        config.cfg_from_file(str(y))
    text = open(os.path.join(REPO, "az-net_amd", "lib", "detect", "config.py")).read()
    for k in ("ITER_LOC=1", "ITER_LOC_SCORE=0.05", "ITER_LOC_MAX=1000"):
        assert re.search(re.escape(k) + r"[,)]\s+# \(not in the reference\)", text), k


def test_several_scales_with_iter_loc_is_refused_by_name(test_cfg):
    from detect import test as dt
    test_cfg.TEST.ITER_LOC = 1
    test_cfg.TEST.SCALES = (480, 600)
    assert dt._iter_loc_rounds() is None                      # one pass: pyramids as ever
    test_cfg.TEST.ITER_LOC = 2
    with pytest.raises(ValueError, match=r"ITER_LOC.*SCALES"):
        dt._iter_loc_rounds()
    for fn in (lambda: dt.test_net({"full": None}, "no-such-file.pkl", None), lambda: dt.test_net_shared(None, None, None)):
        with pytest.raises(ValueError, match=r"ITER_LOC.*SCALES"):      # before a file is read or a net is touched
            fn()
    test_cfg.TEST.SCALES = (600,)
    assert dt._iter_loc_rounds() == (2, 0.05, 1000)
    test_cfg.TEST.ITER_LOC_MAX = 0
    with pytest.raises(ValueError, match="ITER_LOC_MAX"):
        dt._iter_loc_rounds()


def test_flags_of_the_two_detection_tools(monkeypatch, test_cfg, tmp_path):
    from detect import config
    monkeypatch.syspath_prepend(TOOLS)
    import _cli
    import eval_det
    import test_det_net
    import test_shared
    import train_det_net
    tables = [[_cli.COMMON, test_det_net.FLAGS], [_cli.COMMON, _cli.THRESH, test_shared.FLAGS]]
    lead = [["--net", "synthetic", "--prop", "p.pkl"], ["--tz", "0.5"]]
    try:
        for t, first in zip(tables, lead):
            p = _cli.build_parser("t", t)
            a = p.parse_args(first)
            assert a.iter_loc is None and a.iter_loc_score is None and a.iter_loc_max is None
            _cli.set_iter_loc(a)
            assert config.iter_loc() == (1, 0.05, 1000)                  # no flag: the cfg as it stands
            a = p.parse_args(first + ["--iter-loc", "3", "--iter-loc-score", "0.25", "--iter-loc-max", "77", "--bbox-vote"])
            assert (a.iter_loc, a.iter_loc_score, a.iter_loc_max, a.bbox_vote) == (3, 0.25, 77, True)
            _cli.set_iter_loc(a)
            assert config.iter_loc() == (3, 0.25, 77)
            config.cfg_clear_cli()
            for k, v in KEYS.items():
                test_cfg.TEST[k] = v
            a = p.parse_args(first + ["--iter-loc", "2"])                # one flag leaves the other keys alone
            _cli.set_iter_loc(a)
            assert config.iter_loc() == (2, 0.05, 1000)
            config.cfg_clear_cli()
            test_cfg.TEST.ITER_LOC = 1
            for bad in (["--iter-loc", "9"], ["--iter-loc", "0"], ["--iter-loc-max", "5000"], ["--iter-loc-score", "nan"]):
                with pytest.raises(ValueError):
                    _cli.set_iter_loc(p.parse_args(first + bad))
                assert config.iter_loc() == (1, 0.05, 1000)
            for bad in (["--iter-loc"], ["--iter-loc", "two"], ["--iter-loc-max", "1.5"]):
                with pytest.raises(SystemExit):
                    p.parse_args(first + bad)
        # eval_det.py re-scores saved detections and has no net; the trainers evaluate nothing
        with pytest.raises(SystemExit):
            eval_det.build_parser().parse_args(["d.pkl", "--iter-loc", "2"])
        with pytest.raises(SystemExit):
            _cli.build_parser("t", [train_det_net.COMMON, train_det_net.FLAGS]).parse_args(["--iter-loc", "2"])
        # through parse, as the tools call it: a --cfg file read afterwards does not take the flag's value back
        y = tmp_path / "il.yml"
        y.write_text("TEST:\n  ITER_LOC: 4\n  ITER_LOC_MAX: 50\n")
        monkeypatch.setattr("sys.argv", ["test_det_net.py", "--net", "synthetic", "--prop", "p.pkl", "--iter-loc", "2", "--cfg", str(y)])
        a = _cli.parse("t", tables[0])
        config.cfg_from_file(a.cfg_file)
        assert config.iter_loc() == (2, 0.05, 50)
    finally:
        config.cfg_clear_cli()


def test_header_binding_and_library_agree_on_the_entries():
    from aznet_hip import ffi
    header = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    L = ffi.load_library()
    for name in ("az_detect_iter", "az_detect_iter_skip"):
        assert name in ffi.SYMBOLS
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == 19
        fn = getattr(L, name)
        assert len(fn.argtypes) == 19 and fn.restype is ctypes.c_int
        assert fn.argtypes[9:12] == [ctypes.c_int, ctypes.c_double, ctypes.c_int]
    assert int(re.search(r"#define\s+AZ_ITER_LOC_MAX_ROUNDS\s+(\d+)", header).group(1)) == ffi.AZ_ITER_LOC_MAX_ROUNDS == R.MAX_ROUNDS
    assert ffi.AZ_ITER_LOC_MAX_ROWS == R.MAX_ROWS == 4096
    from detect import config
    assert (config.ITER_LOC_MAX_ROUNDS, config.ITER_LOC_MAX_ROWS) == (R.MAX_ROUNDS, R.MAX_ROWS)
    makefile = open(os.path.join(REPO, "az-net_amd", "csrc", "Makefile")).read()
    assert "az_iterloc.o" in makefile
    from aznet_hip.net import HipDetNet, HipFrcnnNet
    assert callable(HipDetNet.detect_iter) and callable(HipFrcnnNet.detect_iter) and callable(ffi.AzContext.detect_iter)
