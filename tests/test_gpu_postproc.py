"""GPU: Soft-NMS and box voting (csrc/az_postproc.hip: az_soft_nms_batched, az_box_vote_batched; AzContext.soft_nms_batched /
box_vote_batched; detect.test.postprocess_detections; tools/eval_det.py) against the NumPy restatement tests/postproc_ref.py.

Methods hard and linear: indices, count and scores bit for bit against the float32 restatement (the library is built without
contraction, so NumPy float32 restates every operation).  Method gaussian: expf is not np.exp, so indices and count against
the float64 restatement on the seed-searched cases whose gaps tests/test_postproc_host.py asserts, and scores within the
suite's 8x rule -- max|got - ref64| / max|ref64| against 8 x the same quantity of the float32 restatement, floor 1e-6
(train_step_ref.bound).  Box voting: bit for bit (one thread sums a box's voters in index order in float64).  Every figure
is printed before it is asserted (run with -s)."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import postproc_ref as P
from train_step_ref import bound, rel_err

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1024, 4096]
GRID_SIZES = [1, 2, 65, 256, 257]                 # every (thresh, min_score) pair; 1024 and 4096 take two pairs (below)
THRESH = [0.0, 0.3, 1.0]
MIN_SCORE = [0.0, 0.001, 2.0]                      # 2.0: above every score
_groups, _refs = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    return ffi.AzContext(0)


def group(n):
    """The clustered group of n boxes every test shares."""
    if n not in _groups:
        _groups[n] = P.clustered_group(900 + n, n) if n else np.zeros((0, 5), np.float32)
        _groups[n].setflags(write=False)
    return _groups[n]


def ref(key, d, method, thresh, min_score):
    """soft_nms_ref in float32, computed once per (case, setting)."""
    k = (key, method, thresh, min_score)
    if k not in _refs:
        _refs[k] = P.soft_nms_ref(d, method, thresh, 0.5, min_score)
    return _refs[k]


def check_exact(got, want, what):
    (gk, gs), (wk, ws) = got, want
    assert gk.dtype == np.int64 and gs.dtype == np.float32
    assert gk.size == wk.size, "%s: %d picked, the restatement picks %d" % (what, gk.size, wk.size)
    assert np.array_equal(gk, wk), "%s: indices differ from pick %d on" % (what, int(np.flatnonzero(gk != wk)[0]))
    assert np.array_equal(gs, ws), "%s: scores differ (max |d| %.3e)" % (what, float(np.max(np.abs(gs - ws))))


# ---- Soft-NMS, hard and linear: bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["hard", "linear"])
def test_every_group_size_in_one_call(ctx, method):
    sets = [group(n) for n in SIZES]
    got = ctx.soft_nms_batched(sets, method, 0.3, 0.5, 0.001)
    assert len(got) == len(SIZES)
    for n, g in zip(SIZES, got):
        check_exact(g, ref(n, group(n), method, 0.3, 0.001), "%s, %d boxes" % (method, n))
    print("  %s: picked %s of %s" % (method, [g[0].size for g in got], SIZES))


@pytest.mark.parametrize("method", ["hard", "linear"])
def test_thresholds_and_min_scores(ctx, method):
    for thresh in THRESH:
        for ms in MIN_SCORE:
            sizes = GRID_SIZES + ([1024, 4096] if (thresh, ms) == (1.0, 0.0) else [])      # (min_score 0: every box is emitted)
            got = ctx.soft_nms_batched([group(n) for n in sizes], method, thresh, 0.5, ms)
            for n, g in zip(sizes, got):
                check_exact(g, ref(n, group(n), method, thresh, ms), "%s, %d boxes, thresh %g, min_score %g" % (method, n, thresh, ms))
                if ms == 0.0:
                    assert sorted(g[0].tolist()) == list(range(n))
                if ms == 2.0:
                    assert g[0].size == 1                     # the first pick is emitted, everything else drops after its decay


@pytest.mark.parametrize("method", ["hard", "linear"])
def test_identical_boxes_equal_scores_and_zero_scores(ctx, method):
    cases = {}
    for n in (70, 300):
        d = group(257)[:1].repeat(n, 0).copy()
        d[:, 4] = np.linspace(0.05, 0.95, n, dtype=np.float32)
        cases["identical boxes %d" % n] = d
    for n in (65, 257, 600):
        cases["equal scores %d" % n] = P.equal_scores(P.clustered_group(n, n))
        cases["duplicates %d" % n] = P.with_duplicates(P.clustered_group(n + 1, n), n)
    for n in (10, 300):
        cases["zero scores %d" % n] = P.equal_scores(P.clustered_group(n + 2, n), 0.0)
        half = P.clustered_group(n + 3, n)
        half[::2, 4] = 0.0
        cases["some zero scores %d" % n] = half
    names = sorted(cases)
    for ms in (0.0, 0.001):
        got = ctx.soft_nms_batched([cases[k] for k in names], method, 0.3, 0.5, ms)
        for k, g in zip(names, got):
            check_exact(g, ref(k, cases[k], method, 0.3, ms), "%s, %s, min_score %g" % (method, k, ms))
    # the tie rule, seen directly: equal scores and boxes that do not touch come out by descending index
    n = 300
    apart = np.zeros((n, 5), np.float32)
    apart[:, 0] = apart[:, 1] = 50.0 * np.arange(n)
    apart[:, 2] = apart[:, 3] = 50.0 * np.arange(n) + 20
    apart[:, 4] = 0.5
    for d in (apart[:64], apart[:257], apart):
        keep, sc = ctx.soft_nms_batched([d], method, 0.3, 0.5, 0.001)[0]
        assert keep.tolist() == list(range(d.shape[0]))[::-1] and np.all(sc == np.float32(0.5))


def test_two_thousand_mixed_groups_in_one_call(ctx):
    """About 2000 groups of at most 100 boxes, empty ones among them: 200 distinct groups, each at ten places of the call (so
    the restatement runs 200 times and every one of the 2000 results is compared in full)."""
    rng = np.random.Generator(np.random.PCG64(11))
    sizes = rng.integers(0, 101, 200)
    sizes[:8] = [0, 0, 1, 2, 63, 64, 65, 100]
    distinct = [P.clustered_group(3000 + i, int(n), clusters=max(1, int(n) // 10)) for i, n in enumerate(sizes)]
    place = rng.permutation(np.repeat(np.arange(200), 10))
    sets = [distinct[i] for i in place]
    assert len(sets) == 2000 and sum(d.shape[0] == 0 for d in sets) >= 20
    for method in ("linear", "hard"):
        got = ctx.soft_nms_batched(sets, method, 0.3, 0.5, 0.001)
        want = [P.soft_nms_ref(d, method, 0.3, 0.5, 0.001) for d in distinct]
        for g, i in zip(got, place):
            check_exact(g, want[i], "%s, group of %d boxes" % (method, sizes[i]))
    keeps = [g[0] for g in got]
    votes = ctx.box_vote_batched(sets, keeps, 0.8)
    want_v = [P.box_vote_ref(d, w[0], 0.8) for d, w in zip(distinct, want)]
    for v, i in zip(votes, place):
        assert v.dtype == np.float32 and np.array_equal(v, want_v[i]), "voting, group of %d boxes" % sizes[i]


def test_repeated_calls_and_stale_scratch(ctx):
    """The same call twice gives the same bits; a small call after a large one (scratch full of the large one's keep lists,
    scores and counts) and the large one again are what they are alone."""
    from aznet_hip import ffi
    big = [group(n) for n in (4096, 1024, 257, 256)]
    small = [group(2), group(0), group(65)]
    fresh = ffi.AzContext(0)
    alone = fresh.soft_nms_batched(small, "linear", 0.3, 0.5, 0.001)
    a = ctx.soft_nms_batched(big, "linear", 0.3, 0.5, 0.001)
    b = ctx.soft_nms_batched(small, "linear", 0.3, 0.5, 0.001)
    c = ctx.soft_nms_batched(big, "linear", 0.3, 0.5, 0.001)
    for x, y in zip(a, c):
        check_exact(x, y, "second call")
    for x, y, n in zip(b, alone, (2, 0, 65)):
        check_exact(x, y, "after a large call")
        check_exact(x, ref(n, group(n), "linear", 0.3, 0.001), "after a large call, %d boxes" % n)
    va = ctx.box_vote_batched(big, [x[0] for x in a], 0.5)
    vb = ctx.box_vote_batched(small, [x[0] for x in b], 0.5)
    vc = ctx.box_vote_batched(big, [x[0] for x in a], 0.5)
    assert all(np.array_equal(x, y) for x, y in zip(va, vc))
    assert all(np.array_equal(x, y) for x, y in zip(vb, fresh.box_vote_batched(small, [x[0] for x in alone], 0.5)))
    fresh.close()


@pytest.mark.parametrize("thresh", [0.0, 0.3, 0.5, 1.0])
def test_hard_equals_az_nms_batched(ctx, thresh):
    sets = [group(n) for n in SIZES if n <= 1024] + [P.random_group(5, 300), P.with_duplicates(P.clustered_group(6, 200), 6)]
    ms = min(P.hard_min_score(d) for d in sets if d.shape[0])
    soft = ctx.soft_nms_batched(sets, "hard", thresh, 0.5, ms)
    hard = ctx.nms_batched(sets, thresh)
    for d, s, h in zip(sets, soft, hard):
        assert np.array_equal(s[0], h), (d.shape[0], thresh)
        assert np.array_equal(s[1], d[h, 4])


# ---- refusals: the code, and nothing written --------------------------------------------------------------------------------
def raw_soft(ctx, d, off, method, thresh, sigma, ms):
    from aznet_hip import ffi
    d = np.ascontiguousarray(d, np.float32)
    off = np.asarray(off, np.int32)
    total = max(int(np.max(off)), 1)
    keep, sc, nk = np.full(total, -7, np.int64), np.full(total, -7.0, np.float32), np.full(max(off.size - 1, 1), -7, np.int32)
    rc = ctx.L.az_soft_nms_batched(ctx.h, ffi._p(d, ctypes.c_float), ffi._p(off, ctypes.c_int32), off.size - 1, method, thresh, sigma, ms,
                                   ffi._p(keep, ctypes.c_int64), ffi._p(sc, ctypes.c_float), ffi._p(nk, ctypes.c_int32))
    return rc, bool(np.all(keep == -7) and np.all(sc == -7.0) and np.all(nk == -7))


def raw_vote(ctx, d, off, keep, nk, vt):
    from aznet_hip import ffi
    d = np.ascontiguousarray(d, np.float32)
    off, keep, nk = np.asarray(off, np.int32), np.asarray(keep, np.int64), np.asarray(nk, np.int32)
    out = np.full((max(int(np.max(off)), 1), 4), -7.0, np.float32)
    rc = ctx.L.az_box_vote_batched(ctx.h, ffi._p(d, ctypes.c_float), ffi._p(off, ctypes.c_int32), off.size - 1, ffi._p(keep, ctypes.c_int64),
                                   ffi._p(nk, ctypes.c_int32), vt, ffi._p(out, ctypes.c_float))
    return rc, bool(np.all(out == -7.0))


def test_refusals_leave_the_outputs_untouched(ctx):
    from aznet_hip import ffi
    d = P.clustered_group(1, 4200)
    two = [0, 10, 30]
    assert raw_soft(ctx, d, [0, 4097], ffi.AZ_NMS_LINEAR, 0.3, 0.5, 0.001) == (ffi.AZ_ERR_CAPACITY, True)
    assert raw_soft(ctx, d, [0, 5, 5, 4200], ffi.AZ_NMS_HARD, 0.3, 0.5, 0.001) == (ffi.AZ_ERR_CAPACITY, True)
    assert b"4096" in ctx.L.az_last_error(ctx.h)
    for method in (3, -1, 7):
        assert raw_soft(ctx, d, two, method, 0.3, 0.5, 0.001) == (ffi.AZ_ERR_INVALID, True)
    for sigma in (0.0, -0.5, float("nan"), float("inf"), 1e-60):
        assert raw_soft(ctx, d, two, ffi.AZ_NMS_GAUSSIAN, 0.3, sigma, 0.001) == (ffi.AZ_ERR_INVALID, True)
        assert raw_soft(ctx, d, two, ffi.AZ_NMS_LINEAR, 0.3, sigma, 0.001) == (ffi.AZ_OK, False)       # sigma is the gaussian's alone
    for ms in (-0.001, -1.0, float("nan")):
        assert raw_soft(ctx, d, two, ffi.AZ_NMS_LINEAR, 0.3, 0.5, ms) == (ffi.AZ_ERR_INVALID, True)
    for off in ([0, 20, 10], [0, 10, 5, 30], [1, 10, 30]):
        assert raw_soft(ctx, d, off, ffi.AZ_NMS_LINEAR, 0.3, 0.5, 0.001) == (ffi.AZ_ERR_INVALID, True)
    assert raw_soft(ctx, d, [0, 4096], ffi.AZ_NMS_LINEAR, 0.3, 0.5, 0.001) == (ffi.AZ_OK, False)
    # voting: a keep index outside its group, a count outside it, bad offsets, too large a group
    keep = np.zeros(4200, np.int64)
    keep[10:13] = [0, 19, 5]
    assert raw_vote(ctx, d, two, keep, [1, 3], 0.5) == (ffi.AZ_OK, False)
    for bad in (20, -1, 1 << 40):
        k = keep.copy()
        k[11] = bad
        assert raw_vote(ctx, d, two, k, [1, 3], 0.5) == (ffi.AZ_ERR_INVALID, True)
    for nk in ([11, 0], [0, -1], [0, 21]):
        assert raw_vote(ctx, d, two, keep, nk, 0.5) == (ffi.AZ_ERR_INVALID, True)
    assert raw_vote(ctx, d, [0, 20, 10], keep, [1, 1], 0.5) == (ffi.AZ_ERR_INVALID, True)
    assert raw_vote(ctx, d, [0, 4097], keep, [1], 0.5) == (ffi.AZ_ERR_CAPACITY, True)
    assert raw_vote(ctx, d, two, keep, [1, 3], float("nan")) == (ffi.AZ_ERR_INVALID, True)
    # nothing to do is fine
    assert ctx.soft_nms_batched([], "linear", 0.3) == [] and ctx.box_vote_batched([], [], 0.5) == []
    e = np.zeros((0, 5), np.float32)
    got = ctx.soft_nms_batched([e, e], "gaussian", 0.3)
    assert [g[0].size for g in got] == [0, 0] and [v.shape for v in ctx.box_vote_batched([e, e], [[], []], 0.5)] == [(0, 4)] * 2
    assert [v.shape for v in ctx.box_vote_batched([group(65), e], [[], []], 0.5)] == [(0, 4)] * 2
    with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
        ctx.soft_nms_batched([e], "soft", 0.3)


# ---- Soft-NMS, gaussian: order against float64, scores by the 8x rule ------------------------------------------------------------
def test_gaussian_against_float64(ctx):
    sets = [P.gaussian_case(n) for n in P.GAUSS_SIZES]
    got = ctx.soft_nms_batched(sets, "gaussian", P.GAUSS["thresh"], P.GAUSS["sigma"], P.GAUSS["min_score"])
    worst = 0.0
    for n, d, (gk, gs) in zip(P.GAUSS_SIZES, sets, got):
        k64, s64 = P.soft_nms_ref(d, "gaussian", dtype=np.float64, **P.GAUSS)
        k32, s32 = P.soft_nms_ref(d, "gaussian", dtype=np.float32, **P.GAUSS)
        assert gk.size == k64.size and np.array_equal(gk, k64), "%d boxes: the picks differ from the float64 restatement's" % n
        e_dev, e_32 = rel_err(gs, s64), rel_err(s32, s64)
        ratio = e_dev / max(e_32, 1e-6 / 8)
        worst = max(worst, ratio)
        print("  gaussian, %3d boxes: %3d picked, device vs float64 %.3e, float32 restatement vs float64 %.3e, ratio %.2f (bound 8)"
              % (n, gk.size, e_dev, e_32, ratio))
        assert e_dev <= bound(e_32), n
    print("  gaussian: worst ratio %.2f" % worst)
    # thresh plays no part
    again = ctx.soft_nms_batched(sets, "gaussian", 0.9, P.GAUSS["sigma"], P.GAUSS["min_score"])
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, again))


# ---- box voting: bit for bit --------------------------------------------------------------------------------------------------
def test_voting_at_every_group_size(ctx):
    for kind in ("hard", "linear"):
        keeps = {n: ref(n, group(n), kind, 0.3, 0.001)[0] for n in SIZES}
        for vt in (0.0, 0.5, 0.8, 1.0):
            got = ctx.box_vote_batched([group(n) for n in SIZES], [keeps[n] for n in SIZES], vt)
            for n, v in zip(SIZES, got):
                want = P.box_vote_ref(group(n), keeps[n], vt)
                assert v.shape == want.shape and v.dtype == np.float32
                assert np.array_equal(v, want), "%d boxes, %s keep list, vote_thresh %g: max |d| %.3e" % (n, kind, vt, float(np.max(np.abs(v - want))))
                if vt == 1.0 and n:
                    assert np.array_equal(v, group(n)[keeps[n], :4])        # distinct boxes: the self vote alone, s * b / s


def test_voting_far_coordinates_zero_scores_and_exact_sums(ctx):
    cases = {}
    far = P.clustered_group(21, 120).copy()
    far[:, :4] += np.float32(1e4)
    cases["near 1e4"] = far
    some = P.clustered_group(22, 90).copy()
    some[::3, 4] = 0.0
    cases["voters of score 0"] = some
    cases["all scores 0"] = P.equal_scores(P.clustered_group(23, 70), 0.0)
    for n in (40, 257):
        cases["whole numbers %d" % n] = P.whole_number_group(n, n)
    names = sorted(cases)
    keeps = [P.soft_nms_ref(cases[k], "linear", 0.3, 0.5, 0.0)[0] for k in names]        # (min_score 0: zero scores are kept too)
    for vt in (0.0, 0.5, 0.8):
        got = ctx.box_vote_batched([cases[k] for k in names], keeps, vt)
        for k, kp, v in zip(names, keeps, got):
            assert np.array_equal(v, P.box_vote_ref(cases[k], kp, vt)), (k, vt)
            if k.startswith("whole"):
                assert np.array_equal(v, P.box_vote_exact(cases[k], kp, vt)), (k, vt)
            if k == "all scores 0":
                assert np.array_equal(v, cases[k][kp, :4])                           # sw == 0: as it was
    # a keep list may name a box twice and need not come from NMS
    d = cases["near 1e4"]
    v = ctx.box_vote_batched([d], [[5, 5, 0]], 0.5)[0]
    assert np.array_equal(v, P.box_vote_ref(d, [5, 5, 0], 0.5)) and np.array_equal(v[0], v[1])


def test_single_set_wrappers(ctx):
    from utils import cython_nms
    d = group(65)
    keep, sc = cython_nms.soft_nms(d)
    want = ref(65, d, "linear", 0.3, 0.001)
    assert isinstance(keep, list) and keep == want[0].tolist() and np.array_equal(sc, want[1])
    assert np.array_equal(cython_nms.box_vote(d, keep), P.box_vote_ref(d, keep, 0.8))
    assert cython_nms.soft_nms(d, "hard", 0.5, min_score=P.hard_min_score(d))[0] == cython_nms.nms(d, 0.5)


# ---- through the front door -------------------------------------------------------------------------------------------------
def same(a, b):
    return len(a) == len(b) and all(
        len(x) == len(y) and all((isinstance(u, list) and u == [] and isinstance(v, list) and v == []) or
                                 (not isinstance(u, list) and not isinstance(v, list) and u.dtype == v.dtype and np.array_equal(u, v))
                                 for u, v in zip(x, y)) for x, y in zip(a, b))


def test_postprocess_detections_under_each_setting(monkeypatch):
    from detect import test as T
    from detect.config import cfg
    for k in ("NMS_METHOD", "BBOX_VOTE", "NMS", "SOFT_NMS_SIGMA", "SOFT_NMS_MIN_SCORE", "BBOX_VOTE_THRESH"):
        monkeypatch.setattr(cfg.TEST, k, cfg.TEST[k])
    boxes = P.front_door_boxes()
    assert same(T.postprocess_detections(boxes), T.apply_nms(boxes, cfg.TEST.NMS))              # the defaults
    for method, vote in (("hard", False), ("hard", True), ("linear", False), ("linear", True)):
        cfg.TEST.NMS_METHOD, cfg.TEST.BBOX_VOTE = method, vote
        got = T.postprocess_detections(boxes)
        want = P.postprocess_ref(boxes, method, cfg.TEST.NMS, cfg.TEST.SOFT_NMS_SIGMA, cfg.TEST.SOFT_NMS_MIN_SCORE, vote,
                                 cfg.TEST.BBOX_VOTE_THRESH)
        assert same(got, want), (method, vote)
        assert got[0] == [[], [], [], []] and all(g.shape[1] == 5 for c in got for g in c if not isinstance(g, list))
    # the planted near-duplicates: gone under NMS, kept at a lower score under linear Soft-NMS
    cfg.TEST.NMS_METHOD, cfg.TEST.BBOX_VOTE = "linear", False
    soft = T.postprocess_detections(boxes)
    hard = T.apply_nms(boxes, cfg.TEST.NMS)
    assert sum(len(g) for c in soft for g in c) > sum(len(g) for c in hard for g in c)


def test_eval_det_tool_with_the_flags(tmp_path):
    all_boxes = [[[] for _ in range(4)] for _ in range(21)]
    for c in range(1, 21):
        for i in range(4):
            d = P.clustered_group(100 * c + i, 12 + c, clusters=2, span=250.0).copy()
            d[:, 2:4] = np.minimum(d[:, 2:4], [[499, 374]])
            all_boxes[c][i] = d
    det = tmp_path / "detections.pkl"
    with open(det, "wb") as f:
        pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)
    tools = os.path.join(REPO, "az-net_amd", "tools")
    p = subprocess.run([sys.executable, os.path.join(tools, "eval_det.py"), str(det), "--imdb", "synthetic_375x500_4",
                        "--out", str(tmp_path / "soft"), "--soft-nms", "linear", "--bbox-vote"], cwd=tools, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("!!! class")]
    assert len(lines) == 20 and "Results:" in p.stdout and "Applying NMS to all detections" in p.stdout
    assert os.path.exists(tmp_path / "soft" / "class1_pr.mat")
    assert pickle.load(open(det, "rb"))[3][2].shape == all_boxes[3][2].shape           # the saved run is read, never rewritten
