"""GPU: iterative box localisation (az_detect_iter / az_detect_iter_skip; restatement and cases: tests/iterloc_ref.py).

The yardstick of the device loop is the host loop over the existing az_detect -- iterloc_ref.iter_ref with AzContext.detect
as its one-shot detection: download, select in NumPy, az_detect on the selected boxes, take the class column.  A roi's bits
do not depend on its batch, so every comparison is array_equal (iterloc_ref.same).  On bias-only heads and on the integer
head the device loop is also held against iter_ref over det_infer_ref.detect_ref with the head's exact deltas (dw = dh = 0:
the decode is a pure f64 expression) and the device's own probabilities of a row, as tests/test_gpu_det_infer_edges.py does."""
import ctypes
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

import det_infer_ref as D
import iterloc_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
H, W, SCALE = R.IMAGE
C = D.BIAS_DIMS["C"]


@pytest.fixture(scope="module")
def env():
    import torch
    from aznet_hip import ffi, synth
    from oracle import az_oracle as orc
    return torch, ffi, synth, orc


def _context(env, Cn=C, fmap=None, **kw):
    torch, ffi, synth, orc = env
    c = ffi.AzContext(0, **kw)
    c.load_head(synth.make_head(seed=1, C=Cn, n6=8, n71=4, n72=4))
    c.load_det_head(D.clip_head() if Cn == C else synth.make_det_head(seed=2, C=Cn, n6=8, n7=8, ncls=2))
    c.set_feature_map(fmap if fmap is not None else np.random.RandomState(1).rand(1, Cn, *D.MAP_HW).astype(np.float32))
    return c


@pytest.fixture(scope="module")
def ctx(env):
    c = _context(env, gemm_mode=0)
    yield c
    c.close()


def host_loop(c, boxes, rounds, ms, mr, hw=(H, W), scale=SCALE, skip=False, **kw):
    det = c.detect_skip if skip else c.detect
    return R.iter_ref(lambda b: det(b, scale, hw[0], hw[1], **kw), boxes, rounds, ms, mr)


def device(c, boxes, rounds, ms, mr, hw=(H, W), scale=SCALE, skip=False, **kw):
    return c.detect_iter(boxes, scale, hw[0], hw[1], rounds, ms, mr, skip=skip, **kw)


def bias_ref(c, head, boxes, rounds, ms, mr, hw=(H, W), scale=SCALE, dedup=1. / 16., batch_size=10000, eps=1e-14):
    """iter_ref over detect_ref: the head's deltas as they are, the probabilities of a row as the device gives them."""
    p = c.detect(boxes[:1], scale, hw[0], hw[1])[0][0]
    fn = lambda index, rois_u: (np.tile(p, (len(index), 1)), np.tile(head["bb"], (len(index), 1)))      # noqa: E731
    return R.iter_ref(lambda b: D.detect_ref(b, scale, dedup, batch_size, hw, eps, fn), boxes, rounds, ms, mr)


def agree(c, boxes, rounds, ms, mr, head=None, **kw):
    got = device(c, boxes, rounds, ms, mr, **kw)
    assert R.same(got, host_loop(c, boxes, rounds, ms, mr, **kw)) is None
    if head is not None:
        assert R.same(got, bias_ref(c, head, boxes, rounds, ms, mr, **kw)) is None
    return got


def between(p, k):
    """A threshold that k of the class scores p[1:] pass: the k-th highest of them itself (a score present in the data)."""
    return float(np.sort(p[1:])[::-1][k - 1])


# ---- round 1 ------------------------------------------------------------------------------------------------------------------
def test_one_round_is_az_detect(ctx):
    head = D.class_head(21)
    ctx.load_det_head(head)
    boxes = R.spread_boxes(65, H, W)
    s, b = ctx.detect(boxes, SCALE, H, W)
    s1, b1, ex = ctx.detect_iter(boxes, SCALE, H, W, 1, 0.0, 1000)
    assert np.array_equal(s, s1) and np.array_equal(b, b1) and ex["count"].size == 0 and ex["cls"].size == 0
    # rounds == 1 does not read the extras pointers
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))      # noqa: E731
    s2, b2 = np.empty_like(s), np.empty_like(b)
    rc = ctx.L.az_detect_iter(ctx.h, p(boxes, ctypes.c_double), 65, SCALE, 1. / 16., 10000, H, W, 1e-14, 1, 0.0, 1000,
                              p(s2, ctypes.c_float), p(b2, ctypes.c_double), None, None, None, None, None)
    assert rc == 0 and np.array_equal(s, s2) and np.array_equal(b, b2)
    # no boxes: AZ_OK, zero counts
    s0, b0, ex0 = ctx.detect_iter(np.zeros((0, 4)), SCALE, H, W, 3, 0.0, 10)
    assert s0.shape == (0, 21) and b0.shape == (0, 84) and ex0["count"].tolist() == [0, 0] and ex0["box"].shape == (0, 4)


# ---- heads, rounds, row counts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5, 65, 300])
@pytest.mark.parametrize("rounds", [2, 3])
def test_bias_and_class_heads_equal_the_host_loop_and_the_restatement(ctx, P, rounds):
    boxes = R.spread_boxes(P, H, W)
    for head in (R.shift_head(3, bc=[0.0, 1.0, 0.5]), D.class_head(21)):
        ctx.load_det_head(head)
        p = ctx.detect(boxes[:1], SCALE, H, W)[0][0]
        ncls = p.size
        for ms, mr in ((0.0, 1000), (between(p, max(1, (ncls - 1) // 4)), 1000), (between(p, 2), 100)):
            got = agree(ctx, boxes, rounds, ms, mr, head=head)
            n_pass = int((p[1:] >= np.float32(ms)).sum()) * P
            assert got[2]["count"].tolist() == [min(n_pass, mr)] * (rounds - 1)      # (every row scores alike: no round thins out)
            assert got[2]["round"].tolist() == sum([[r + 2] * min(n_pass, mr) for r in range(rounds - 1)], [])


@pytest.mark.parametrize("P", [1, 5, 65, 300])
def test_scores_that_differ_from_row_to_row(ctx, P):
    # fc6 reads the pooled map: every roi has its own scores, so later rounds thin out and the cut falls between distinct scores
    ctx.load_det_head(R.row_score_head(21))
    boxes = R.spread_boxes(P, H, W, seed=P)
    s = ctx.detect(boxes, SCALE, H, W)[0]
    assert np.unique(s[:, 1:]).size > P                       # (not a bias-only head)
    ms = float(np.sort(s[:, 1:].ravel())[::-1][min(s[:, 1:].size - 1, 2 * P)])
    n = int((s[:, 1:] >= np.float32(ms)).sum())
    assert n >= min(2 * P + 1, s[:, 1:].size)
    for rounds in (2, 3):
        got = agree(ctx, boxes, rounds, ms, 1000)
        assert got[2]["count"][0] == min(n, 1000)
        agree(ctx, boxes, rounds, ms, max(1, P // 2))
    agree(ctx, boxes, 8, ms, 1000)                            # the most rounds the entry takes


@pytest.fixture(scope="module")
def int_case(env):
    return D.int_case(env[3])


def test_integer_head(env, int_case):
    case = int_case
    c = _context(env, 12, fmap=case["fmap"], gemm_mode=0)
    try:
        c.load_det_head(case["zero_sizes"])
        ih, iw = case["im"]
        fn = lambda index, rois_u: c.det_forward(rois_u)      # noqa: E731  (the deltas are exact multiples of 2^-k, dw = dh = 0)
        for P in (1, 5, 65, 300):
            boxes = case["boxes"][:P]
            s = c.detect(boxes, 1.0, ih, iw, batch_size=64)[0]
            ms = float(np.sort(s[:, 1:].ravel())[::-1][min(s[:, 1:].size - 1, P)])
            for rounds in (2, 3):
                got = device(c, boxes, rounds, ms, 1000, hw=(ih, iw), scale=1.0, batch_size=64)
                assert R.same(got, host_loop(c, boxes, rounds, ms, 1000, hw=(ih, iw), scale=1.0, batch_size=64)) is None
                ref = R.iter_ref(lambda b: D.detect_ref(b, 1.0, 1. / 16., 64, (ih, iw), 1e-14, fn), boxes, rounds, ms, 1000)
                assert R.same(got, ref) is None and got[2]["count"][0] >= 1
    finally:
        c.close()


@pytest.mark.parametrize("ncls", [2, 21, 256])
def test_class_counts(ctx, ncls):
    boxes = R.spread_boxes(65, H, W)
    for head in (D.class_head(ncls), R.row_score_head(ncls)):
        ctx.load_det_head(head)
        s = ctx.detect(boxes, SCALE, H, W)[0]
        ms = float(np.median(s[:, 1:]))
        for mr in (1000, 4096, 37):
            got = agree(ctx, boxes, 3, ms, mr, head=head if head["W6"].max() == 0 else None)
            assert got[2]["cls"].min() >= 1 and got[2]["cls"].max() < ncls and got[2]["count"][0] > 0


# ---- the threshold -----------------------------------------------------------------------------------------------------------
def test_min_score_above_all_zero_and_exactly_a_score(ctx):
    ctx.load_det_head(R.row_score_head(21))
    boxes = R.spread_boxes(65, H, W)
    s = ctx.detect(boxes, SCALE, H, W)[0]
    top = np.sort(s[:, 1:].ravel())[::-1]
    got = agree(ctx, boxes, 3, float(np.nextafter(top[0], np.float32(2))), 1000)
    assert got[2]["count"].tolist() == [0, 0] and got[2]["cls"].size == 0          # no extras, the loop ends
    got = agree(ctx, boxes, 3, float(top[0]), 1000)                                # exactly the highest score: kept (>=)
    assert got[2]["count"][0] == int((s[:, 1:] == top[0]).sum()) >= 1
    got = agree(ctx, boxes, 2, float(top[9]), 1000)
    assert got[2]["count"].tolist() == [int((s[:, 1:] >= top[9]).sum())]
    # a double just above a score that rounds to it in float32: the comparison is the float32 one
    ms = float(top[9]) + (float(np.nextafter(top[9], np.float32(2))) - float(top[9])) * 0.25
    assert np.float32(ms) == top[9] and ms > float(top[9])
    assert agree(ctx, boxes, 2, ms, 1000)[2]["count"].tolist() == got[2]["count"].tolist()
    got = agree(ctx, boxes, 3, 0.0, 1000)                                          # everything passes: the cap bites
    assert got[2]["count"].tolist() == [1000, 1000]
    got = agree(ctx, boxes, 2, -1.0, 4096)
    assert got[2]["count"].tolist() == [65 * 20]


# ---- the cap -----------------------------------------------------------------------------------------------------------------
def test_max_rows_around_the_passing_count_and_ties_across_the_cut(ctx):
    boxes = R.spread_boxes(65, H, W)
    ctx.load_det_head(R.row_score_head(21))
    s = ctx.detect(boxes, SCALE, H, W)[0]
    ms = float(np.sort(s[:, 1:].ravel())[::-1][99])
    n = int((s[:, 1:] >= np.float32(ms)).sum())
    for mr in (1, n - 1, n, n + 1):
        got = agree(ctx, boxes, 3, ms, mr)
        assert got[2]["count"][0] == min(n, mr)
    # every row scores alike (a bias-only head): the cut falls inside a class's run of equal scores -> the lowest f
    head = D.class_head(21)
    ctx.load_det_head(head)
    p = ctx.detect(boxes[:1], SCALE, H, W)[0][0]
    for mr in (1, 64, 65, 66, 100, 131):
        got = agree(ctx, boxes, 3, between(p, 3), mr, head=head)
        assert got[2]["count"].tolist() == [mr, mr]
    best = 1 + int(np.argmax(p[1:]))
    got = agree(ctx, boxes, 2, 0.0, 70, head=head)
    assert (got[2]["cls"] == best).sum() >= 65 and np.all(np.diff(got[2]["cls"]) >= 0)      # (still in ascending f)
    # all classes equal: the first max_rows pairs in f
    uni = D.bias_head(5, np.zeros(20))
    ctx.load_det_head(uni)
    got = agree(ctx, boxes, 2, 0.0, 100, head=uni)
    assert got[2]["cls"].tolist() == [1] * 65 + [2] * 35 and got[2]["src"].tolist() == list(range(65)) + list(range(35))


def test_four_thousand_and_ninety_six_rows(ctx):
    ctx.load_det_head(R.row_score_head(21))
    boxes = R.spread_boxes(300, H, W)
    got = agree(ctx, boxes, 2, 0.0, 4096)
    assert got[2]["count"].tolist() == [4096]
    got = agree(ctx, boxes, 3, 0.0, 4095)
    assert got[2]["count"].tolist() == [4095, 4095]


# ---- the dedup inside a round ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 10000])
def test_batch_sizes_and_duplicates_among_the_selected_boxes(ctx, batch):
    # rows that repeat (and rows a fraction of a cell apart): their refined boxes repeat as well, and classes whose deltas
    # differ by less than a cell merge -- the dedup inside a round must not show
    boxes = D.chunk_boxes(40, H, W, SCALE)
    head = D.class_head(21)
    ctx.load_det_head(head)
    p = ctx.detect(boxes[:1], SCALE, H, W)[0][0]
    for dd in (1. / 16., 0.0):
        got = agree(ctx, boxes, 3, between(p, 4), 1000, head=head, batch_size=batch, dedup=dd)
        assert got[2]["count"].tolist() == [160, 160]
        assert np.unique(got[2]["box"][:160], axis=0).shape[0] < 160
    got = agree(ctx, boxes, 3, between(p, 4), 1000, head=head, batch_size=batch, eps=1.0)
    ctx.load_det_head(R.row_score_head(21))
    agree(ctx, boxes, 3, 0.06, 50, batch_size=batch)


@pytest.mark.parametrize("hw_scale", D.IMAGES)
def test_clipped_and_degenerate_refined_boxes(ctx, hw_scale):
    h, w, scale = hw_scale
    head = D.clip_head()
    ctx.load_det_head(head)
    boxes = D.clip_anchors(h, w)
    for eps in (0.0, 1e-14):
        got = agree(ctx, boxes, 3, 0.0, 1000, head=head, hw=(h, w), scale=scale, eps=eps)
        n = len(boxes) * (len(D.CLIP_SHIFTS) - 1)
        assert got[2]["count"].tolist() == [n, n]
        bx = got[2]["box"]
        assert bx[:, 0].min() == 0 and bx[:, 2].max() == w - 1 and np.any(bx[:, 2] < bx[:, 0])      # clipped, and degenerate


# ---- the skip entry, a low-rank head, the 16-bit-term mode ---------------------------------------------------------------------
def test_skip_entry_equals_the_host_loop_over_az_detect_skip(env):
    torch, ffi, synth, orc = env
    Cs, hw = (4, 8, 4), ((152, 252), (76, 126), D.MAP_HW)
    rng = np.random.RandomState(3)
    maps = [torch.from_numpy(rng.rand(1, c, h, w).astype(np.float32)).cuda() for c, (h, w) in zip(Cs, hw)]
    c = _context(env, gemm_mode=0)
    try:
        c.load_det_head(R.row_score_head(21))
        c.load_skip_front(synth.make_skip_front(seed=1, Cs=Cs, Cout=C))
        c.set_skip_maps(maps)
        boxes = R.spread_boxes(65, H, W)
        s = c.detect_skip(boxes, SCALE, H, W)[0]
        ms = float(np.sort(s[:, 1:].ravel())[::-1][150])
        n = int((s[:, 1:] >= np.float32(ms)).sum())
        for rounds, mr in ((2, 1000), (3, 1000), (3, 100)):
            got = agree(c, boxes, rounds, ms, mr, skip=True)
            assert got[2]["count"][0] == min(mr, n) and n >= 151
        assert not np.array_equal(s, c.detect(boxes, SCALE, H, W)[0])             # (the front is not RoIPool of the last map)
    finally:
        c.close()
    bare = _context(env, gemm_mode=0)
    try:
        with pytest.raises(ffi.AzError) as e:                                     # no front: the skip entries' own refusal
            bare.detect_iter(R.spread_boxes(5, H, W), SCALE, H, W, 2, 0.0, 10, skip=True)
        assert e.value.code == ffi.AZ_ERR_STATE
    finally:
        bare.close()


def test_planted_lowrank_head(env):
    import head_sizes_ref as HS
    import lowrank_ref as LR
    torch, ffi, synth, orc = env
    pool = lambda f, r: orc.roi_pool(f[0], r)      # noqa: E731
    case = LR.planted_head(21, 8, 8, pool=pool)
    c = ffi.AzContext(0, max_regions=512, gemm_mode=0)
    try:
        c.load_head(HS.int_az_case((LR.DIMS[0], 4, 4, 4), pool=pool)["head"])
        c.load_det_head(case["head"])
        assert (c.det_dims.get("r6", 0), c.det_dims.get("r7", 0)) == (8, 8)
        c.set_feature_map(case["fmap"])
        boxes = case["rois"][:65, 1:5].astype(np.float64)
        s = c.detect(boxes, 1.0, HS.IM_H, HS.IM_W)[0]
        ms = float(np.sort(s[:, 1:].ravel())[::-1][200])
        for rounds, mr in ((2, 512), (3, 64)):
            got = device(c, boxes, rounds, ms, mr, hw=(HS.IM_H, HS.IM_W), scale=1.0)
            assert R.same(got, host_loop(c, boxes, rounds, ms, mr, hw=(HS.IM_H, HS.IM_W), scale=1.0)) is None
            assert got[2]["count"][0] == min(mr, int((s[:, 1:] >= np.float32(ms)).sum()))
    finally:
        c.close()


def test_gemm_mode_three_against_the_host_loop_in_that_mode(env, int_case):
    # (the integer head's sizes, 12 x 132 x 100 x 21: fc6 on three bf16 terms, as tests/test_gpu_head_sizes.py runs them)
    case = int_case
    c = _context(env, 12, fmap=case["fmap"], gemm_mode=3)
    try:
        c.load_det_head(case["head"])
        ih, iw = case["im"]
        for P in (65, 300):
            boxes = case["boxes"][:P]
            s = c.detect(boxes, 1.0, ih, iw)[0]
            ms = float(np.sort(s[:, 1:].ravel())[::-1][3 * P])
            got = agree(c, boxes, 3, ms, 1000, hw=(ih, iw), scale=1.0)
            assert got[2]["count"][0] == min(1000, int((s[:, 1:] >= np.float32(ms)).sum()))
    finally:
        c.close()


def test_device_count_variant_gives_the_same_answers(env, monkeypatch):
    # AZ_ITERLOC_SYNC=0: no round's row count is read back; every round is enqueued at max_rows rows, empty ones included
    monkeypatch.setenv("AZ_ITERLOC_SYNC", "0")
    c = _context(env, gemm_mode=0)
    monkeypatch.delenv("AZ_ITERLOC_SYNC")
    try:
        c.load_det_head(R.row_score_head(21))
        boxes = R.spread_boxes(65, H, W)
        s = c.detect(boxes, SCALE, H, W)[0]
        top = np.sort(s[:, 1:].ravel())[::-1]
        for ms, mr in ((float(top[150]), 1000), (float(top[150]), 64), (float(top[0]), 300), (2.0, 10), (0.0, 161)):
            agree(c, boxes, 4, ms, mr)
    finally:
        c.close()


# ---- state -------------------------------------------------------------------------------------------------------------------
def test_repeated_calls_and_a_call_after_a_larger_one(ctx):
    ctx.load_det_head(R.row_score_head(21))
    big, small = R.spread_boxes(300, H, W), R.spread_boxes(5, H, W, seed=9)
    want_small = host_loop(ctx, small, 3, 0.05, 50)
    want_big = host_loop(ctx, big, 3, 0.0, 700)
    for _ in range(2):
        assert R.same(device(ctx, big, 3, 0.0, 700), want_big) is None
        assert R.same(device(ctx, small, 3, 0.05, 50), want_small) is None         # stale rows of the larger call do not show
        assert R.same(device(ctx, small, 3, 0.05, 50), want_small) is None
    s, b = ctx.detect(small, SCALE, H, W)                                          # ... and az_detect behind it is itself
    assert np.array_equal(s, want_small[0]) and np.array_equal(b, want_small[1])
    # under profiling: the same answers, and the new launches by name
    ctx.set_profiling(2)
    try:
        assert R.same(device(ctx, big, 3, 0.0, 700), want_big) is None
        names = [n for n, _, _ in ctx.last_kernel_times()]
    finally:
        ctx.set_profiling(0)
    assert names.count("iter_select") == 2 and names.count("iter_take") == 2 and names.count("det_epilogue") == 3


def test_every_refusal_leaves_the_outputs_untouched(env, ctx):
    torch, ffi, synth, orc = env
    ctx.load_det_head(D.class_head(21))
    boxes = np.ascontiguousarray(R.spread_boxes(5, H, W))
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))      # noqa: E731

    def call(c=ctx, fn="az_detect_iter", **over):
        a = dict(boxes=p(boxes, ctypes.c_double), P=5, scale=SCALE, dedup=1. / 16., batch=10000, h=H, w=W, eps=1e-14, rounds=3,
                 ms=0.0, mr=10, drop=())
        a.update(over)
        rows = 2 * D.CAP                                          # (rounds - 1) * max_rows of the largest call that is taken
        out = dict(s=np.full((5, 21), -7, np.float32), b=np.full((5, 84), -7.0), cls=np.full(rows, -7, np.int32),
                   src=np.full(rows, -7, np.int32), sc=np.full(rows, -7, np.float32), bx=np.full((rows, 4), -7.0),
                   cnt=np.full(2, -7, np.int32))
        ptr = dict(s=p(out["s"], ctypes.c_float), b=p(out["b"], ctypes.c_double), cls=p(out["cls"], ctypes.c_int32),
                   src=p(out["src"], ctypes.c_int32), sc=p(out["sc"], ctypes.c_float), bx=p(out["bx"], ctypes.c_double),
                   cnt=p(out["cnt"], ctypes.c_int32))
        for k in a["drop"]:
            ptr[k] = None
        rc = getattr(c.L, fn)(c.h, a["boxes"], a["P"], a["scale"], a["dedup"], a["batch"], a["h"], a["w"], a["eps"], a["rounds"],
                              a["ms"], a["mr"], ptr["s"], ptr["b"], ptr["cls"], ptr["src"], ptr["sc"], ptr["bx"], ptr["cnt"])
        return rc, all(np.all(v == -7) for v in out.values())

    assert call() == (ffi.AZ_OK, False)
    INV, CAP, ST = ffi.AZ_ERR_INVALID, ffi.AZ_ERR_CAPACITY, ffi.AZ_ERR_STATE
    for over, code in ((dict(rounds=0), INV), (dict(rounds=9), INV), (dict(rounds=-1), INV), (dict(mr=0), INV), (dict(mr=4097), INV),
                       (dict(mr=-5), INV), (dict(P=-1), INV), (dict(boxes=None), INV), (dict(batch=0), INV), (dict(scale=0.0), INV),
                       (dict(scale=float("nan")), INV), (dict(drop=("cls",)), INV), (dict(drop=("src",)), INV),
                       (dict(drop=("sc",)), INV), (dict(drop=("bx",)), INV), (dict(drop=("cnt",)), INV),
                       (dict(P=ctx.max_regions + 1), CAP)):
        assert call(**over) == (code, True), over
    assert call(fn="az_detect_iter_skip") == (ST, True)                          # no front loaded
    assert "az_detect_iter" in ctx.L.az_last_error(ctx.h).decode()
    small = _context(env, gemm_mode=0, max_regions=D.CAP)
    try:
        small.load_det_head(D.class_head(21))
        assert call(c=small, mr=D.CAP + 1) == (CAP, True)                        # max_rows above the region capacity
        assert call(c=small, mr=D.CAP) == (ffi.AZ_OK, False)
    finally:
        small.close()
    bare = ffi.AzContext(0)
    try:
        assert call(c=bare) == (ST, True)                                        # no detection head
    finally:
        bare.close()
    with pytest.raises(ffi.AzError):                                             # the binding passes the refusal on
        ctx.detect_iter(boxes, SCALE, H, W, 9, 0.0, 10)
    got = ctx.detect_iter(boxes, SCALE, H, W, 3, 0.0, 10)                        # the context still works
    assert R.same(got, host_loop(ctx, boxes, 3, 0.0, 10)) is None


# ---- the nets and detect.test ---------------------------------------------------------------------------------------------
def test_nets_and_im_detect_refined(env, monkeypatch):
    torch, ffi, synth, orc = env
    from aznet_hip.net import HipAZNet, HipDetNet, HipFrcnnNet
    from detect import test as T
    from detect.config import cfg
    for k in ("ITER_LOC", "ITER_LOC_SCORE", "ITER_LOC_MAX"):
        monkeypatch.setattr(cfg.TEST, k, cfg.TEST[k])
    dhead = synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)
    Cn = synth.SMALL_DET_DIMS["C"]
    fmap = torch.from_numpy(synth.make_feature_map(5, Cn, 38, 50)).cuda().contiguous(memory_format=torch.channels_last)
    im = np.zeros((375, 500, 3), np.uint8)
    props = R.spread_boxes(40, 375, 500)
    args = (cfg.DEDUP_BOXES, cfg.SEAR.BATCH_SIZE, cfg.EPS)
    scale = T._im_scale(im.shape)[0]
    fnet = HipFrcnnNet(dhead, backbone=lambda blob: fmap, name="iterloc_full")
    try:
        s = fnet.detect(fmap, props, scale, im.shape, *args)[0]
        ms = float(np.sort(s[:, 1:].ravel())[::-1][120])
        got = fnet.detect_iter(fmap, props, scale, im.shape, *args, 3, ms, 100)
        want = R.iter_ref(lambda b: fnet.detect(fmap, b, scale, im.shape, *args), props, 3, ms, 100)
        assert R.same(got, want) is None and got[2]["count"][0] == 100
        cfg.TEST.ITER_LOC, cfg.TEST.ITER_LOC_SCORE, cfg.TEST.ITER_LOC_MAX = 3, ms, 100
        s2, b2, ex = T.im_detect_refined({"full": fnet}, im, props, fnet.num_classes)
        s1, b1 = T.im_detect({"full": fnet}, im, props, fnet.num_classes)
        assert np.array_equal(s1, s2) and np.array_equal(b1, b2) and s2.dtype == np.float64
        assert R.same((got[0], got[1], ex), want) is None
        cfg.TEST.ITER_LOC = 1
        assert T.im_detect_refined({"full": fnet}, im, props, fnet.num_classes)[2]["cls"].size == 0
        with pytest.raises(ffi.AzError) as e:                                    # more proposals than the region capacity
            fnet.detect_iter(fmap, np.tile(props, (fnet.ctx.max_regions // 40 + 1, 1)), scale, im.shape, *args, 2, ms, 100)
        assert e.value.code == ffi.AZ_ERR_CAPACITY
    finally:
        fnet.ctx.close()
    az = HipAZNet(synth.make_head(seed=77, **synth.SMALL_DIMS), name="iterloc_az")
    try:
        dnet = HipDetNet(dhead, az)
        az.set_conv(fmap)
        got = dnet.detect_iter(props, scale, im.shape, *args, 3, ms, 100)
        want = R.iter_ref(lambda b: dnet.detect(b, scale, im.shape, *args), props, 3, ms, 100)
        assert R.same(got, want) is None and got[2]["count"][0] == 100
        cfg.TEST.ITER_LOC = 3
        conv = {name: fmap for name in cfg.SEAR.FRCNN_CONV}
        s2, b2, ex = T.im_detect_refined({"fc": dnet}, im, props, dnet.num_classes, conv)
        assert R.same((s2.astype(np.float32), b2, ex), want) is None
    finally:
        az.ctx.close()


def test_test_det_net_with_iter_loc_and_bbox_vote(tmp_path):
    from detect import config as Cf
    rng = np.random.Generator(np.random.PCG64(2))
    props = []
    for n in (30, 0, 25, 33):
        x1, y1 = rng.uniform(0, 440, n), rng.uniform(0, 320, n)
        props.append(np.stack([x1, y1, np.minimum(x1 + rng.uniform(20, 400, n), 499), np.minimum(y1 + rng.uniform(20, 300, n), 374)], 1))
    pf = str(tmp_path / "proposals.pkl")
    with open(pf, "wb") as f:
        pickle.dump({"boxes": props, "time": 0.0, "recall": 0}, f)
    env = dict(os.environ)
    env["AZ_BACKBONE_DETERMINISTIC"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([TOOLS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    rows, roots = {}, []
    try:
        for tag, flags in (("plain", []), ("iter", ["--iter-loc", "2", "--iter-loc-score", "0.0", "--iter-loc-max", "50"])):
            exp = "iterloc_test_%s_%d" % (tag, os.getpid())
            roots.append(os.path.join(Cf.cfg.ROOT_DIR, "output", exp))
            r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(TOOLS, "test_det_net.py"), "--gpu", "0",
                                "--net", "synthetic:7", "--prop", pf, "--imdb", "synthetic_375x500_4", "--bbox-vote", "--exp", exp]
                               + flags, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 0, r.stdout[-3000:]
            assert r.stdout.count("im_detect: ") == 3 and "Applying NMS to all detections" in r.stdout
            assert "On average, " in r.stdout
            assert ("'ITER_LOC': 2" in r.stdout) == (tag == "iter")
            df = os.path.join(roots[-1], "synthetic_375x500_4", "vgg16_frcnn_synthetic_7", "detections.pkl")
            with open(df, "rb") as f:
                dets = pickle.load(f)
            rows[tag] = sum(dets[j][i].shape[0] for j in range(1, 21) for i in (0, 2, 3))
            if tag == "iter":
                # the AP lines of these detections (the synthetic imdb has no evaluate_detections of its own: eval_det.py)
                q = subprocess.run([sys.executable, os.path.join(TOOLS, "eval_det.py"), df, "--imdb", "synthetic_375x500_4",
                                    "--out", str(tmp_path / "ap"), "--bbox-vote"], cwd=TOOLS, capture_output=True, text=True,
                                   timeout=600)
                assert q.returncode == 0, q.stderr[-3000:]
                assert len([ln for ln in q.stdout.splitlines() if ln.startswith("!!! class")]) == 20
        print("  detections.pkl rows: %d without --iter-loc, %d with" % (rows["plain"], rows["iter"]))
        assert rows["plain"] == 30 * 20 + 25 * 20 + 33 * 20 and rows["iter"] > rows["plain"]
    finally:
        for d in roots:
            shutil.rmtree(d, ignore_errors=True)
