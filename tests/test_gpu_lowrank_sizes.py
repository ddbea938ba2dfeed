"""GPU: the truncated-SVD detection head off its one size (cases: tests/lowrank_ref.py SIZES; premises:
tests/test_lowrank_sizes_host.py).  tests/test_gpu_lowrank.py runs one layer size (44, 260, 516) at ranks of at most 128 and
at most 300 rows, where every launch of k_lowrank_gemm has fewer tiles than workgroups.  Here:

  WIDE  (4, 2116, 8), 2304 regions    fc6_U has 34 n-tiles, the last 4 columns wide; at 2048 rows 1088 tiles fall on 1024
                                      workgroups, so 64 of them take a second item (m-tiles 30 and 31: rows 1920 .. 2047) --
                                      the grid-stride step, the recomputed tile indices and the un-barriered prologue of the
                                      second item.  r7 = 4: fc7_L with K = 2116.
  DEEP  (160, 260, 516), 512 regions  K6 = 7840: 62 chunks of 128 in fc6_L, the last one 32 long (the paper-sized head has
                                      61); ranks 132 / 256 / 260: two and three n-tiles in the L stage, azk_fc_reduce past
                                      column 128 of dlr_t, up to nine K steps in the U stage; r6 = 260 is min(out, in).
  TINY  (4, 8, 8), 64 regions         everything below one tile; a rank equal to n6.
  LONG  (672, 132, 8), 64 regions     K6 = 32928, the shallowest fc6 at which the n-tile term of azk_lowrank_split shows:
                                      206 chunks of 160 at rank 132 (two n-tiles: 256 chunks at most), 258 of 128 at
                                      rank 128.  No layer of the other sizes is deep enough for that term to matter.
  DIMS  (44, 260, 516), 512 regions   ranks above 128 at the size whose other paths are pinned already.

  2. the U-stage kernel alone at more tiles than workgroups, integers, bit for bit, the guard rows behind M untouched;
  3. planted integer factorisations of every size: bbox_pred of the low-rank head == az_load_det_head(U L) == the exact
     integers, cls_prob within 1e-6 of the float64 softmax, at the row counts of each size;
  4. random heads: the 8 x rule against the float64 / float32 restatements (DEEP, DIMS, az_det_forward_skip), a roi's bits
     alone and among others; WIDE bit for bit against 160-row launches (one turn), az_detect with duplicates, az_detect_batch;
  5. loads between sizes on one context against fresh contexts.
Every tolerance-based figure is printed before it is asserted (run with -s)."""
import functools

import numpy as np
import pytest

import det_infer_ref as D
import det_rows_ref as DR
import head_sizes_ref as H
import lowrank_ref as LR
import skip_ref as S
import train_step_ref as R

pytestmark = pytest.mark.gpu
ROWS = (1, 8, 31, 32, 33, 64, 65, 130, 161, 300)          # tests/test_gpu_lowrank.py's


def _pool(fmap, rois):
    from oracle import az_oracle as orc
    return orc.roi_pool(fmap[0], rois).reshape(rois.shape[0], -1)


def _context(name):
    """A context of a size's region capacity with a small AZ head of its C (az_set_feature_map needs one)."""
    from aznet_hip import ffi
    (C, n6, n7), cap, _ = LR.SIZES[name]
    ctx = ffi.AzContext(0, max_regions=cap, gemm_mode=0)
    ctx.load_head(R.filler_head(3, C, 4, 4, 4))
    return ctx


class Env(object):
    """One context per size, made on first use."""
    def __init__(self):
        self.ctxs = {}

    def ctx(self, name):
        if name not in self.ctxs:
            self.ctxs[name] = _context(name)
        return self.ctxs[name]

    def close(self):
        for c in self.ctxs.values():
            c.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()
    for f in (planted, rand, wide_random, wide_chunked):
        f.cache_clear()


def check(tag, got, r64, r32):
    e_dev, e_cpu = R.rel_err(got, r64), R.rel_err(r32, r64)
    b = R.bound(e_cpu)
    print("  %-44s device %.3e   float32-CPU %.3e   bound %.3e   ratio %.3f   %s"
          % (tag, e_dev, e_cpu, b, e_dev / e_cpu if e_cpu else 0.0, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


# ---- 2. the U-stage kernel alone, more tiles than workgroups ------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit_ctx():
    from aznet_hip import ffi
    ctx = ffi.AzContext(0, max_regions=LR.UNIT_BIG_CAP)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=2)
def unit_case(M, N, K):
    return LR.unit_case(M, N, K)


def _unit(ctx, case, M):
    X, W, b, Y = case
    for relu in (False, True):
        got = ctx.lowrank_gemm_unit(X, W, b, relu=relu, M=M)          # (AZ_ERR_HIP if a row behind M was written)
        want = (np.maximum(Y[:M], 0) if relu else Y[:M]).astype(np.float32)
        bad = np.flatnonzero((got != want).any(axis=1)) if got.shape == want.shape else None
        assert bad is not None and bad.size == 0, "M %d N %d K %d relu %d: %d rows differ, first %d, last %d" % (
            M, W.shape[0], W.shape[1], relu, bad.size, bad[0], bad[-1])


@pytest.mark.parametrize("shape", LR.UNIT_BIG, ids=lambda s: "M%d_N%d_K%d" % s)
def test_unit_second_items(unit_ctx, shape):
    """Y = X W^T + b on integers where nt * mt > 1024: the workgroups' second items, bit for bit."""
    case = unit_case(*shape)
    assert (case[3] < 0).any() and (case[3] > 0).any()
    _unit(unit_ctx, case, shape[0])


@pytest.mark.parametrize("M", LR.UNIT_BIG_MASKED[1])
def test_unit_second_items_hold_the_masked_last_m_tile(unit_ctx, M):
    """M = 64 q + 1: the last m-tile has one row, and its tiles are second items."""
    _unit(unit_ctx, unit_case(*LR.UNIT_BIG_MASKED[0]), M)


# ---- 3. planted exact factorisations at every size ----------------------------------------------------------------------------
PLANTED = tuple((name,) + case for name in ("WIDE", "DEEP", "TINY", "LONG", "DIMS") for case in LR.SIZES[name][2])


@functools.lru_cache(maxsize=None)
def planted(name, ncls, r6, r7):
    c = LR.sized_planted(name, ncls, r6, r7, pool=_pool)
    assert c["abs_sum"] < LR.EXACT
    return c


def _launches(name):
    """The row windows of a size's roi set: (the reference launches, the other windows)."""
    if name == "WIDE":
        n = 2048
        return [slice(0, n)], [w for k in LR.WIDE_ROWS for w in (slice(0, k), slice(n - k, n))] + [slice(j, j + 1) for j in (1920, 1999, 2047)]
    if name in ("TINY", "LONG"):
        return [slice(0, 64)], [slice(0, k) for k in LR.TINY_ROWS]
    return [slice(0, 300), slice(300, 812)], [slice(0, k) for k in ROWS]


@pytest.mark.parametrize("case", PLANTED, ids=lambda c: "%s_ncls%d_r6_%d_r7_%d" % c)
def test_planted_factorisation_matches_the_full_head(env, case):
    name, ranks = case[0], case[2:]
    ctx, c = env.ctx(name), planted(*case)
    rois, main, others = c["rois"], *_launches(name)
    ctx.set_feature_map(c["fmap"])
    ctx.load_det_head(c["full"])
    full = [ctx.det_forward(rois[w]) for w in main]
    for w, (p_full, b_full) in zip(main, full):
        assert same(b_full, c["bbox"][w]), "the full head on W = U L, rows %s" % (w,)
    ctx.load_det_head_lowrank(c["head"])
    assert (ctx.det_dims["r6"], ctx.det_dims["r7"]) == ranks
    p_all = np.zeros(c["p64"].shape, np.float32)
    for w, (p_full, b_full) in zip(main, full):
        p, b = ctx.det_forward(rois[w])
        bad = np.flatnonzero((b != b_full).any(axis=1))
        assert bad.size == 0, "bbox_pred, low rank against the full head, rows %s: %d rows differ (first %d, last %d)" % (
            w, bad.size, bad[0], bad[-1])
        e_lr, e_full = float(np.abs(p - c["p64"][w]).max()), float(np.abs(p_full - c["p64"][w]).max())
        print("  planted %s rows %d..%d: max |cls_prob - f64| low rank %.3e, full %.3e (k = %d, partial sums <= %.0f)"
              % (case, w.start, w.stop, e_lr, e_full, c["k"], c["abs_sum"]))
        assert e_lr <= 1e-6 and e_full <= 1e-6
        p_all[w] = p
    for w in others:
        pn, bn = ctx.det_forward(rois[w])
        assert same(bn, c["bbox"][w]), "bbox_pred, rows %s" % (w,)
        assert same(pn, p_all[w]), "cls_prob, rows %s against the same rows of the whole launch" % (w,)


# ---- 4. random heads --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rand(name, r6, r7):
    c = LR.sized_random(name, r6, r7)
    p5 = _pool(c["fmap"], c["rois"])
    c["r64"], c["r32"] = LR.head_on_pool5(c["head"], p5, np.float64), LR.head_on_pool5(c["head"], p5, np.float32)
    return c


def _head_fn(c, dtype):
    return lambda index, rois_u: LR.head_on_pool5(c["head"], _pool(c["fmap"], rois_u), dtype)


@pytest.mark.parametrize("case", LR.RANDOM_SIZES, ids=lambda c: "%s_r6_%d_r7_%d" % c)
def test_random_head_forward_and_detect(env, case):
    name, ranks = case[0], case[1:]
    ctx, c = env.ctx(name), rand(*case)
    rois, ok = c["rois"], True
    ctx.load_det_head(c["head"])
    assert (ctx.det_dims["r6"], ctx.det_dims["r7"]) == ranks
    ctx.set_feature_map(c["fmap"])
    print("random low-rank head %s" % (case,))
    refs = {}
    for w in (slice(0, 300), slice(300, 812)):
        refs[w.start] = ctx.det_forward(rois[w])
        for tensor, got, r64, r32 in zip(("cls_prob", "bbox_pred"), refs[w.start], c["r64"], c["r32"]):
            ok &= check("%s rows %d..%d" % (tensor, w.start, w.stop), got, r64[w], r32[w])
    # a roi's bits: alone, and among 1 ... 300 others
    ref = refs[0]
    for n in ROWS:
        for x, y in zip(ctx.det_forward(rois[:n]), ref):
            assert same(x, y[:n]), "prefix of the 300-row launch, %d rows" % n
    for j in (0, 63, 64, 137, 299):
        for x, y in zip(ctx.det_forward(rois[j:j + 1]), ref):
            assert np.array_equal(x[0], y[j]), "roi %d alone" % j
    for j in (0, 255, 511):
        for x, y in zip(ctx.det_forward(rois[300 + j:301 + j]), refs[300]):
            assert np.array_equal(x[0], y[j]), "roi %d of the 512-row launch alone" % j
    # az_detect: the decoded boxes and the scores of every proposal
    boxes = rois[:300, 1:].astype(np.float64)
    im_hw, eps = (H.IM_H, H.IM_W), 1e-14
    s, b = ctx.detect(boxes, 1.0, im_hw[0], im_hw[1], eps=eps)
    s64, b64, _ = D.detect_ref(boxes, [1.0], 1. / 16., 10000, im_hw, eps, _head_fn(c, np.float64))
    s32, b32, _ = D.detect_ref(boxes, [1.0], 1. / 16., 10000, im_hw, eps, _head_fn(c, np.float32))
    ok &= check("az_detect scores", s, s64, s32)
    ok &= check("az_detect boxes", b, b64, b32)
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


def test_det_forward_skip_runs_a_lowrank_head(env):
    """az_det_forward_skip on the skip fixture (S.SMALL_CS, Cout = 44) with the (36, 128) head."""
    import torch
    from aznet_hip import synth
    ctx = env.ctx("DIMS")
    c = LR.random_case(36, 128)
    ctx.load_det_head(c["head"])
    assert (ctx.det_dims["r6"], ctx.det_dims["r7"]) == (36, 128)
    front = synth.make_skip_front(seed=21, Cs=S.SMALL_CS, Cout=LR.DIMS[0])
    ctx.load_skip_front(front)
    maps = S.make_maps(5, S.SMALL_CS)
    ctx.set_skip_maps([torch.from_numpy(m).cuda() for m in maps])
    rois = S.random_rois(60)
    p, b = ctx.det_forward_skip(rois)
    r64 = LR.head_on_pool5(c["head"], S.pool5(front, maps, rois, np.float64), np.float64)
    r32 = LR.head_on_pool5(c["head"], S.pool5(front, maps, rois, np.float32), np.float32)
    assert np.abs(r64[1]).max() > 0
    ok = check("az_det_forward_skip cls_prob", p, r64[0], r32[0])
    ok &= check("az_det_forward_skip bbox_pred", b, r64[1], r32[1])
    for n in (1, 33):
        for x, y in zip(ctx.det_forward_skip(rois[:n]), (p, b)):
            assert same(x, y[:n]), "prefix of the 60-row launch, %d rows" % n
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


# WIDE: the rows of the second turn against launches that have none
@functools.lru_cache(maxsize=None)
def wide_random():
    return rand("WIDE", *LR.RANDOM_WIDE)


def _wide(env):
    ctx, c = env.ctx("WIDE"), wide_random()
    ctx.load_det_head(c["head"])                        # (the planted cases of part 3 may have run in between)
    assert (ctx.det_dims["r6"], ctx.det_dims["r7"]) == LR.RANDOM_WIDE
    ctx.set_feature_map(c["fmap"])
    return ctx, c


@functools.lru_cache(maxsize=None)
def wide_chunked(ctx):
    """(cls_prob, bbox_pred) of all 2048 rois from launches of 160 rows: 102 tiles, one turn."""
    rois = wide_random()["rois"]
    outs = [ctx.det_forward(rois[i:i + LR.CHUNK]) for i in range(0, rois.shape[0], LR.CHUNK)]
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def _detect_chunked(ctx, boxes):
    parts = [ctx.detect(boxes[i:i + LR.CHUNK], 1.0, H.IM_H, H.IM_W) for i in range(0, len(boxes), LR.CHUNK)]
    return np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])


def test_wide_random_head_same_bits_as_one_turn_launches(env):
    ctx, c = _wide(env)
    ref = wide_chunked(ctx)
    ok = True
    for tensor, got, r64, r32 in zip(("cls_prob", "bbox_pred"), ctx.det_forward(c["rois"]), c["r64"], c["r32"]):
        ok &= check("WIDE %s, 2048 rows" % tensor, got, r64, r32)
    for tensor, got, r64, r32 in zip(("cls_prob", "bbox_pred"), ref, c["r64"], c["r32"]):
        ok &= check("WIDE %s, 160-row launches" % tensor, got, r64, r32)
    for n in LR.WIDE_ROWS:
        for back in (False, True):
            rows = DR.window(n, back)
            for tensor, g, r in zip(("cls_prob", "bbox_pred"), ctx.det_forward(c["rois"][rows]), ref):
                bad = np.flatnonzero((g != r[rows]).any(axis=1))
                assert bad.size == 0, "%s, %d rows, %s window: %d rows differ (first %d, last %d of the window)" % (
                    tensor, n, "back" if back else "front", bad.size, bad[0], bad[-1])
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


@pytest.mark.parametrize("P,u", LR.FEW, ids=lambda v: str(v))
def test_wide_duplicates_under_a_large_bound(env, P, u):
    """az_detect of P = 2000 boxes of which u are distinct, against az_detect of the distinct boxes (in one-turn launches)."""
    ctx, c = _wide(env)
    boxes, distinct, rep = DR.few_unique(P, u)
    s, b = ctx.detect(boxes, 1.0, H.IM_H, H.IM_W)
    sr, br = _detect_chunked(ctx, distinct)
    ncls = c["head"]["Wc"].shape[0]
    assert s.shape == (P, ncls) and b.shape == (P, 4 * ncls) and np.abs(br).max() > 0
    assert np.array_equal(s, sr[rep]) and np.array_equal(b, br[rep])
    if u > LR.CHUNK:                                    # ... and az_detect of the distinct boxes in one call
        s1, b1 = ctx.detect(distinct, 1.0, H.IM_H, H.IM_W)
        assert np.array_equal(s1, sr) and np.array_equal(b1, br)


@pytest.mark.parametrize("counts", LR.BATCHES, ids=lambda v: "x".join(map(str, v)))
def test_wide_rows_of_several_images_share_second_turn_tiles(env, counts):
    from aznet_hip import synth
    ctx, c = _wide(env)
    C = LR.SIZES["WIDE"][0][0]
    maps = [synth.make_feature_map(80 + i, C, H.MAP_H, H.MAP_W) for i in range(len(counts))]
    boxes = DR.batch_boxes(counts)
    got = ctx.detect_batch(maps, boxes, [1.0] * len(counts), [(H.IM_H, H.IM_W)] * len(counts))
    for i, (m, bx) in enumerate(zip(maps, boxes)):
        ctx.set_feature_map(m)
        s1, b1 = ctx.detect(bx, 1.0, H.IM_H, H.IM_W)                  # the image alone: fewer tiles than workgroups
        assert np.array_equal(got[i][0], s1) and np.array_equal(got[i][1], b1), "image %d of %s" % (i, counts)
        sr, br = _detect_chunked(ctx, bx)
        assert np.array_equal(s1, sr) and np.array_equal(b1, br) and np.abs(br).max() > 0


# ---- 5. loads between sizes on one context ----------------------------------------------------------------------------------------
def test_loads_between_ranks_on_one_context(env):
    """Low rank (260, 260) -> (4, 0) -> full -> (0, 256) on one context: dlr_t, dpart and the L / U buffers are re-made at
    every load (dpart's size comes from another term of its maximum each time); each answers as a fresh context does,
    and a refused load in between leaves the previous answers."""
    from aznet_hip import ffi
    ctx = env.ctx("DIMS")
    cases = [LR.random_case(*r) if r else None for r in LR.LOAD_ORDER]
    full = cases[0]["uncompressed"]
    heads = [c["head"] if c else full for c in cases]
    fmap, rois = cases[0]["fmap"], cases[0]["rois"]
    C, n6, n7 = LR.DIMS
    z = lambda *s: np.zeros(s, np.float32)          # noqa: E731
    refused = {"L6": z(6, C * 49), "U6": z(n6, 6), "b6": z(n6), "W7": z(n7, n6), "b7": z(n7), "Wc": z(21, n7), "bc": z(21),
               "Wb": z(84, n7), "bb": z(84)}
    outs = []
    for r, head in zip(LR.LOAD_ORDER, heads):
        ctx.load_det_head(head)
        assert (ctx.det_dims.get("r6", 0), ctx.det_dims.get("r7", 0)) == (r or (0, 0))
        ctx.set_feature_map(fmap)
        got = ctx.det_forward(rois)
        fresh = _context("DIMS")
        try:
            fresh.load_det_head(head)
            fresh.set_feature_map(fmap)
            want = fresh.det_forward(rois)
        finally:
            fresh.close()
        for x, y in zip(got, want):
            assert same(x, y), "after the load of %s" % (r,)
        with pytest.raises(ffi.AzError) as e:
            ctx.load_det_head_lowrank(refused)
        assert e.value.code == ffi.AZ_ERR_INVALID
        for x, y in zip(ctx.det_forward(rois), want):
            assert same(x, y), "a refused load after %s leaves the loaded head answering as before" % (r,)
        outs.append(want[1])
    assert all(not np.array_equal(outs[0], o) for o in outs[1:]), "four different models"
