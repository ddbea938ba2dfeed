"""GPU: the skip-connection detector (az_skip.hip; models/COCO/VGG16_skip/frcnn/test_fc.prototxt) against the NumPy
restatement of tests/skip_ref.py.

Maps come from a 96 x 128 image (scaled pixels): conv3_3 24 x 32, conv4_3 12 x 16, conv5_3 6 x 8 cells.  Channel sets: the
reduced (20, 36, 12) -- no source a multiple of the wave width -- and the full (256, 512, 512).
  1. pool: az_skip_pool(normalise = 0) bit for bit against the restatement, its conv5_3 block bit for bit against az_roi_pool
  2. GRN: within train_step_ref.bound (8 x the float32 restatement's error against float64, floor 1e-6); zero blocks; one channel
  3. the 1x1 convolution on integer operands, bit for bit
  4. az_det_forward_skip / az_detect_skip against the float64 restatement, same bound; boxes 1e-4 of the box scale
  5. chunk seam (AZ_SKIP_CHUNK and + 1 rois), permutation, repetition, az_detect untouched by a front on its context
  6. every refusal of the ABI, and the context's answers afterwards
  7. detect.test (test_net, im_detect_shared) with a skip configuration; tools/test_det_net.py's loader on a model file
Every figure is printed before it is asserted (run with -s)."""
import contextlib
import os

import numpy as np
import pytest

import skip_ref as S
import train_step_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RED = dict(n6=260, n7=516)


@contextlib.contextmanager
def context(Cout, n6=4, n7=4, ncls=2, max_regions=512, gemm_mode=0, az_head=True, det_seed=9):
    """A context with a tiny AZ head (az_roi_pool and the 16-bit-term modes need one) and a detection head of C = Cout."""
    from aznet_hip import ffi, synth
    ctx = ffi.AzContext(0, max_regions=max_regions, gemm_mode=gemm_mode)
    try:
        if az_head:
            ctx.load_head(synth.make_head(seed=3, C=Cout, n6=4, n71=4, n72=4))
        head = synth.make_det_head(seed=det_seed, C=Cout, n6=n6, n7=n7, ncls=ncls)
        ctx.load_det_head(head)
        yield ctx, head
    finally:
        ctx.close()


def front_for(Cs, Cout, seed=1):
    from aznet_hip import synth
    return synth.make_skip_front(seed=seed, Cs=Cs, Cout=Cout, scales=S.SCALES[:len(Cs)] if len(Cs) != 3 else S.SCALES)


def cuda_maps(maps):
    import torch
    return [torch.from_numpy(m).cuda() for m in maps]


def check(tag, got, r64, r32):
    e_dev, e_cpu = R.rel_err(got, r64), R.rel_err(r32, r64)
    b = R.bound(e_cpu)
    print("  %-40s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (tag, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b


def all_rois():
    return np.concatenate([S.hostile_rois(), S.random_rois(115)], 0)          # 130: both forms of k_roi_pool


# ---- 1. pool ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", [S.SMALL_CS, S.FULL_CS], ids=["20x36x12", "256x512x512"])
def test_pool_bit_for_bit(Cs):
    maps, rois = S.make_maps(11, Cs), all_rois()
    want = S.cat_raw(maps, rois)
    # (the hostile set does what it is there for: whole rows pooled from nothing, and bins empty at 1/16 only)
    b3, b5 = want[:15 * 49, :Cs[0]], want[:15 * 49, Cs[0] + Cs[1]:]
    assert (np.abs(want[:2 * 49]).max() == 0) and ((b5.max(axis=1) == 0) & (b3.max(axis=1) > 0)).any()
    with context(Cs[2]) as (ctx, _):
        ctx.load_skip_front(front_for(Cs, Cs[2]))
        ctx.set_skip_maps(cuda_maps(maps))
        for n in (1, 15, 35, 130):
            got = ctx.skip_pool(rois[:n], normalise=False)
            assert got.shape == (n * 49, sum(Cs))
            assert np.array_equal(got, want[:n * 49]), n
        got = ctx.skip_pool(rois, normalise=False)
        ctx.set_feature_map(maps[2])                                   # the same conv5_3 through the golden-backed kernel
        for n in (35, 130):
            p5 = ctx.roi_pool(rois[:n]).reshape(n, Cs[2], 49).transpose(0, 2, 1).reshape(n * 49, Cs[2])
            assert np.array_equal(got[:n * 49, Cs[0] + Cs[1]:], p5), n


# ---- 2. GRN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cs", [S.SMALL_CS, S.FULL_CS], ids=["20x36x12", "256x512x512"])
def test_grn_within_bound(Cs):
    rois, ok = all_rois()[:40], True
    front = front_for(Cs, Cs[2])
    with context(Cs[2]) as (ctx, _):
        ctx.load_skip_front(front)
        for tag, zero in (("all sources", ()), ("conv4_3 zero", (1,)), ("all zero", (0, 1, 2))):
            maps = S.make_maps(12, Cs, zero=zero)
            ctx.set_skip_maps(cuda_maps(maps))
            got = ctx.skip_pool(rois, normalise=True)
            assert np.isfinite(got).all(), tag
            r64, r32 = S.cat_norm(maps, rois, dtype=np.float64), S.cat_norm(maps, rois, dtype=np.float32)
            assert np.isfinite(r32).all()
            ok &= check("concat5 %s %s" % (Cs, tag), got, r64, r32)
            o = 0
            for i, C in enumerate(Cs):
                if i in zero:
                    assert not got[:, o:o + C].any(), (tag, i)         # zeros, never NaN
                o += C
            # rows pooled from nothing (the two rois outside the map) are zeros as well
            assert not got[:2 * 49].any()
    assert ok, "concat5 exceeds 8 x the float32 restatement's error"


def test_grn_single_channel_is_the_gain():
    Cs, gain = S.SMALL_CS, 1000.0
    maps = S.make_maps(13, Cs)
    keep = (7, 35, 0)
    for m, k in zip(maps, keep):
        one = np.abs(m[:, k]) + np.float32(0.25)                       # positive everywhere
        m[:] = 0.0
        m[:, k] = one
    rois = all_rois()[:40]
    raw = S.cat_raw(maps, rois)
    for eps in (1e-10, 0.0):
        front = dict(front_for(Cs, Cs[2]), gain=gain, eps=eps)
        with context(Cs[2]) as (ctx, _):
            ctx.load_skip_front(front)
            ctx.set_skip_maps(cuda_maps(maps))
            got = ctx.skip_pool(rois, normalise=True)
        assert np.isfinite(got).all()
        ulp = float(np.spacing(np.float32(gain)))
        hit = raw > 0
        assert hit.sum() > 3 * 30 * 49 and np.array_equal(got != 0, hit)
        err = np.abs(got[hit].astype(np.float64) - gain).max()
        print("  single channel, eps %g: max |y - gain| = %.3e (1 ulp = %.3e)" % (eps, err, ulp))
        assert err <= ulp


# ---- 3. the 1x1 convolution ---------------------------------------------------------------------------------------------------
CONV_ROWS = (1, 48, 49, 50, 127, 128, 129, 294)
CONV_COUT = (12, 128, 132, 512)


@pytest.mark.parametrize("Cs", [(68,), (32, 64), S.FULL_CS], ids=["K68", "K96", "K1280"])
def test_conv_integer_bit_for_bit(Cs):
    K = sum(Cs)
    rng = np.random.Generator(np.random.PCG64(100 + K))
    cat = rng.integers(-3, 4, (max(CONV_ROWS), K)).astype(np.float32)
    done = 0
    for Cout in CONV_COUT:
        Wp = rng.integers(-3, 4, (Cout, K)).astype(np.float32)
        bp = rng.integers(-8, 9, Cout).astype(np.float32)
        assert float((np.abs(cat) @ np.abs(Wp).T).max()) + 8 < 2 ** 24       # every partial sum, in any order, is exact
        pre = cat.astype(np.float64) @ Wp.astype(np.float64).T + bp
        assert (pre < 0).any() and (pre > 0).any()                           # ReLU gates
        want = np.maximum(pre, 0).astype(np.float32)
        front = {"Cs": Cs, "scales": S.SCALES[:len(Cs)], "Wp": Wp, "bp": bp}
        with context(Cout) as (ctx, _):
            ctx.load_skip_front(front)
            for rows in CONV_ROWS:
                got = ctx.skip_conv(cat[:rows])
                assert got.shape == (rows, Cout)
                assert np.array_equal(got, want[:rows]), (K, Cout, rows)
                done += 1
    assert done == len(CONV_COUT) * len(CONV_ROWS), "none skipped"


# ---- 4. the whole head --------------------------------------------------------------------------------------------------------
def _head_case(ctx, head, front, maps, rois, boxes, tag, dedups=(0.5, 1. / 16.)):
    from oracle import az_oracle as orc
    ok = True
    ctx.load_skip_front(front)
    ctx.set_skip_maps(cuda_maps(maps))
    p, b = ctx.det_forward_skip(rois)
    r64, r32 = S.det_forward(front, head, maps, rois, np.float64), S.det_forward(front, head, maps, rois, np.float32)
    ok &= check("%s cls_prob" % tag, p, r64[0], r32[0])
    ok &= check("%s bbox_pred" % tag, b, r64[1], r32[1])
    # the pool5 blob itself: the rows the 1x1 convolution stores are what fc6 reads
    p5 = ctx.skip_conv(ctx.skip_pool(rois, normalise=True))
    p5 = p5.reshape(rois.shape[0], 49, -1).transpose(0, 2, 1).reshape(rois.shape[0], -1)
    ok &= check("%s pool5" % tag, p5, S.pool5(front, maps, rois, np.float64), S.pool5(front, maps, rois, np.float32))
    for dedup in dedups:
        s, bx = ctx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W, dedup=dedup)
        s64, bx64 = S.detect(orc, front, head, maps, boxes, 1.0, (S.IM_H, S.IM_W), dedup, np.float64)
        s32, _ = S.detect(orc, front, head, maps, boxes, 1.0, (S.IM_H, S.IM_W), dedup, np.float32)
        assert s.shape == s64.shape and bx.shape == bx64.shape
        ok &= check("%s detect scores, dedup %.4f" % (tag, dedup), s, s64, s32)
        # decoded boxes: 1e-4 relative to the box scale (tests/test_gpu_fullsize.py), here an image of 128 px
        np.testing.assert_allclose(bx, bx64, rtol=1e-4, atol=1e-4 * S.IM_W)
        # the un-dedup is a gather: a box's row is the row of its unique roi, bit for bit
        rb, index, inv = ctx.roi_dedup(boxes, 1.0, dedup=dedup)
        pu, _ = ctx.det_forward_skip(rb[index])
        assert np.array_equal(s, pu[inv]), dedup
    return ok


def _dup_boxes(n, seed):
    """n proposals, a third of them copies (exact, or within the 0.5 dedup's rounding cell) of earlier ones."""
    b = S.random_boxes(n, seed)
    b = np.rint(b / 4.0) * 4.0                                         # (x * 0.5 is an integer: a 0.4 px shift stays in its cell)
    k = n // 3
    b[n - k:] = b[:k]
    b[n - k:n - k // 2] += 0.4
    return b


@pytest.mark.parametrize("ncls", [21, 81])
def test_whole_head_reduced(ncls):
    Cs = S.SMALL_CS
    maps, rois, boxes = S.make_maps(14, Cs), np.concatenate([S.hostile_rois(), S.random_rois(45, 8)], 0), _dup_boxes(60, 5)
    with context(Cs[2], ncls=ncls, **RED) as (ctx, head):
        ok = _head_case(ctx, head, front_for(Cs, Cs[2]), maps, rois, boxes, "reduced %d" % ncls)
        s, _ = ctx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W, dedup=0.5)
        assert np.array_equal(s[40:], s[:20])                          # duplicated boxes: identical rows
        from oracle import az_oracle as orc
        n_unique = len(orc.roi_dedup(orc.get_rois_blob(boxes, 1.0), 0.5)[0])
        assert len(ctx.roi_dedup(boxes, 1.0, dedup=0.5)[1]) == n_unique <= 40
    assert ok, "a tensor exceeds 8 x the float32 restatement's error"


def test_whole_head_full_sizes():
    Cs = S.FULL_CS
    maps, rois, boxes = S.make_maps(15, Cs), S.random_rois(5, 9), S.random_boxes(5, 9)
    with context(512, n6=4096, n7=4096, ncls=21) as (ctx, head):
        ok = _head_case(ctx, head, front_for(Cs, 512), maps, rois, boxes, "full", dedups=(0.5,))
    assert ok, "a tensor exceeds 8 x the float32 restatement's error"


# ---- 5. chunks and determinism --------------------------------------------------------------------------------------------------
def test_chunks_permutation_repetition():
    from aznet_hip import ffi
    Cs = S.SMALL_CS
    maps = S.make_maps(16, Cs)
    with context(Cs[2], ncls=21, **RED) as (ctx, head):
        front = front_for(Cs, Cs[2])
        ctx.load_skip_front(front)
        ctx.set_skip_maps(cuda_maps(maps))
        for n in (ffi.AZ_SKIP_CHUNK, ffi.AZ_SKIP_CHUNK + 1):
            rois = S.random_rois(n, 21)
            rois[:15] = S.hostile_rois()
            p, b = ctx.det_forward_skip(rois)
            p2, b2 = ctx.det_forward_skip(rois)
            assert np.array_equal(p, p2) and np.array_equal(b, b2), "the same call twice"
            perm = np.random.Generator(np.random.PCG64(n)).permutation(n)
            assert perm[-1] != n - 1 or n == 1
            pp, bp = ctx.det_forward_skip(rois[perm])
            assert np.array_equal(pp, p[perm]) and np.array_equal(bp, b[perm]), "a roi's bits depend on its position (%d rois)" % n
            # the last roi alone: the one past the chunk seam when n = AZ_SKIP_CHUNK + 1
            p1, b1 = ctx.det_forward_skip(rois[n - 1:])
            assert np.array_equal(p1[0], p[n - 1]) and np.array_equal(b1[0], b[n - 1])
            cat = ctx.skip_pool(rois, normalise=True)
            assert np.array_equal(cat[perm.repeat(49) * 49 + np.tile(np.arange(49), n)], ctx.skip_pool(rois[perm], normalise=True))
            r64 = S.det_forward(front, head, maps, rois, np.float64)
            r32 = S.det_forward(front, head, maps, rois, np.float32)
            assert check("%d rois cls_prob" % n, p, r64[0], r32[0]) and check("%d rois bbox_pred" % n, b, r64[1], r32[1])
            boxes = S.random_boxes(n, 22)
            s, bx = ctx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W, dedup=0.0)        # no dedup: n unique rows
            s2, bx2 = ctx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W, dedup=0.0)
            assert np.array_equal(s, s2) and np.array_equal(bx, bx2)
            sp, bxp = ctx.detect_skip(boxes[perm], 1.0, S.IM_H, S.IM_W, dedup=0.0)
            assert np.array_equal(sp, s[perm]) and np.array_equal(bxp, bx[perm])


def test_az_detect_untouched_by_a_front():
    Cs = S.SMALL_CS
    maps, boxes, rois = S.make_maps(17, Cs), S.random_boxes(150, 23), S.random_rois(150, 24)
    with context(Cs[2], ncls=21, **RED) as (ctx, _):
        ctx.set_feature_map(maps[2])
        before = ctx.detect(boxes, 1.0, S.IM_H, S.IM_W) + ctx.det_forward(rois) + ctx.head_forward(rois)
        ctx.load_skip_front(front_for(Cs, Cs[2]))
        ctx.set_skip_maps(cuda_maps(maps))
        # conv5_3 is the context's ordinary map as well: both plain heads answer from it
        mid = ctx.detect(boxes, 1.0, S.IM_H, S.IM_W) + ctx.det_forward(rois) + ctx.head_forward(rois)
        ctx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W)
        ctx.det_forward_skip(rois)
        ctx.set_feature_map(maps[2])
        after = ctx.detect(boxes, 1.0, S.IM_H, S.IM_W) + ctx.det_forward(rois) + ctx.head_forward(rois)
        for a, m, z in zip(before, mid, after):
            assert np.array_equal(a, m) and np.array_equal(a, z)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def _refused(ffi, code, fn, *a, **k):
    with pytest.raises(ffi.AzError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals():
    from aznet_hip import ffi
    Cs = S.SMALL_CS
    maps, rois, boxes = S.make_maps(18, Cs), S.random_rois(20, 25), S.random_boxes(20, 26)
    front = front_for(Cs, Cs[2])
    # no detection head
    ctx = ffi.AzContext(0, max_regions=64)
    try:
        _refused(ffi, ffi.AZ_ERR_STATE, ctx.load_skip_front, front)
    finally:
        ctx.close()
    with context(Cs[2], ncls=21, **RED) as (ctx, head):
        # no front yet
        for fn, a in ((ctx.detect_skip, (boxes, 1.0, S.IM_H, S.IM_W)), (ctx.det_forward_skip, (rois,)),
                      (ctx.skip_pool, (rois,)), (ctx.skip_conv, (np.zeros((3, sum(Cs)), np.float32),)),
                      (ctx.set_skip_maps, (cuda_maps(maps),))):
            _refused(ffi, ffi.AZ_ERR_STATE, fn, *a)
        # a front, no maps
        ctx.load_skip_front(front)
        for fn, a in ((ctx.detect_skip, (boxes, 1.0, S.IM_H, S.IM_W)), (ctx.det_forward_skip, (rois,)), (ctx.skip_pool, (rois,))):
            _refused(ffi, ffi.AZ_ERR_STATE, fn, *a)
        ctx.set_skip_maps(cuda_maps(maps))
        ctx.set_feature_map(maps[2])
        want = ctx.det_forward_skip(rois) + ctx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W) + ctx.detect(boxes, 1.0, S.IM_H, S.IM_W)

        def same():
            got = ctx.det_forward_skip(rois) + ctx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W) + ctx.detect(boxes, 1.0, S.IM_H, S.IM_W)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)

        # loads that must leave the loaded front in place
        bad = [
            dict(front, Cs=(20, 36, 12, 4), scales=(0.5,) + S.SCALES, Wp=np.zeros((12, 72), np.float32)),    # four sources
            dict(front, Cs=(22, 34, 12)),                                                                   # not multiples of 4
            dict(front, Cs=(0, 56, 12)),
            dict(front, scales=(0.25, 0.0, 0.0625)),
            dict(front, Wp=np.zeros((16, sum(Cs)), np.float32), bp=np.zeros(16, np.float32)),               # Cout != the head's C
            dict(front, eps=-1.0),
        ]
        for f in bad:
            _refused(ffi, ffi.AZ_ERR_INVALID, ctx.load_skip_front, f)
            assert ctx.skip_dims["Cout"] == Cs[2]
            same()
        # maps whose channel counts differ from the front's, or too few of them: the maps set before stay
        wrong = S.make_maps(18, (20, 40, 12))
        _refused(ffi, ffi.AZ_ERR_INVALID, ctx.set_skip_maps, cuda_maps(wrong))
        _refused(ffi, ffi.AZ_ERR_INVALID, ctx.set_skip_maps, cuda_maps(maps[1:]))
        same()
        # bad arguments of the entries
        _refused(ffi, ffi.AZ_ERR_INVALID, ctx.detect_skip, boxes, 0.0, S.IM_H, S.IM_W)
        _refused(ffi, ffi.AZ_ERR_INVALID, ctx.detect_skip, boxes, 1.0, S.IM_H, S.IM_W, batch_size=0)
        same()
        # more rois than the region capacity (512)
        big_r, big_b = S.random_rois(513, 27), S.random_boxes(513, 28)
        _refused(ffi, ffi.AZ_ERR_CAPACITY, ctx.detect_skip, big_b, 1.0, S.IM_H, S.IM_W)
        _refused(ffi, ffi.AZ_ERR_CAPACITY, ctx.det_forward_skip, big_r)
        _refused(ffi, ffi.AZ_ERR_CAPACITY, ctx.skip_pool, big_r)
        same()
        # nothing and a single row are served
        assert ctx.det_forward_skip(rois[:0])[0].shape == (0, 21) and ctx.skip_pool(rois[:0]).shape == (0, sum(Cs))
        assert ctx.detect_skip(boxes[:0], 1.0, S.IM_H, S.IM_W)[0].shape == (0, 21)
        same()
    # a detection head of another C drops the front (it folds to the head's C): a clean refusal, not a stale answer
    with context(Cs[2], ncls=21, az_head=False, **RED) as (ctx, _):
        from aznet_hip import synth
        ctx.load_skip_front(front)
        ctx.set_skip_maps(cuda_maps(maps))
        ctx.det_forward_skip(rois)
        ctx.load_det_head(synth.make_det_head(seed=2, C=16, n6=8, n7=8, ncls=3))
        assert ctx.skip_dims is None
        for fn, a in ((ctx.det_forward_skip, (rois,)), (ctx.skip_pool, (rois,)), (ctx.set_skip_maps, (cuda_maps(maps),))):
            _refused(ffi, ffi.AZ_ERR_STATE, fn, *a)
        _refused(ffi, ffi.AZ_ERR_INVALID, ctx.load_skip_front, front)
    # a pyramid set on the context
    with context(Cs[2], ncls=21, **RED) as (ctx, _):
        ctx.load_skip_front(front)
        ctx.set_skip_maps(cuda_maps(maps))
        ok = ctx.det_forward_skip(rois)
        import torch
        m5 = torch.from_numpy(maps[2]).cuda().contiguous(memory_format=torch.channels_last)
        ctx.set_feature_pyramid([m5])
        for fn, a in ((ctx.detect_skip, (boxes, 1.0, S.IM_H, S.IM_W)), (ctx.det_forward_skip, (rois,)), (ctx.skip_pool, (rois,)),
                      (ctx.skip_conv, (np.zeros((3, sum(Cs)), np.float32),))):
            _refused(ffi, ffi.AZ_ERR_STATE, fn, *a)
        # ... and the pyramid entries still answer
        s, _ = ctx.detect_pyramid(boxes, [1.0], S.IM_H, S.IM_W)
        assert np.isfinite(s).all()
        # fresh skip maps replace the pyramid: the skip entries answer again, with the same bits as before
        ctx.set_skip_maps(cuda_maps(maps))
        again = ctx.det_forward_skip(rois)
        assert np.array_equal(again[0], ok[0]) and np.array_equal(again[1], ok[1])
        _refused(ffi, ffi.AZ_ERR_STATE, ctx.detect_pyramid, boxes, [1.0], S.IM_H, S.IM_W)
    # the 16-bit-term GEMM modes
    for mode in (2, 3):
        with context(Cs[2], ncls=21, gemm_mode=mode, **RED) as (ctx, _):
            _refused(ffi, ffi.AZ_ERR_STATE, ctx.load_skip_front, front)
            assert ctx.skip_dims is None
            _refused(ffi, ffi.AZ_ERR_STATE, ctx.detect_skip, boxes, 1.0, S.IM_H, S.IM_W)
            _refused(ffi, ffi.AZ_ERR_STATE, ctx.det_forward_skip, rois)
            ctx.set_feature_map(maps[2])
            assert np.isfinite(ctx.detect(boxes, 1.0, S.IM_H, S.IM_W)[0]).all()
    # a context limited to fewer regions than a chunk: its capacity is the bound
    with context(Cs[2], ncls=21, max_regions=64, **RED) as (ctx, head):
        ctx.load_skip_front(front)
        ctx.set_skip_maps(cuda_maps(maps))
        _refused(ffi, ffi.AZ_ERR_CAPACITY, ctx.detect_skip, S.random_boxes(65, 29), 1.0, S.IM_H, S.IM_W)
        r = S.random_rois(64, 30)
        p, b = ctx.det_forward_skip(r)
        r64, r32 = S.det_forward(front, head, maps, r, np.float64), S.det_forward(front, head, maps, r, np.float32)
        assert check("64 of 64 regions cls_prob", p, r64[0], r32[0]) and check("64 of 64 regions bbox_pred", b, r64[1], r32[1])


# ---- 7. detect.test and the tools with a skip configuration ---------------------------------------------------------------------
SKIP_YML = os.path.join(REPO, "tests", "golden", "voc_skip.yml")


@pytest.fixture
def skip_cfg(tmp_path):
    """cfg from the skip settings, one test scale that leaves a 96 x 128 image as it is, output under tmp_path; restored
    afterwards."""
    import copy
    from detect import config as C
    saved = copy.deepcopy(dict(C.cfg))
    C.cfg_from_file(SKIP_YML)
    C.cfg.TEST.SCALES, C.cfg.TEST.MAX_SIZE = (S.IM_H,), S.IM_W
    C.cfg_set_mode("Test", 0.0)                       # (as the tools do: SEAR.Tz, SEAR.NUM_PROPOSALS)
    C.cfg.ROOT_DIR = str(tmp_path)
    C.cfg_set_path("skip_test")
    yield C
    S.restore_tree(C.cfg, saved)


def _reduced_nets():
    """A VGG16 of 1/16 width (conv3_3 16, conv4_3 32, conv5_3 32 channels), a detection head and a front to match."""
    from aznet_hip import synth
    from aznet_hip.backbone import VGG16Conv5
    bk = VGG16Conv5(device="cuda:0", seed=5, width_div=16, channels_last_out=True)
    bk.normalize_output(np.ones((1, 3, S.IM_H, S.IM_W), np.float32))
    Cs = (16, 32, 32)
    return bk, Cs, synth.make_det_head(seed=31, C=32, ncls=21, **RED), synth.make_skip_front(seed=32, Cs=Cs, Cout=32)


def _np_maps(conv):
    return [conv[n].detach().cpu().contiguous().numpy() for n in S.NAMES]


def test_test_net_with_a_skip_configuration(skip_cfg, tmp_path, capsys, monkeypatch):
    import pickle
    from aznet_hip.net import HipFrcnnNet
    from datasets.factory import get_imdb
    from detect import test as T
    from oracle import az_oracle as orc
    C = skip_cfg
    bk, Cs, head, front = _reduced_nets()
    imdb = get_imdb("synthetic_%dx%d_2" % (S.IM_H, S.IM_W))
    assert imdb.num_classes == 21
    props = [S.random_boxes(30, 41), S.random_boxes(25, 42)]
    pf = str(tmp_path / "proposals.pkl")
    with open(pf, "wb") as f:
        pickle.dump({"boxes": props, "time": 0.0, "recall": 0}, f)
    # a plain net under the skip configuration never runs
    plain = HipFrcnnNet(head, bk, max_regions=512, name="plain")
    with pytest.raises(ValueError, match="no skip front"):
        T.test_net({"full": plain}, pf, imdb)
    plain.ctx.close()
    net = HipFrcnnNet(head, bk, max_regions=512, name="skip", skip_front=front)
    runs = []
    for nb, debug in ((1, False), (4, True)):
        C.cfg.TEST.BATCH_IMAGES = nb
        (monkeypatch.setenv("AZ_FULL_DEBUG", "1") if debug else monkeypatch.delenv("AZ_FULL_DEBUG", raising=False))
        capsys.readouterr()
        T.test_net({"full": net}, pf, imdb)
        out = capsys.readouterr().out
        assert out.count("image by image") == (1 if debug else 0)
        assert "im_detect: 1/2" in out and "im_detect: 2/2" in out
        with open(os.path.join(C.get_output_dir(imdb, net), "detections.pkl"), "rb") as f:
            runs.append(pickle.load(f))
    dets = runs[0]
    assert len(dets) == 21 and all(len(d) == 2 for d in dets) and dets[0] == [[], []]
    n_det = 0
    for j in range(1, 21):
        for i in range(2):
            assert dets[j][i].ndim == 2 and dets[j][i].shape[1] == 5 and dets[j][i].dtype == np.float32
            assert dets[j][i].shape[0] <= props[i].shape[0]
            assert np.array_equal(dets[j][i], runs[1][j][i])               # BATCH_IMAGES = 4 ran image by image: same bits
            n_det += dets[j][i].shape[0]
    assert n_det > 0
    # one image through im_detect against the restatement on the maps its backbone makes
    im = imdb.image_at(0)
    scores, boxes = T.im_detect({"full": net}, im, props[0], 21)
    blob = net.image_blob_enqueue(im, C.cfg.PIXEL_MEANS, 1.0)
    maps = _np_maps(net.compute_conv(blob))
    assert [m.shape[1:] for m in maps] == [(16, 24, 32), (32, 12, 16), (32, 6, 8)]
    s64, b64 = S.detect(orc, front, head, maps, props[0], 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float64, batch_size=C.cfg.SEAR.BATCH_SIZE)
    s32, _ = S.detect(orc, front, head, maps, props[0], 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float32, batch_size=C.cfg.SEAR.BATCH_SIZE)
    assert check("im_detect scores", scores, s64, s32)
    np.testing.assert_allclose(boxes, b64, rtol=1e-4, atol=1e-4 * S.IM_W)
    net.ctx.close()
    # the tool's own loader on a model file with conv_pool5: the front comes with the head
    import sys
    from aznet_hip import caffemodel as cm
    tools = os.path.join(REPO, "az-net_amd", "tools")
    sys.path[:0] = [tools]
    try:
        import test_det_net
        path = str(tmp_path / "skip16.caffemodel")
        cm.write_caffemodel(path, S.skip_model_layers(seed=7, width_div=16, num_classes=21, **RED))
        fnet = test_det_net.load_frcnn_net(path, 0)
    finally:
        sys.path.remove(tools)
    fhead = cm.det_head_from_layers(cm.load_caffemodel(path))
    assert fnet.skip_names == S.NAMES and fnet.skip_front["Cs"] == (16, 32, 32)
    C.cfg.TEST.BATCH_IMAGES = 1
    T.test_net({"full": fnet}, pf, imdb)
    assert "im_detect: 2/2" in capsys.readouterr().out
    with open(os.path.join(C.get_output_dir(imdb, fnet), "detections.pkl"), "rb") as f:
        fdets = pickle.load(f)
    assert len(fdets) == 21 and sum(fdets[j][i].shape[0] for j in range(1, 21) for i in range(2)) > 0
    scores, boxes = T.im_detect({"full": fnet}, im, props[0], 21)
    maps = _np_maps(fnet.compute_conv(fnet.image_blob_enqueue(im, C.cfg.PIXEL_MEANS, 1.0)))
    kw = dict(batch_size=C.cfg.SEAR.BATCH_SIZE)
    s64, b64 = S.detect(orc, fhead["skip_front"], fhead, maps, props[0], 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float64, **kw)
    s32, _ = S.detect(orc, fhead["skip_front"], fhead, maps, props[0], 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float32, **kw)
    assert check("model file, im_detect scores", scores, s64, s32)
    np.testing.assert_allclose(boxes, b64, rtol=1e-4, atol=1e-4 * S.IM_W)
    fnet.ctx.close()


def test_shared_detection_with_a_skip_configuration(skip_cfg):
    from aznet_hip import synth
    from aznet_hip.net import HipAZNet, HipDetNet
    from datasets.factory import get_imdb
    from detect import test as T
    from oracle import az_oracle as orc
    C = skip_cfg
    bk, Cs, head, front = _reduced_nets()
    az = HipAZNet(synth.make_head(seed=33, C=32, n6=64, n71=32, n72=16), backbone=bk, max_regions=512, gemm_mode=0)
    im = get_imdb("synthetic_%dx%d_2" % (S.IM_H, S.IM_W)).image_at(1)
    # the AZ net alone still hands out conv5_3 only: a skip configuration with a plain detection net is refused
    plain = HipDetNet(head, az, name="plain")
    with pytest.raises(ValueError, match="no skip front"):
        T.im_detect_shared(az, {"fc": plain}, im, 21)
    det = HipDetNet(head, az, name="skip", skip_front=front)
    assert az.taps == ("conv3_3", "conv4_3")
    Y, conv = T.im_propose(az, im, return_conv=True)
    assert list(conv) == list(S.NAMES) and len({id(v) for v in conv.values()}) == 3
    scores, boxes, _ = T._frcnn_forward({"fc": det}, im, Y, 21, conv)
    maps = _np_maps(conv)
    s64, b64 = S.detect(orc, front, head, maps, Y, 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float64, batch_size=C.cfg.SEAR.BATCH_SIZE)
    s32, _ = S.detect(orc, front, head, maps, Y, 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float32, batch_size=C.cfg.SEAR.BATCH_SIZE)
    assert scores.shape == (Y.shape[0], 21) and check("shared scores", scores, s64, s32)
    np.testing.assert_allclose(boxes, b64, rtol=1e-4, atol=1e-4 * S.IM_W)
    # im_detect_shared is the two steps in one; the same image gives the same bits
    s2, b2 = T.im_detect_shared(az, {"fc": det}, im, 21)
    assert np.array_equal(s2, scores) and np.array_equal(b2, boxes)
    # the pycaffe-shaped surface: forward(rois=, conv3_3=, conv4_3=, conv5_3=)
    rois = S.random_rois(9, 43)
    out = det.forward(rois=rois, **conv)
    r64, r32 = S.det_forward(front, head, maps, rois, np.float64), S.det_forward(front, head, maps, rois, np.float32)
    assert check("forward cls_prob", out["cls_prob"], r64[0], r32[0]) and check("forward bbox_pred", out["bbox_pred"], r64[1], r32[1])
    az.ctx.close()


def test_the_tools_synthetic_net_under_a_skip_configuration(skip_cfg, tmp_path, capsys):
    """tools/test_det_net.py's own loader with `--net synthetic:7` (the full-size synthetic VGG16 and head) and the skip
    configuration: test_net attaches the seeded synthetic front and runs the skip detector."""
    import pickle
    import sys
    from aznet_hip import synth
    from datasets.factory import get_imdb
    from detect import test as T
    from oracle import az_oracle as orc
    C = skip_cfg
    tools = os.path.join(REPO, "az-net_amd", "tools")
    sys.path[:0] = [tools]
    try:
        import test_det_net
        net = test_det_net.load_frcnn_net("synthetic:7", 0)
    finally:
        sys.path.remove(tools)
    assert net.skip_front is None and net.name == "vgg16_frcnn_synthetic_7"
    imdb = get_imdb("synthetic_%dx%d_2" % (S.IM_H, S.IM_W))
    props = [S.random_boxes(12, 51), S.random_boxes(0, 52)]
    pf = str(tmp_path / "proposals.pkl")
    with open(pf, "wb") as f:
        pickle.dump({"boxes": props, "time": 0.0, "recall": 0}, f)
    T.test_net({"full": net}, pf, imdb)
    assert "im_detect: 1/2" in capsys.readouterr().out
    front = synth.make_skip_front(seed=9)
    assert net.skip_names == S.NAMES and np.array_equal(net.skip_front["Wp"], front["Wp"])
    with open(os.path.join(C.get_output_dir(imdb, net), "detections.pkl"), "rb") as f:
        dets = pickle.load(f)
    assert len(dets) == 21 and all(dets[j][0].shape[1] == 5 for j in range(1, 21)) and all(dets[j][1] == [] for j in range(1, 21))
    im = imdb.image_at(0)
    scores, boxes = T.im_detect({"full": net}, im, props[0], 21)
    maps = _np_maps(net.compute_conv(net.image_blob_enqueue(im, C.cfg.PIXEL_MEANS, 1.0)))
    assert [m.shape[1] for m in maps] == list(S.FULL_CS)
    head = synth.make_det_head(seed=7, **synth.FULL_DET_DIMS)
    kw = dict(batch_size=C.cfg.SEAR.BATCH_SIZE)
    s64, b64 = S.detect(orc, front, head, maps, props[0], 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float64, **kw)
    s32, _ = S.detect(orc, front, head, maps, props[0], 1.0, im.shape, C.cfg.DEDUP_BOXES, np.float32, **kw)
    assert check("synthetic:7 im_detect scores", scores, s64, s32)
    np.testing.assert_allclose(boxes, b64, rtol=1e-4, atol=1e-4 * S.IM_W)
    net.ctx.close()
