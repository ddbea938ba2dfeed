"""GPU: the detection family -- az_det_forward*, az_detect, az_detect_skip, az_detect_pyramid, az_detect_batch, az_detect_iter*
and the nets over them -- as one pass enqueued in several forms (DetPass and det_pass_enqueue, az_detect.hip; _DetNet.run,
aznet_hip/net.py).  Three things that hold whichever way the forms share their code:
  a. the launch sequence of every entry, as az_last_kernel_times names it under profiling mode 2 (the lists are written out
     here: bench.py and the perf scripts key on these names; only the batch pass times its dedup);
  b. the identities between entries that the code documents, on raw bytes;
  c. the code and text of what the entries refuse on the host, before any launch.
Only public AzContext / net methods are used.  Sizes: the smallest at which each fork is taken -- 48 boxes of which five are
exact duplicates (fewer unique rows than boxes: the un-dedup gather does real work), a batch of 40, 0 and 40 boxes on a
context of 64 regions (two passes, one empty image), the skip front at its smallest sources (one chunk)."""
import numpy as np
import pytest

import skip_ref as S

pytestmark = pytest.mark.gpu

IM = (600, 1000)                 # scale 1: a 38 x 63 map
HEAD = ["det_fc6_gemm", "det_fc6_reduce", "det_fc7_gemm", "det_fc7_reduce", "det_tail_gemm", "det_epilogue"]
PLAIN = ["det_roi_pool"] + HEAD
SKIP = ["skip_pool_norm_0", "skip_pool_norm_1", "skip_pool_norm_2", "skip_conv_gemm"] + HEAD
BATCH_PASS = ["det_rois_dedup"] + PLAIN


def iter_rounds(first, taken):
    """rounds = 3: round 1, then select + pass + take for each of the `taken` later rounds that found sources; the select
    of a round that found none ends the loop."""
    return first + taken * (["iter_select"] + first + ["iter_take"]) + (["iter_select"] if taken < 2 else [])


def boxes_in(h, w, n, seed):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(0, 0.6 * w, n), rng.uniform(0, 0.6 * h, n)
    b = np.round(np.stack([x1, y1, x1 + rng.uniform(0.1 * w, 0.4 * w, n), y1 + rng.uniform(0.1 * h, 0.4 * h, n)], 1), 1)
    b[-5:] = b[:5]                                                  # exact duplicates
    return b


def rois_of(boxes):
    return np.concatenate([np.zeros((boxes.shape[0], 1)), boxes], 1).astype(np.float32)


@pytest.fixture(scope="module")
def world():
    import torch
    from aznet_hip import ffi, synth

    class World(object):
        pass

    w = World()
    w.torch, w.ffi = torch, ffi
    w.C = synth.SMALL_DET_DIMS["C"]
    w.az = synth.make_head(seed=77, **synth.SMALL_DIMS)
    w.det = synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)
    w.fmap = synth.make_feature_map(11, w.C, 38, 63)
    w.fmap2 = synth.make_feature_map(12, w.C, 38, 63)
    w.boxes = boxes_in(IM[0], IM[1], 48, 5)
    w.front = synth.make_skip_front(seed=1, Cs=S.SMALL_CS, Cout=w.C, scales=S.SCALES)
    w.skip_maps = S.make_maps(11, S.SMALL_CS)
    w.skip_boxes = boxes_in(S.IM_H, S.IM_W, 48, 6)
    return w


def cuda_cl(w, m):
    return w.torch.from_numpy(m).cuda().contiguous(memory_format=w.torch.channels_last)


@pytest.fixture(scope="module")
def ctx(world):
    c = world.ffi.AzContext(0, max_regions=512, gemm_mode=0)
    c.load_head(world.az)                         # (set_feature_map takes the map's channel count from the AZ head)
    c.load_det_head(world.det)
    c.set_feature_map(world.fmap)
    yield c
    c.close()


@pytest.fixture(scope="module")
def skip_ctx(world):
    c = world.ffi.AzContext(0, max_regions=512, gemm_mode=0)
    c.load_det_head(world.det)
    c.load_skip_front(world.front)
    c.set_skip_maps([world.torch.from_numpy(m).cuda() for m in world.skip_maps])
    yield c
    c.close()


def stages(c, fn, *a, **kw):
    c.set_profiling(2)
    try:
        fn(*a, **kw)
        names = [n for n, _, _ in c.last_kernel_times()]
    finally:
        c.set_profiling(0)
    print(names)
    return names


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def eighth(scores):
    """The 8th largest non-background score: a threshold that leaves round 2 its 8 rows."""
    return float(np.sort(scores[:, 1:].ravel())[::-1][7])


# ---- a. launch sequences ------------------------------------------------------------------------------------------------------
def test_launch_sequence_of_the_head_alone(world, ctx, skip_ctx):
    assert stages(ctx, ctx.det_forward, rois_of(world.boxes)) == PLAIN
    assert stages(skip_ctx, skip_ctx.det_forward_skip, rois_of(world.skip_boxes)) == SKIP


def test_launch_sequence_of_one_image(world, ctx, skip_ctx):
    assert stages(ctx, ctx.detect, world.boxes, 1.0, *IM) == PLAIN
    assert stages(skip_ctx, skip_ctx.detect_skip, world.skip_boxes, 1.0, S.IM_H, S.IM_W) == SKIP


def test_launch_sequence_over_a_pyramid(world):
    c = world.ffi.AzContext(0, max_regions=512, gemm_mode=0)
    try:
        c.load_det_head(world.det)
        c.set_feature_pyramid([cuda_cl(world, world.fmap), cuda_cl(world, world.fmap2)])
        assert stages(c, c.detect_pyramid, world.boxes, [1.0, 0.5], *IM) == PLAIN
    finally:
        c.close()


def test_launch_sequence_of_a_batch_in_two_passes(world):
    c = world.ffi.AzContext(0, max_regions=64, gemm_mode=0)
    try:
        c.load_det_head(world.det)
        maps = [cuda_cl(world, world.fmap), None, cuda_cl(world, world.fmap2)]
        sets = [world.boxes[:40], np.zeros((0, 4)), world.boxes[8:]]
        names = stages(c, c.detect_batch, maps, sets, [1.0] * 3, [IM] * 3)
        assert names == 2 * BATCH_PASS                # (the profile keeps both passes)
        outs = c.detect_batch(maps, sets, [1.0] * 3, [IM] * 3)
        assert [o[0].shape[0] for o in outs] == [40, 0, 40]
    finally:
        c.close()


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
def test_launch_sequence_of_three_rounds(world, ctx, skip_ctx, skip):
    c, boxes, hw = (skip_ctx, world.skip_boxes, (S.IM_H, S.IM_W)) if skip else (ctx, world.boxes, IM)
    s1 = (c.detect_skip if skip else c.detect)(boxes, 1.0, *hw)[0]
    names = stages(c, c.detect_iter, boxes, 1.0, hw[0], hw[1], 3, eighth(s1), 8, skip=skip)
    # (on the plain map round 2's rows pass the threshold again; on the skip maps none of them does: round 3's select finds
    #  no sources there and the loop ends -- both ways through the loop are pinned)
    assert names == (iter_rounds(SKIP, 1) if skip else iter_rounds(PLAIN, 2))


# ---- b. identities between entries, on raw bytes ----------------------------------------------------------------------------
def test_a_batch_of_one_image_is_detect(world, ctx):
    want = ctx.detect(world.boxes, 1.0, *IM)
    got = ctx.detect_batch([cuda_cl(world, world.fmap)], [world.boxes], [1.0], [IM])[0]
    assert same(got, want) and np.unique(want[0], axis=0).shape[0] > 8


def test_one_round_is_detect(world, ctx, skip_ctx):
    s, b, ex = ctx.detect_iter(world.boxes, 1.0, IM[0], IM[1], 1, 0.0, 8)
    assert same((s, b), ctx.detect(world.boxes, 1.0, *IM)) and ex["count"].size == 0
    s, b, ex = skip_ctx.detect_iter(world.skip_boxes, 1.0, S.IM_H, S.IM_W, 1, 0.0, 8, skip=True)
    assert same((s, b), skip_ctx.detect_skip(world.skip_boxes, 1.0, S.IM_H, S.IM_W)) and ex["count"].size == 0


def test_both_nets_and_both_routes_of_frcnn_forward(world):
    from aznet_hip.net import HipAZNet, HipDetNet, HipFrcnnNet
    from detect import test as T
    from detect.config import cfg
    az = HipAZNet(world.az, name="det_family_az", max_regions=512, gemm_mode=0)
    fr = HipFrcnnNet(world.det, None, name="det_family_full", max_regions=512)
    try:
        az.set_conv(world.fmap)
        det = HipDetNet(world.det, az, name="det_family_fc")
        args = (cfg.DEDUP_BOXES, cfg.SEAR.BATCH_SIZE, cfg.EPS)
        want = det.detect(world.boxes, 1.0, IM, *args)
        assert same(fr.detect(cuda_cl(world, world.fmap), world.boxes, 1.0, IM + (3,), *args), want)
        im = np.zeros(IM + (3,), dtype=np.uint8)
        fwd = T._frcnn_forward(det, im, world.boxes, det.num_classes, refine=None)
        assert len(fwd) == 3 and same(fwd[:2], T.im_detect(det, im, world.boxes, det.num_classes))
        assert fwd[0].dtype == np.float64 and fwd[0].shape == (48, det.num_classes)
    finally:
        az.ctx.close()
        fr.ctx.close()


# ---- c. refusals: code and text ---------------------------------------------------------------------------------------------
def refused(world, want, fn, *a, **kw):
    with pytest.raises(world.ffi.AzError) as e:
        fn(*a, **kw)
    assert str(e.value) == want


def test_refusals_keep_their_code_and_text(world, ctx):
    b = world.boxes
    assert (world.ffi.AZ_ERR_INVALID, world.ffi.AZ_ERR_CAPACITY, world.ffi.AZ_ERR_STATE) == (-1, -3, -4)
    refused(world, "AZ_ERR_INVALID (-1): az_detect: bad arguments", ctx.detect, b, 0.0, *IM)
    refused(world, "AZ_ERR_STATE (-4): az_detect_pyramid: no pyramid of that many maps set (az_set_feature_pyramid_dev_nhwc)",
            ctx.detect_pyramid, b, [1.0, 0.5], *IM)
    refused(world, "AZ_ERR_INVALID (-1): az_detect_iter: 1 <= rounds <= AZ_ITER_LOC_MAX_ROUNDS",
            ctx.detect_iter, b, 1.0, IM[0], IM[1], 9, 0.0, 8)
    refused(world, "AZ_ERR_STATE (-4): az_detect_skip: az_load_skip_front has not been called", ctx.detect_skip, b, 1.0, *IM)
    refused(world, "AZ_ERR_CAPACITY (-3): az_detect: too many boxes", ctx.detect, boxes_in(IM[0], IM[1], 513, 7), 1.0, *IM)
    # (nothing was launched, nothing is left behind: the context still detects)
    assert ctx.detect(b, 1.0, *IM)[0].shape == (48, 21)
