"""GPU: detection inference at its decode, pyramid, NMS and blob edges, against the references of tests/det_infer_ref.py
(each checked against the oracle by tests/test_det_infer_host.py).

  A. az_detect / az_detect_batch on bias-only heads (deltas = bb, logits = bc exactly; dw = dh = 0: expf is 1 and the decode
     a pure f64 expression) and on the integer head: array_equal, except boxes with non-zero log-size deltas (rtol 1e-6 /
     atol 1e-4, the bound of tests/test_gpu_select_edges.py) and non-uniform probabilities (1e-6 from float64).
  B. the pyramid's level choice and key (az_roi_dedup_pyramid) around every switch point, and az_detect_pyramid's rows
     against az_detect on the map of their level: bit for bit.
  C. az_nms_batched / az_nms in every transport (host-mapped, copied back, profiled): the oracle's walk, exactly.
  D. the image front-end at its grid, rounding and clamp edges: oracle.image_blob, bit for bit.
"""
import ctypes

import numpy as np
import pytest

import det_infer_ref as D
import pyramid_ref as pr

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-4          # boxes with non-zero dw / dh (expf against np.exp)
PTOL, SUMTOL = 1e-6, 1e-5        # probabilities against float64, and their sum


@pytest.fixture(scope="module")
def env():
    import torch
    from aznet_hip import ffi, synth
    from oracle import az_oracle as orc
    return torch, ffi, synth, orc


def _context(env, C, fmap=None, **kw):
    """A context with a small AZ head of C channels (a feature map needs one) and, unless given, a random C x 38 x 63 map."""
    torch, ffi, synth, orc = env
    c = ffi.AzContext(0, gemm_mode=0, **kw)
    c.load_head(synth.make_head(seed=1, C=C, n6=8, n71=4, n72=4))
    c.load_det_head(D.clip_head() if C == D.BIAS_DIMS["C"] else synth.make_det_head(seed=2, C=C, n6=8, n7=8, ncls=2))
    c.set_feature_map(fmap if fmap is not None else np.random.RandomState(1).rand(1, C, *D.MAP_HW).astype(np.float32))
    return c


@pytest.fixture(scope="module")
def ctx(env):
    c = _context(env, D.BIAS_DIMS["C"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def cap_ctx(env):
    c = _context(env, D.BIAS_DIMS["C"], max_regions=D.CAP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def int_case(env):
    return D.int_case(env[3])


@pytest.fixture(scope="module")
def int_ctx(env, int_case):
    c = _context(env, 12, fmap=int_case["fmap"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def pyr_ctx(env):
    torch, ffi, synth, orc = env
    c = ffi.AzContext(0, gemm_mode=0)
    c.load_head(synth.make_head(seed=77, **synth.SMALL_DIMS))
    c.load_det_head(synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS))
    yield c
    c.close()


def _detect_equals(c, head, boxes, scale, H, W, eps, dedup=1. / 16., batch=10000, exact=True):
    s, b = c.detect(boxes, scale, H, W, dedup=dedup, batch_size=batch, eps=eps)
    rs, rb, info = D.detect_ref(boxes, scale, dedup, batch, (H, W), eps, D.bias_rows(head))
    assert s.shape == rs.shape and b.shape == rb.shape
    if exact:
        assert np.array_equal(b, rb)
    else:
        assert np.allclose(b, rb, rtol=RTOL, atol=ATOL)
    return s, rs, info


# ---- A. az_detect ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,scale", D.IMAGES)
def test_clip_sides_eps_and_anchor_coordinates_decode_exactly(ctx, H, W, scale):
    head = D.clip_head()
    ctx.load_det_head(head)
    for eps in D.EPS:
        s, rs, _ = _detect_equals(ctx, head, D.clip_anchors(H, W), scale, H, W, eps)
        assert np.array_equal(s, rs)
        assert np.array_equal(s, np.full(s.shape, np.float32(1) / np.float32(len(D.CLIP_SHIFTS))))    # uniform logits


@pytest.mark.parametrize("ncls", D.CLASS_COUNTS)
def test_every_class_column_shows_its_own_deltas(ctx, ncls):
    for H, W, scale in D.IMAGES:
        for log_sizes in (False, True):
            head = D.class_head(ncls, log_sizes)
            ctx.load_det_head(head)
            s, rs, _ = _detect_equals(ctx, head, D.class_anchors(H, W), scale, H, W, 1e-14, exact=not log_sizes)
            p64 = np.exp(head["bc"].astype(np.float64) - head["bc"].max())
            assert np.isfinite(s).all() and np.abs(s - p64 / p64.sum()).max() <= PTOL
            assert np.abs(s.astype(np.float64).sum(1) - 1).max() <= SUMTOL
        uni = D.bias_head(ncls, head["bb"])
        ctx.load_det_head(uni)
        s, _ = ctx.detect(D.class_anchors(H, W), scale, H, W)
        assert np.array_equal(s, np.full(s.shape, np.float32(1) / np.float32(ncls)))


@pytest.mark.parametrize("ncls", [2, 21, 65, 256])
def test_extreme_logits_stay_finite_and_normalised(ctx, ncls):
    H, W, scale = D.IMAGES[0]
    hot = np.zeros(ncls, np.float32)
    hot[ncls // 3] = 100.0
    for bc in (hot, np.full(ncls, -100.0, np.float32), -hot):
        ctx.load_det_head(D.bias_head(ncls, np.zeros(4 * ncls), bc))
        s, _ = ctx.detect(D.class_anchors(H, W), scale, H, W)
        p64 = np.exp(bc.astype(np.float64) - bc.max())
        assert np.isfinite(s).all()
        assert np.abs(s.astype(np.float64).sum(1) - 1).max() <= SUMTOL
        assert np.abs(s - p64 / p64.sum()).max() <= PTOL


@pytest.mark.parametrize("batch", D.BATCHES)
def test_chunks_give_every_row_its_own_answer(cap_ctx, batch):
    H, W, scale = D.IMAGES[0]
    head = D.bias_head(21, D.class_head(21)["bb"])                 # distinct deltas, uniform logits: scores exact too
    cap_ctx.load_det_head(head)
    for P in D.chunk_sizes(batch):
        boxes = D.chunk_boxes(P, H, W, scale)
        s, rs, info = _detect_equals(cap_ctx, head, boxes, scale, H, W, 1e-14, batch=batch)
        assert np.array_equal(s, rs)
        rois, index, inv = cap_ctx.roi_dedup(boxes, scale, batch_size=batch)
        assert len(index) == len(info["index"]), (P, batch)
        assert np.array_equal(index, info["index"]) and np.array_equal(inv, info["inv"]) and np.array_equal(rois, info["rois"])


def test_dedup_factor_zero_negative_and_one(ctx):
    H, W, scale = D.IMAGES[0]
    head = D.class_head(21)
    ctx.load_det_head(head)
    boxes = D.chunk_boxes(40, H, W, scale)
    for dd in (0.0, -1.0):                                        # identity: duplicates are not merged, answers the same
        _detect_equals(ctx, head, boxes, scale, H, W, 1e-14, dedup=dd, batch=7)
        rois, index, inv = ctx.roi_dedup(boxes, scale, dedup=dd, batch_size=7)
        assert np.array_equal(index, np.arange(40)) and np.array_equal(inv, np.arange(40))
    _, _, merged = _detect_equals(ctx, head, boxes, scale, H, W, 1e-14, batch=7)
    assert len(merged["index"]) < 40
    boxes = D.overflow_boxes()                                    # dedup 1: hash fields overlap, keys below zero
    for batch in (10000, 5):
        _, _, info = _detect_equals(ctx, head, boxes, 1.0, 1300, 2600, 1e-14, dedup=1.0, batch=batch)
        rois, index, inv = ctx.roi_dedup(boxes, 1.0, dedup=1.0, batch_size=batch)
        assert np.array_equal(index, info["index"]) and np.array_equal(inv, info["inv"])
    assert inv[0] == inv[1] and inv[6] == inv[7]


def test_capacity_and_emptiness_leave_the_outputs_alone(env, cap_ctx):
    torch, ffi, synth, orc = env
    H, W, scale = D.IMAGES[0]
    head = D.class_head(21)
    cap_ctx.load_det_head(head)
    boxes = np.ascontiguousarray(D.chunk_boxes(D.CAP + 1, H, W, scale))
    s = np.full((D.CAP + 1, 21), -7.0, np.float32)
    b = np.full((D.CAP + 1, 84), -7.0, np.float64)
    call = lambda P: cap_ctx.L.az_detect(cap_ctx.h, ffi._p(boxes, ctypes.c_double), P, scale, 1. / 16., 10000, H, W, 1e-14,   # noqa: E731
                                         ffi._p(s, ctypes.c_float), ffi._p(b, ctypes.c_double))
    assert call(D.CAP + 1) == ffi.AZ_ERR_CAPACITY
    assert np.all(s == -7.0) and np.all(b == -7.0)
    assert call(0) == ffi.AZ_OK
    assert np.all(s == -7.0) and np.all(b == -7.0)
    with pytest.raises(ffi.AzError):
        cap_ctx.roi_dedup(boxes, scale)
    _detect_equals(cap_ctx, head, boxes[:D.CAP], scale, H, W, 1e-14)         # the context works afterwards


def test_batched_entry_clips_every_row_to_its_own_image(env, ctx):
    torch, ffi, synth, orc = env
    head = D.clip_head()
    ctx.load_det_head(head)
    images = ((375, 500, 1.6), (16, 16, 16.0), (120, 90, 4.0))
    C = D.BIAS_DIMS["C"]
    maps = [torch.rand(1, C, h, w, device="cuda") for h, w in ((38, 63), (16, 16), (30, 23))]
    boxes = [D.clip_anchors(H, W) for H, W, _ in images]
    got = ctx.detect_batch(maps, boxes, [sc for _, _, sc in images], [(H, W) for H, W, _ in images], eps=0.0)
    for (H, W, sc), bx, (s, b) in zip(images, boxes, got):
        rs, rb, _ = D.detect_ref(bx, sc, 1. / 16., 10000, (H, W), 0.0, D.bias_rows(head))
        assert np.array_equal(b, rb) and np.array_equal(s, rs)
    ctx.set_feature_map(np.random.RandomState(1).rand(1, C, *D.MAP_HW).astype(np.float32))


def test_integer_head_deltas_are_exact_through_the_decode(int_ctx, int_case):
    case = int_case
    boxes = case["boxes"]
    rois = np.hstack([np.zeros((len(boxes), 1)), boxes]).astype(np.float32)
    for head, deltas, exact in ((case["zero_sizes"], case["zero_deltas"], True), (case["head"], case["deltas"], False)):
        int_ctx.load_det_head(head)
        p, d = int_ctx.det_forward(rois)
        assert np.array_equal(d, deltas)                          # dx, dy (and dw, dh): multiples of 2^-k, exactly
        assert np.abs(p - case["p64"]).max() <= PTOL
        fn = lambda index, rois_u: (p[index], deltas[index])      # noqa: E731
        for H, W in (case["im"], (16, 16)):
            s, b = int_ctx.detect(boxes, 1.0, H, W, batch_size=64)
            rs, rb, info = D.detect_ref(boxes, 1.0, 1. / 16., 64, (H, W), 1e-14, fn)
            assert np.array_equal(s, rs)
            if exact:
                assert np.array_equal(b, rb)
            else:
                assert np.allclose(b, rb, rtol=RTOL, atol=ATOL)


# ---- B. the pyramid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.SCALE_SETS))
def test_level_choice_around_every_switch_point(ctx, name):
    scales = D.SCALE_SETS[name]
    boxes = np.concatenate([D.switch_boxes(scales), D.spread_boxes(), D.degenerate_boxes()[:3]])
    for dedup in (1. / 16., 1.0):
        rois, index, inv = ctx.roi_dedup_pyramid(boxes, scales, dedup=dedup)
        r, i, v = D.unique_rows(boxes, scales, dedup, 10000)
        assert np.array_equal(rois[:, 0], r[:, 0])                # the level NumPy's argmin takes
        assert np.array_equal(rois, r) and np.array_equal(index, i) and np.array_equal(inv, v)


def test_infinite_and_nan_areas_take_level_zero(ctx):
    boxes = D.degenerate_boxes()
    for name in ("three", "descending", "unsorted", "eight"):
        scales = D.SCALE_SETS[name]
        rois, index, inv = ctx.roi_dedup_pyramid(boxes, scales, dedup=0.0)
        with np.errstate(all="ignore"):
            r, i, v = D.unique_rows(boxes, scales, 0.0, 10000)
        assert np.array_equal(rois, r, equal_nan=True) and np.array_equal(index, i) and np.array_equal(inv, v)
        assert np.all(rois[3:, 0] == 0)


@pytest.mark.parametrize("batch", D.BATCHES)
def test_pyramid_dedup_merges_levels_at_a_sixteenth_only(cap_ctx, batch):
    scales = [1.0, 2.0]
    pool = np.concatenate([D.merge_pair(), D.spread_boxes(12, seed=9), D.merge_pair()[::-1]])
    for P in D.chunk_sizes(batch):
        boxes = pool[np.arange(P) % len(pool)]
        for dedup in (1. / 16., 1.0, 0.0):
            rois, index, inv = cap_ctx.roi_dedup_pyramid(boxes, scales, dedup=dedup, batch_size=batch)
            r, i, v = D.unique_rows(boxes, scales, dedup, batch)
            assert np.array_equal(rois, r) and np.array_equal(index, i) and np.array_equal(inv, v), (P, dedup)
    if batch >= 4:
        four = D.merge_pair()
        assert len(cap_ctx.roi_dedup_pyramid(four, scales, dedup=1. / 16., batch_size=batch)[1]) == 2
        assert len(cap_ctx.roi_dedup_pyramid(four, scales, dedup=1.0, batch_size=batch)[1]) == 4


def test_pyramid_rows_are_az_detects_on_the_map_of_their_level(env, pyr_ctx):
    torch, ffi, synth, orc = env
    H, W = 300, 400
    scales = np.array(D.SCALE_SETS["three"])
    _, _, bh, bw = pr.blob_shape((H, W), scales)
    mh, mw = synth.conv_out_size(bh), synth.conv_out_size(bw)
    assert mh <= D.MAP_HW[0] and mw <= D.MAP_HW[1]
    C = synth.SMALL_DET_DIMS["C"]
    maps = [synth.make_feature_map(60 + k, C, mh, mw).astype(np.float32) for k in range(3)]
    dev = [torch.from_numpy(m.reshape(1, C, mh, mw)).cuda().contiguous(memory_format=torch.channels_last) for m in maps]
    rng = np.random.RandomState(21)
    sets = []
    for k in range(3):
        n = 48
        side = 224.0 / scales[k] * rng.uniform(0.96, 1.04, n)
        x1, y1 = rng.uniform(-30, W - 60, n), rng.uniform(-30, H - 60, n)       # past the border on every side
        b = np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.97, 1.03, n)], 1)
        b[40:] = b[:8] + 0.25                                                    # merged at 1/16
        assert np.all(pr.rois_blob(b, scales)[:, 0] == k)
        sets.append(b)
    pyr_ctx.set_feature_pyramid(dev)
    got = [pyr_ctx.detect_pyramid(b, scales, H, W, batch_size=32) for b in sets]
    for k in range(3):
        pyr_ctx.set_feature_map(maps[k].reshape(1, C, mh, mw))
        s, b = pyr_ctx.detect(sets[k], scales[k], H, W, batch_size=32)
        assert np.array_equal(got[k][0], s) and np.array_equal(got[k][1], b), k
    assert not np.array_equal(got[0][0][:8], got[1][0][:8])


# ---- C. NMS ---------------------------------------------------------------------------------------------------------------
def _keeps(orc, groups, thresh):
    return [D.reference_keep(orc, g, thresh) for g in groups]


@pytest.mark.parametrize("name", sorted(D.NMS_TABLE))
def test_nms_batched_in_every_transport(env, ctx, name):
    torch, ffi, synth, orc = env
    sizes, seed = D.NMS_TABLE[name]
    groups = D.nms_groups(sizes, seed)
    for thresh in (0.5, 0.3):
        ref = _keeps(orc, groups, thresh)
        got = ctx.nms_batched(groups, thresh)
        assert [list(k) for k in got] == ref, (name, thresh, "unprofiled")
        try:
            ctx.set_profiling(2)
            prof = ctx.nms_batched(groups, thresh)
        finally:
            ctx.set_profiling(0)
        assert [list(k) for k in prof] == ref, (name, thresh, "profiled")


@pytest.mark.parametrize("n", [1, 100, 256, 257, 1025])
def test_nms_profiled_equals_unprofiled(env, ctx, n):
    torch, ffi, synth, orc = env
    rng = np.random.RandomState(n)
    for kind in range(5):
        dets = D.nms_case(rng, n, kind)
        ref = D.reference_keep(orc, dets, 0.5)
        assert list(ctx.nms(dets, 0.5)) == ref
        try:
            ctx.set_profiling(2)
            prof = list(ctx.nms(dets, 0.5))
        finally:
            ctx.set_profiling(0)
        assert prof == ref


def test_nms_results_do_not_go_stale(env, ctx):
    torch, ffi, synth, orc = env
    large = D.nms_groups([256, 100, ("none", 256), 64, 7, ("first", 256)], 31)
    small = D.nms_groups([256, 100, ("first", 256), 64], 32)          # the same offsets, other boxes, fewer groups
    for groups in (large, small, large):
        assert [list(k) for k in ctx.nms_batched(groups, 0.5)] == _keeps(orc, groups, 0.5)
    rng = np.random.RandomState(33)
    for it in range(30):
        sizes = [int(v) for v in rng.choice([0, 1, 2, 63, 64, 65, 255, 256], size=int(rng.randint(1, 12)))]
        groups = D.nms_groups(sizes, 100 + it)
        thresh = float(rng.choice([0.0, 0.3, 0.5, 1.0]))
        assert [list(k) for k in ctx.nms_batched(groups, thresh)] == _keeps(orc, groups, thresh), it
        dets = D.nms_case(rng, int(rng.choice([1, 17, 256, 300])), it % 5)
        assert list(ctx.nms(dets, thresh)) == D.reference_keep(orc, dets, thresh), it


def test_apply_nms_with_empty_classes_and_an_image_without_detections(env):
    torch, ffi, synth, orc = env
    import detect.test as dtest
    rng = np.random.RandomState(41)
    ncls, nim = 5, 3
    all_boxes = [[[] for _ in range(nim)] for _ in range(ncls)]
    for c in range(1, ncls):
        for i in range(nim):
            if i == 1 or c == 3:                                      # image 1 has no detections, class 3 none anywhere
                continue
            d = D.nms_case(rng, int(rng.choice([1, 30, 100])), (c + i) % 5)
            d[:, 4] = rng.permutation(len(d)) / float(len(d))         # distinct scores: the reference's own order
            all_boxes[c][i] = d
    all_boxes[2][2] = np.zeros((0, 5), np.float32)
    got, ref = dtest.apply_nms(all_boxes, 0.3), orc.apply_nms(all_boxes, 0.3)
    for c in range(ncls):
        for i in range(nim):
            assert np.array_equal(np.asarray(got[c][i]), np.asarray(ref[c][i])), (c, i)
    assert all(len(got[c][1]) == 0 for c in range(ncls)) and len(got[1][0]) > 0


# ---- D. the image front-end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,scale,what", D.BLOB_CASES)
def test_image_blob_at_its_grid_rounding_and_clamp_edges(env, ctx, h, w, scale, what):
    torch, ffi, synth, orc = env
    assert ctx.image_blob_size(h, w, scale) == orc.image_blob_size(h, w, scale)
    for kind in ("random", "zeros", "full", "checker"):
        im = D.blob_image(h, w, kind)
        got = ctx.image_blob(im, D.MEANS, scale)
        assert np.array_equal(got, orc.image_blob(im, D.MEANS, scale)), (what, kind)
        if scale == 1.0:
            assert np.array_equal(got[0], (im.astype(np.float32) - D.MEANS).transpose(2, 0, 1))


def test_image_blob_on_a_stream_equals_the_synchronous_form(env, ctx):
    torch, ffi, synth, orc = env
    st = torch.cuda.Stream()
    outs = []
    for h, w, scale in ((20, 30, 1.7), (90, 130, 0.6), (11, 14, 2.0)):          # the upload slots grow, then are reused
        im = D.blob_image(h, w, "random", seed=5)
        oh, ow = ctx.image_blob_size(h, w, scale)
        out = torch.zeros(1, 3, oh, ow, device="cuda")
        torch.cuda.synchronize()
        ctx.image_blob(im, D.MEANS, scale, out=out, stream=st.cuda_stream)
        outs.append((im, scale, out))
    st.synchronize()
    for im, scale, out in outs:
        ref = ctx.image_blob(im, D.MEANS, scale)
        assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ref, orc.image_blob(im, D.MEANS, scale))
        sync = torch.zeros_like(out)
        ctx.image_blob(im, D.MEANS, scale, out=sync)
        assert np.array_equal(sync.cpu().numpy(), ref)


def test_image_blob_refuses_a_wrong_size_and_a_bad_scale(env, ctx):
    torch, ffi, synth, orc = env
    im = D.blob_image(10, 12, "random")
    blob = np.full((3, 40, 40), -7.0, np.float32)
    call = lambda scale, oh, ow: ctx.L.az_image_blob_host(ctx.h, ffi._p(im, ctypes.c_uint8), 10, 12, ffi._p(D.MEANS, ctypes.c_float),   # noqa: E731
                                                          float(scale), ffi._p(blob, ctypes.c_float), oh, ow)
    for scale, oh, ow in ((1.5, 15, 17), (1.5, 14, 18), (1.5, 16, 18), (0.0, 1, 1), (-1.0, 10, 12), (float("nan"), 10, 12),
                          (0.01, 0, 0)):
        assert call(scale, oh, ow) == ffi.AZ_ERR_INVALID, (scale, oh, ow)
    assert np.all(blob == -7.0)
    assert call(1.5, 15, 18) == ffi.AZ_OK
    assert np.array_equal(blob.ravel()[:3 * 15 * 18].reshape(1, 3, 15, 18), orc.image_blob(im, D.MEANS, 1.5))
