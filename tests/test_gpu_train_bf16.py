"""GPU: bf16-operand training (AZ_TRAIN_BF16: k_solver_gemm_bf16 behind az_solver_*, az_det_solver_* and the skip front)
against tests/bf16_ref.py, the float64 restatement of the SAME model: both operands of every matrix product rounded to
bfloat16 (nearest, ties to even), the products summed exactly.  The fp32 model is a different model (2e-3 .. 3e-3 away:
tests/test_bf16_host.py) and is never the yardstick here.

Tolerances.  Products of two bf16 values are exact in float32, so integer cases (every partial sum below 2^24, asserted on
the CPU in test_bf16_host.py) are bit for bit, whatever the order inside the instruction.  Everything else: per tensor
max|got - ref64| / max|ref64| at most 8 x the same quantity of the float32 CPU restatement of the bf16 model, floor 1e-6
(train_step_ref.bound), the project's standing bound.  In the one-step tests no ReLU gate may differ from the float64
model's (the seeds are those at which float32's do not: test_bf16_host.py).  Every figure is printed before it is asserted.

`accumulate`: az_solver_gemm_unit_prec has no such argument, so the kernel's own flag (one slab: bbox_pred_dx of `small`,
K = 8) and the slab sum onto a non-zero D (bbox_pred_dx of `voc` / `coco`, adj_bbox_dx and int7_2_dx of the AZ cases) are
covered by the step tests, through d_pre7 / d_pre71 / d_pre6."""
import os

import numpy as np
import pytest

import bf16_ref as B
import det_step_ref as D
import det_train_ref as DR
import skip_ref as S
import skip_train_ref as T
import train_step_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g21_train_det.npz")
FP32, BF16 = 0, 1
AZ_LAYERS = ((6, 0, "b6"), (71, 1, "b71"), (72, 2, "b72"))


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def check(name, got, r64, r32, rows=None):
    e_dev, e_cpu = B.rel_err(got, r64), B.rel_err(r32, r64)
    b = B.bound(e_cpu)
    print("  %-16s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (name, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    if rows is not None:
        rows.append((name, e_dev, e_cpu, b))
    return e_dev <= b


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def exceeding(rows):
    return "a tensor exceeds 8 x the float32-CPU error: " + ", ".join(r[0] for r in rows if r[1] > r[3])


# ---- 1. GEMM unit, integer operands: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", B.INT_MN)
def test_gemm_integer_exact(ctx, M, N):
    from aznet_hip import ffi
    for form in (0, 1, 2):
        for K in B.INT_K:
            rng = np.random.Generator(np.random.PCG64(1000 * form + K))
            a, b, want = B.gemm_operands(form, M, N, K, B.integer_draw(rng))
            got = ffi.gemm_unit(ctx, form, a, b, precision=BF16)
            assert got.shape == want.shape and same_bits(got, want.astype(np.float32)), (form, M, N, K)


def test_gemm_integer_exact_past_256_tiles(ctx):
    from aznet_hip import ffi
    M, N, K = B.INT_BIG
    for form in (0, 1):
        a, b, want = B.gemm_operands(form, M, N, K, B.integer_draw(np.random.Generator(np.random.PCG64(form))))
        assert same_bits(ffi.gemm_unit(ctx, form, a, b, precision=BF16), want.astype(np.float32)), form


# ---- 2. GEMM unit, rounding: what a truncating or an fp32 kernel fails -----------------------------------------------------------
@pytest.mark.parametrize("kind", ["ties", "mixed"])
def test_gemm_rounds_to_nearest_even(ctx, kind):
    from aznet_hip import ffi
    for M, N, K in B.ROUND_SHAPES:
        for form in (0, 1, 2):
            rng = np.random.Generator(np.random.PCG64(7 * form + K))
            a, b, exact = B.gemm_operands(form, M, N, K, (B.tie_draw if kind == "ties" else B.mixed_draw)(rng))
            want = B.rounded_product(form, a, b).astype(np.float32)
            got = ffi.gemm_unit(ctx, form, a, b, precision=BF16)
            fp = ffi.gemm_unit(ctx, form, a, b, precision=FP32)
            assert same_bits(fp, exact.astype(np.float32)), "fp32 mode is exact on these operands"
            assert same_bits(got, want), (kind, form, M, N, K)
            assert not np.array_equal(got, fp), "bf16 mode gave the fp32 product"


# ---- 3. GEMM unit, random operands ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", B.RANDOM_SHAPES)
def test_gemm_random_within_the_standing_bound(ctx, M, N, K):
    from aznet_hip import ffi
    rows = []
    for form in (0, 1, 2):
        rng = np.random.Generator(np.random.PCG64(100 * form + M))
        a, b, _ = B.gemm_operands(form, M, N, K, B.normal_draw(rng))
        r64, r32 = B.rounded_product(form, a, b), B.rounded_product(form, a, b, np.float32)
        check("form %d %dx%dx%d" % (form, M, N, K), ffi.gemm_unit(ctx, form, a, b, precision=BF16), r64, r32, rows)
    assert all(r[1] <= r[3] for r in rows), exceeding(rows)


# ---- 4. steps in bf16 mode ---------------------------------------------------------------------------------------------------------
def make_det(ctx, head, max_rois=256, seed=1, prec=BF16):
    from aznet_hip import ffi
    n6, n7, ncls = head["W6"].shape[0], head["W7"].shape[0], head["Wc"].shape[0]
    sol = ffi.AzDetSolver(ctx, head["W6"].shape[1] // 49, n6, n7, ncls, max_rois=max_rois, seed=seed, head=head)
    if prec is not None:
        sol.set_precision(prec)
    return sol


def det_args(conv, blobs):
    return (conv, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"])


def az_args(conv, blobs):
    return (conv, blobs["rois"], blobs["adj_labels"], blobs["adj_targets"], blobs["adj_loss_weights"], blobs["zoom_labels"])


def fetched_masks(sol, seed, it, layers):
    from aznet_hip import ffi
    masks = {}
    for t, l, _ in layers:
        m = sol.fetch("mask%d" % t)
        assert np.array_equal(m, ffi.dropout_mask(seed, it, l, m.size, ratio=0.5).reshape(m.shape)), "mask of layer %d" % t
        masks[t] = m
    return masks


def assert_gates_equal(sol, r64, tags):
    for t in tags:
        diff = (sol.fetch("pre%d" % t) > 0) != r64["gates"][t]
        print("  gates of layer %d: %d of %d differ from the float64 bf16 model" % (t, int(diff.sum()), diff.size))
        assert not diff.any(), "a ReLU gate of layer %d differs from the float64 bf16 model" % t


def relu_dropout_exact(sol, masks, layers):
    for t, _, _ in layers:
        pre, a, dp = sol.fetch("pre%d" % t), sol.fetch("a%d" % t), sol.fetch("d_pre%d" % t)
        relu = np.maximum(pre, np.float32(0))
        assert same_bits(a, np.where(masks[t] > 0, relu * np.float32(2), np.float32(0)).astype(np.float32)), "a%d" % t
        assert not dp[(pre <= 0) | (masks[t] == 0)].any()


def two_updates(sol, keys, start, r64, r32, sumsq, sgd, rows):
    """A clipped update, then an unclipped one on top of its history: weights and history against both restatements."""
    rate, mom, wd = 0.001, 0.9, 0.0005
    zeros = {k: np.zeros_like(v) for k, v in start.items()}
    ok = True
    for rep, clip_at in ((0, 1e-3), (1, None)):
        cs = R.clip_scale(sumsq, clip_at)
        if rep == 0:
            assert cs < 1.0
            p64, h64 = sgd(start, r64["grads"], zeros, rate, mom, wd, R.clip_scale(r64["sumsq"], clip_at))
            p32, h32 = sgd(start, r32["grads"], zeros, rate, mom, wd, R.clip_scale(r32["sumsq"], clip_at), dtype=np.float32)
        else:
            p64, h64 = sgd(p64, r64["grads"], h64, rate, mom, wd, 1.0)
            p32, h32 = sgd(p32, r32["grads"], h32, rate, mom, wd, 1.0, dtype=np.float32)
        sol.update(rate, mom, wd, cs)
        for k in keys:
            ok &= check("w_%s/%d" % (k, rep), sol.fetch("w_" + k), p64[k], p32[k], rows)
            ok &= check("h_%s/%d" % (k, rep), sol.fetch("h_" + k), h64[k], h32[k], rows)
    return ok


def det_sgd(*a, **kw):
    return R.sgd(*a, lr_mult=D.LR_MULT, decay_mult=D.DECAY_MULT, **kw)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["small", "voc", "coco"])
def test_det_step(ctx, name, channels_last):
    import torch
    head, fmap, blobs = B.det_case(name)
    print("%s head %s, %s" % (name, D.HEADS[name], "channels_last" if channels_last else "NCHW"))
    seed, it = 3, 0
    sol = make_det(ctx, head)
    conv = torch.from_numpy(fmap).cuda()
    if channels_last:
        conv = conv.contiguous(memory_format=torch.channels_last)
    dmap = torch.empty_like(conv)
    losses, sumsq = sol.step(*det_args(conv, blobs), seed, it, dmap=dmap)
    pool, arg = D.roi_pool(fmap, blobs["rois"])
    assert same_bits(sol.fetch("pool5"), pool) and same_bits(sol.fetch("argmax"), arg)          # as in fp32 mode
    masks = fetched_masks(sol, seed, it, D.LAYERS)
    relu_dropout_exact(sol, masks, D.LAYERS)
    r64 = B.det_step(head, pool, blobs, masks)
    r32 = B.det_step(head, pool, blobs, masks, dtype=np.float32)
    assert_gates_equal(sol, r64, (6, 7))
    rows, ok = [], True
    for nm in ("pre6", "a6", "pre7", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score", "d_bbox_pred", "d_pre7", "d_pre6",
               "d_pool5"):
        ok &= check(nm, sol.fetch(nm).reshape(np.shape(r64[nm])), r64[nm], r32[nm], rows)
    ok &= check("losses", losses, r64["losses"], r32["losses"], rows)
    for k in D.KEYS:
        ok &= check("g_" + k, sol.fetch("g_" + k), r64["grads"][k], r32["grads"][k], rows)
    ok &= check("sumsq", [sumsq], [r64["sumsq"]], [r32["sumsq"]], rows)
    d64 = D.roi_pool_backward(r64["d_pool5"], arg, blobs["rois"], fmap.shape)
    d32 = D.roi_pool_backward(r32["d_pool5"], arg, blobs["rois"], fmap.shape)
    ok &= check("d_conv5_3", dmap.cpu().numpy(), d64, d32, rows)
    ok &= two_updates(sol, D.KEYS, head, r64, r32, sumsq, det_sgd, rows)
    p_t, b_t = sol.forward_test(conv, blobs["rois"])                                           # TEST phase in the same mode
    (p64, b64), (p32, b32) = B.det_forward_test(sol.read(), pool), B.det_forward_test(sol.read(), pool, np.float32)
    ok &= check("cls_prob (test)", p_t, p64, p32, rows) & check("bbox_pred (test)", b_t, b64, b32, rows)
    sol.close()
    assert ok, exceeding(rows)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", sorted(B.AZ_CASES))
def test_az_step(ctx, name, channels_last):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = B.az_case(name)
    print("AZ case %s %s, %s" % (name, B.AZ_CASES[name], "channels_last" if channels_last else "NCHW"))
    seed, it = 3, 0
    sol = ffi.AzSolver(ctx, fmap.shape[1], head["W6"].shape[0], head["W71"].shape[0], head["W72"].shape[0], max_rois=256, seed=1, head=head)
    sol.set_precision(BF16)
    conv = torch.from_numpy(fmap).cuda()
    if channels_last:
        conv = conv.contiguous(memory_format=torch.channels_last)
    dmap = torch.empty_like(conv)
    losses, sumsq = sol.step(*az_args(conv, blobs), seed, it, dmap=dmap)
    pool, arg = R.roi_pool(fmap, blobs["rois"])
    assert same_bits(sol.fetch("pool5"), pool) and same_bits(sol.fetch("argmax"), arg)
    masks = fetched_masks(sol, seed, it, AZ_LAYERS)
    relu_dropout_exact(sol, masks, AZ_LAYERS)
    r64 = B.az_step(head, pool, blobs, masks)
    r32 = B.az_step(head, pool, blobs, masks, dtype=np.float32)
    assert_gates_equal(sol, r64, (6, 71, 72))
    rows, ok = [], True
    for nm in ("pre6", "a6", "pre71", "a71", "pre72", "a72", "adj_score", "adj_bbox", "zoom_score", "d_adj_score", "d_adj_bbox",
               "d_zoom_score", "d_pre71", "d_pre72", "d_pre6", "d_pool5"):
        ok &= check(nm, sol.fetch(nm).reshape(np.shape(r64[nm])), r64[nm], r32[nm], rows)
    ok &= check("losses", losses, r64["losses"], r32["losses"], rows)
    for k in R.KEYS:
        ok &= check("g_" + k, sol.fetch("g_" + k), r64["grads"][k], r32["grads"][k], rows)
    ok &= check("sumsq", [sumsq], [r64["sumsq"]], [r32["sumsq"]], rows)
    d64 = R.roi_pool_backward(r64["d_pool5"], arg, blobs["rois"], fmap.shape)
    d32 = R.roi_pool_backward(r32["d_pool5"], arg, blobs["rois"], fmap.shape)
    ok &= check("d_conv5_3", dmap.cpu().numpy(), d64, d32, rows)
    ok &= two_updates(sol, R.KEYS, head, r64, r32, sumsq, R.sgd, rows)
    sol.close()
    assert ok, exceeding(rows)


def make_skip(ctx, head, front, Cs, max_rois=256, seed=1, prec=BF16):
    sol = make_det(ctx, head, max_rois=max_rois, seed=seed, prec=prec)
    sol.attach_skip(Cs, S.SCALES, gain=front["gain"], eps=front["eps"], seed=seed, front=front)
    return sol


def to_dev(maps, channels_last=False):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]
    return [t.contiguous(memory_format=torch.channels_last) for t in out] if channels_last else out


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_skip_step(ctx, channels_last):
    import torch
    head, front, maps, blobs = B.skip_case()
    Cs = tuple(m.shape[1] for m in maps)
    Rn = blobs["rois"].shape[0]
    print("skip SMALL: Cs %s, Cout %d, R %d (%d rows), %s" % (Cs, front["Wp"].shape[0], Rn, Rn * 49, "channels_last" if channels_last else "NCHW"))
    seed, it = 3, 0
    sol = make_skip(ctx, head, front, Cs)
    dev = to_dev(maps, channels_last)
    dmaps = [torch.empty_like(m) for m in dev]
    args = (dev, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"])
    losses, sumsq = sol.step_skip(*args, seed, it, dmaps=dmaps)
    pooled = T.pool_argmax(maps, blobs["rois"])
    assert same_bits(sol.fetch("skip_argmax"), pooled[1]), "skip_argmax"
    masks = fetched_masks(sol, seed, it, D.LAYERS)
    r64 = B.skip_step(head, front, maps, blobs, masks, pooled=pooled)
    r32 = B.skip_step(head, front, maps, blobs, masks, dtype=np.float32, pooled=pooled)
    assert_gates_equal(sol, r64, (6, 7))
    diff = (T.unflatten_caffe(sol.fetch("pool5"), Rn) > 0) != r64["gates"]["pool"]
    print("  gates of relu_pool: %d of %d differ from the float64 bf16 model" % (int(diff.sum()), diff.size))
    assert not diff.any()
    rows, ok = [], True
    for nm in ("cat", "pool5", "pre6", "a6", "pre7", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score", "d_bbox_pred", "d_pre7",
               "d_pre6", "d_pool5", "d_y", "d_cat", "d_raw"):
        ok &= check(nm, sol.fetch(nm).reshape(np.shape(r64[nm])), r64[nm], r32[nm], rows)
    for i in range(3):
        ok &= check("d map %d" % i, dmaps[i].cpu().numpy(), r64["dmaps"][i], r32["dmaps"][i], rows)
    ok &= check("losses", losses, r64["losses"], r32["losses"], rows)
    for k in T.KEYS:
        ok &= check("g_" + k, sol.fetch("g_" + k), r64["grads"][k], r32["grads"][k], rows)
    ok &= check("sumsq", [sumsq], [r64["sumsq"]], [r32["sumsq"]], rows)
    start = dict(head, Wp=front["Wp"], bp=front["bp"])
    ok &= two_updates(sol, T.KEYS, start, r64, r32, sumsq, T.sgd, rows)
    sol.close()
    assert ok, exceeding(rows)


def test_skip_cat_has_fp32_mode_bits(ctx):
    """GRN, concat and scale are no matrix product: `cat` and the arg-max have the bits of fp32 mode."""
    head, front, maps, blobs = B.skip_case()
    Cs = tuple(m.shape[1] for m in maps)
    dev = to_dev(maps)
    out = []
    for prec in (FP32, BF16):
        sol = make_skip(ctx, head, front, Cs, prec=prec)
        sol.forward_test_skip(dev, blobs["rois"])
        out.append((sol.fetch("cat"), sol.fetch("skip_argmax"), sol.fetch("pool5")))
        sol.close()
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]) and not np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("name", ["voc", "coco"])
def test_integer_heads_bit_for_bit(ctx, name):
    """Integer maps, weights and biases: every operand, rounded to bf16 or not, is an integer, so every partial sum is one;
    where sum |q(a)| |q(w)| + |b| stays below 2^24 the device must give the float64 bf16 model's bits, whatever the order of
    the sum inside an instruction."""
    import torch
    d = D.HEADS[name]
    rng = np.random.Generator(np.random.PCG64(41))
    C, n6, n7, ncls, n = d["C"], d["n6"], d["n7"], d["ncls"], d["R"]
    ints = lambda shape, lo, hi: rng.integers(lo, hi + 1, shape).astype(np.float32)
    head = {"W6": ints((n6, C * 49), -8, 8), "b6": ints(n6, -3, 3), "W7": ints((n7, n6), -1, 1), "b7": ints(n7, -3, 3),
            "Wc": ints((ncls, n7), -1, 1), "bc": ints(ncls, -3, 3), "Wb": ints((4 * ncls, n7), -1, 1), "bb": ints(4 * ncls, -3, 3)}
    fmap = ints((2, C, D.MAP_H, D.MAP_W), 0, 8)
    blobs = D.random_blobs(9, n, 2, D.MAP_H, D.MAP_W, ncls)
    pool, _ = D.roi_pool(fmap, blobs["rois"])
    r = B.det_step(head, pool, blobs, None, want_dpool=False)
    plain = D.step(head, pool, blobs, None, want_dpool=False)
    x = pool.astype(np.float64)
    for nm, wk, bk, nxt in (("fc6", "W6", "b6", "a6"), ("fc7", "W7", "b7", "a7"), ("cls_score", "Wc", "bc", None), ("bbox_pred", "Wb", "bb", None)):
        worst = float((np.abs(B.q(x)) @ np.abs(B.q(head[wk])).T.astype(np.float64) + np.abs(head[bk])).max())
        print("  %s: largest possible |partial sum| %.0f (2^24 = %d)" % (nm, worst, 2 ** 24))
        assert worst < 2 ** 24
        if nxt is not None:
            x = r[nxt]
    # a6 needs more than 8 bits here: the bf16 model rounds it, and its scores are not the fp32 model's
    assert np.abs(r["a6"]).max() > 512 and not np.array_equal(B.q(r["a6"]), r["a6"])
    assert not np.array_equal(r["cls_score"], plain["cls_score"]) and np.abs(r["cls_score"]).max() > 100
    sol = make_det(ctx, head)
    sol.set_hyper(dropout_ratio=[0.0, 0.0])
    conv = torch.from_numpy(fmap).cuda()
    _, b = sol.forward_test(conv, blobs["rois"])
    for nm in ("pre6", "pre7", "cls_score"):
        assert same_bits(sol.fetch(nm), r[nm].astype(np.float32)), nm + " of forward_test"
    assert same_bits(b, r["bbox_pred"].astype(np.float32)), "bbox_pred of forward_test"
    sol.step(*det_args(conv, blobs), 1, 0)
    for nm in ("pre6", "pre7", "cls_score", "bbox_pred"):
        assert same_bits(sol.fetch(nm), r[nm].astype(np.float32)), nm + " of the step"
    sol.close()


DET_NAMES = ["pool5", "argmax", "pre6", "pre7", "mask6", "mask7", "a6", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score",
             "d_bbox_pred", "d_pre6", "d_pre7", "d_pool5"] + [p + k for p in ("g_", "w_", "h_") for k in D.KEYS]


def test_same_steps_twice_same_bits(ctx):
    import torch
    head, fmap, blobs = D.case("coco", seed=23)
    conv = torch.from_numpy(fmap).cuda()
    runs = []
    for _ in range(2):
        sol = make_det(ctx, head)
        dmap = torch.empty_like(conv)
        out = []
        for it in range(3):                                           # three steps: the history is part of the state
            losses, sq = sol.step(*det_args(conv, blobs), 9, it, dmap=dmap)
            sol.update(0.01, 0.9, 0.0005, R.clip_scale(sq, 0.5))
            out.append([losses.copy(), np.float64(sq), dmap.cpu().numpy()] + [sol.fetch(n) for n in DET_NAMES])
        runs.append(out)
        sol.close()
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a, b):
            assert same_bits(np.atleast_1d(x), np.atleast_1d(y))
    assert not np.array_equal(runs[0][0][0], runs[0][2][0])


# ---- 5. mode semantics ---------------------------------------------------------------------------------------------------------------
def det_snapshot(sol, conv, blobs, dmap):
    losses, sq = sol.step(*det_args(conv, blobs), 9, 0, dmap=dmap)
    return [losses.copy(), np.float64(sq), dmap.cpu().numpy()] + [sol.fetch(n) for n in DET_NAMES if n[:2] not in ("w_", "h_")]


def all_same(a, b):
    return all(same_bits(np.atleast_1d(x), np.atleast_1d(y)) for x, y in zip(a, b))


def test_det_mode_semantics(ctx):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = D.case("voc", seed=11)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.empty_like(conv)
    never, given = make_det(ctx, head, prec=None), make_det(ctx, head, prec=FP32)
    first = det_snapshot(never, conv, blobs, dmap)
    assert all_same(first, det_snapshot(given, conv, blobs, dmap)), "AZ_TRAIN_FP32 is not the default's bits"
    given.close()
    sol = never
    sol.set_precision(BF16)
    second = det_snapshot(sol, conv, blobs, dmap)
    sol.set_precision(FP32)
    third = det_snapshot(sol, conv, blobs, dmap)
    assert all_same(first, third), "fp32, bf16, fp32: the third step is not the first"
    i = DET_NAMES.index("pre6") + 3
    gap = B.rel_err(second[i], first[i])
    print("  pre6: bf16 mode is %.2e (relative) from fp32 mode" % gap)
    assert not np.array_equal(second[i], first[i]) and gap > 1e-4
    for mode, want in ((BF16, second), (FP32, first)):
        sol.set_precision(mode)
        for bad in (2, -1):
            with pytest.raises(ffi.AzError) as e:
                sol.set_precision(bad)
            assert e.value.code == ffi.AZ_ERR_INVALID
        assert all_same(want, det_snapshot(sol, conv, blobs, dmap)), "a refused value changed the mode"
    sol.close()
    a, b, _ = B.gemm_operands(0, 5, 6, 7, B.integer_draw(np.random.Generator(np.random.PCG64(1))))
    for bad in (2, -1):
        with pytest.raises(ffi.AzError) as e:
            ffi.gemm_unit(ctx, 0, a, b, precision=bad)
        assert e.value.code == ffi.AZ_ERR_INVALID
    assert same_bits(ffi.gemm_unit(ctx, 0, a, b), ffi.gemm_unit(ctx, 0, a, b, precision=FP32))


def test_az_mode_semantics(ctx):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = R.small_case(R=37, seed=19)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.empty_like(conv)
    names = ["pre6", "pre71", "pre72", "a6", "adj_score", "adj_bbox", "zoom_score", "d_pre6", "d_pre71", "d_pre72", "d_pool5"] + ["g_" + k for k in R.KEYS]

    def snap(sol):
        losses, sq = sol.step(*az_args(conv, blobs), 9, 0, dmap=dmap)
        return [losses.copy(), np.float64(sq), dmap.cpu().numpy()] + [sol.fetch(n) for n in names]
    mk = lambda: ffi.AzSolver(ctx, 16, 128, 64, 32, max_rois=64, head=head)
    never, given = mk(), mk()
    given.set_precision(FP32)
    first = snap(never)
    assert all_same(first, snap(given))
    given.close()
    never.set_precision(BF16)
    second = snap(never)
    never.set_precision(FP32)
    assert all_same(first, snap(never))
    assert not np.array_equal(second[3], first[3]) and B.rel_err(second[3], first[3]) > 1e-4
    never.set_precision(BF16)
    for bad in (2, -1):
        with pytest.raises(ffi.AzError) as e:
            never.set_precision(bad)
        assert e.value.code == ffi.AZ_ERR_INVALID
    assert all_same(second, snap(never))
    never.close()


# ---- 6. the front door --------------------------------------------------------------------------------------------------------------------
def traj_gates(sol, step_fn, before, pool, blobs, masks, layers):
    """The device's gates, allowed to differ from the float64 bf16 model only within rounding of zero and in at most 1e-4 of
    a layer's units (the rule of the existing trajectory tests), for the restatements to use."""
    gates = {t: sol.fetch("pre%d" % t) > 0 for t, _, _ in layers}
    r64 = step_fn(before, pool, blobs, masks, gates=gates, want_dpool=False)
    r32 = step_fn(before, pool, blobs, masks, gates=gates, dtype=np.float32, want_dpool=False)
    for t, _, _ in layers:
        pre64 = r64["pre%d" % t]
        fwd = B.bound(B.rel_err(r32["pre%d" % t], pre64)) * np.abs(pre64).max()
        diff = gates[t] != (pre64 > 0)
        print("  gates of layer %d: %d of %d differ from float64" % (t, int(diff.sum()), diff.size))
        assert np.all(np.abs(pre64[diff]) <= fwd), "a gate differs where the pre-activation is not within rounding of zero"
        assert diff.mean() <= 1e-4
    return gates


def test_det_front_door(ctx, tmp_path, monkeypatch):
    from aznet_hip import caffemodel as cm, ffi, synth
    from detect.config import cfg
    from detect.train_det import SolverWrapper
    from roi_data_layer import roidb as rdl
    TJ = D.TRAJ
    monkeypatch.setattr(cfg.TRAIN, "PRECISION", "bf16")
    ffi.set_default_context(ctx)
    imdb, _, _ = DR.synthetic_roidb(rdl, np.load(GOLD), tmp_path, monkeypatch)
    np.random.seed(TJ["np_seed"])
    sw = SolverWrapper(D.traj_solver_files(str(tmp_path)), imdb, str(tmp_path / "out"), backbone=D.traj_backbone("cuda:0"), ctx=ctx,
                       dims=dict(n6=TJ["n6"], n7=TJ["n7"]), seed=TJ["solver_seed"])
    start = sw.trainer.read()
    ref64, ref32 = B.DetTrajectory(start, np.float64, TJ["solver"]), B.DetTrajectory(start, np.float32, TJ["solver"])
    ok, tot = True, []
    for it in range(TJ["steps"]):
        before = sw.trainer.read()
        losses = sw.step()
        conv, blobs = sw.last_conv.cpu().numpy(), sw.last_blobs
        pool, _ = D.roi_pool(conv, blobs["rois"])
        print("step %d (%d rows)" % (it, pool.shape[0]))
        masks = fetched_masks(sw.trainer, TJ["solver_seed"], it, D.LAYERS)
        gates = traj_gates(sw.trainer, B.det_step, before, pool, blobs, masks, D.LAYERS)
        r64, r32 = ref64.step(conv, blobs, TJ["solver_seed"], gates), ref32.step(conv, blobs, TJ["solver_seed"], gates)
        ok &= check("losses[%d]" % it, losses, r64["losses"], r32["losses"])
        if it == 0:                                                   # the wrapper did put the trainer into bf16 mode
            fp = D.step(before, pool, blobs, masks, want_dpool=False)
            e_bf, e_fp = B.rel_err(sw.trainer.fetch("pre6"), r64["pre6"]), B.rel_err(sw.trainer.fetch("pre6"), fp["pre6"])
            print("  pre6: %.2e from the bf16 model, %.2e from the fp32 model" % (e_bf, e_fp))
            assert e_fp > 1e-4 > e_bf
        tot.append(float(np.sum(losses)))
    assert ok, "a step's losses exceed 8 x the float32-CPU error"
    print("summed loss: first five %.4f, last five %.4f" % (sum(tot[:5]), sum(tot[-5:])))
    assert sum(tot[-5:]) < sum(tot[:5])
    # the snapshot holds the fp32 master weights: it loads as ever, and its forward is the trainer's TEST-phase forward
    path = sw.snapshot()
    head = cm.det_head_from_layers(cm.load_caffemodel(path))
    conv0 = sw.last_conv[0:1].contiguous()
    rois = sw.last_blobs["rois"][sw.last_blobs["rois"][:, 0] == 0].copy()
    now = sw.trainer.read()
    assert np.array_equal(head["W6"], now["W6"]) and np.array_equal(head["Wb"], (now["Wb"] * sw.bbox_stds[:, None]).astype(np.float32))
    pool, _ = D.roi_pool(conv0.cpu().numpy(), rois)
    un = lambda b: b.astype(np.float64) * sw.bbox_stds + sw.bbox_means
    p_bf, b_bf = sw.trainer.forward_test(conv0, rois)                 # bf16 mode: against the bf16 model
    (p64, b64), (p32, b32) = B.det_forward_test(now, pool), B.det_forward_test(now, pool, np.float32)
    ok = check("cls_prob (trainer, bf16)", p_bf, p64, p32) & check("bbox_pred (trainer, bf16)", un(b_bf), un(b64), un(b32))
    sw.trainer.set_precision(FP32)                                    # fp32 mode: against the inference head on the snapshot
    p_tr, b_tr = sw.trainer.forward_test(conv0, rois)
    ctx.load_head(synth.make_head(seed=1, **synth.SMALL_DIMS))       # (a context takes a map once it has an AZ head: C = 16 too)
    ctx.load_det_head(head)
    ctx.set_feature_map(conv0.cpu().numpy())
    p_inf, b_inf = ctx.det_forward(rois)
    (p64, b64), (p32, b32) = D.forward_test(now, pool), D.forward_test(now, pool, dtype=np.float32)
    ok &= check("cls_prob (trainer, fp32)", p_tr, p64, p32) & check("cls_prob (az_det_forward)", p_inf, p64, p32)
    ok &= check("bbox_pred (trainer, fp32)", un(b_tr), un(b64), un(b32)) & check("bbox_pred (az_det_forward)", b_inf, un(b64), un(b32))
    assert ok


def test_az_front_door(ctx, tmp_path, monkeypatch):
    from aznet_hip import caffemodel as cm, ffi, synth
    from aznet_hip.net import HipAZNet
    from datasets.synthetic import SyntheticImdb
    from detect.config import cfg
    from detect.train_az import SolverWrapper, get_training_roidb
    TJ = R.TRAJ
    monkeypatch.setattr(cfg.TRAIN, "PRECISION", "bf16")
    ffi.set_default_context(ctx)
    imdb = SyntheticImdb(TJ["height"], TJ["width"], TJ["n_images"])
    np.random.seed(TJ["roidb_seed"])
    get_training_roidb(imdb)
    dims = {k: v for k, v in synth.SMALL_DIMS.items() if k != "C"}
    sw = SolverWrapper(R.traj_solver_files(str(tmp_path), True), imdb, str(tmp_path / "out"), backbone=R.traj_backbone("cuda:0"),
                       ctx=ctx, dims=dims, seed=TJ["solver_seed"])
    start = sw.trainer.read()
    ref64, ref32 = B.AzTrajectory(start, np.float64), B.AzTrajectory(start, np.float32)
    ok, tot = True, []
    for it in range(TJ["steps"]):
        before = sw.trainer.read()
        losses = sw.step()
        conv, blobs = sw.last_conv.cpu().numpy(), sw.last_blobs
        pool, _ = R.roi_pool(conv, blobs["rois"])
        print("step %d" % it)
        masks = fetched_masks(sw.trainer, TJ["solver_seed"], it, AZ_LAYERS)
        gates = traj_gates(sw.trainer, B.az_step, before, pool, blobs, masks, AZ_LAYERS)
        r64, r32 = ref64.step(conv, blobs, TJ["solver_seed"], gates), ref32.step(conv, blobs, TJ["solver_seed"], gates)
        ok &= check("losses[%d]" % it, losses, r64["losses"], r32["losses"])
        if it == 0:
            fp = R.step(before, pool, blobs, masks, want_dpool=False)
            e_bf, e_fp = B.rel_err(sw.trainer.fetch("pre6"), r64["pre6"]), B.rel_err(sw.trainer.fetch("pre6"), fp["pre6"])
            print("  pre6: %.2e from the bf16 model, %.2e from the fp32 model" % (e_bf, e_fp))
            assert e_fp > 1e-4 > e_bf
        tot.append(float(np.sum(losses)))
    assert ok, "a step's losses exceed 8 x the float32-CPU error"
    print("summed loss: first five %.4f, last five %.4f" % (sum(tot[:5]), sum(tot[-5:])))
    assert sum(tot[-5:]) < sum(tot[:5])
    path = sw.snapshot()
    layers = cm.load_caffemodel(path)
    conv0 = sw.last_conv[0:1].contiguous()
    rois = sw.last_blobs["rois"][sw.last_blobs["rois"][:, 0] == 0].copy()
    now = sw.trainer.read()
    pool, _ = R.roi_pool(conv0.cpu().numpy(), rois)
    z, a, b = sw.trainer.forward_test(conv0, rois)                    # bf16 mode: against the bf16 model
    r64, r32 = B.az_forward_test(now, pool), B.az_forward_test(now, pool, np.float32)
    ok = True
    for nm, got, x64, x32 in zip(("zoom_score", "adj_score", "adj_bbox"), (z, a, b), r64, r32):
        ok &= check(nm + " (trainer, bf16)", got, x64, x32)
    assert ok
    sw.trainer.set_precision(FP32)                                    # fp32 mode: against HipAZNet on the snapshot, as ever
    z, a, b = sw.trainer.forward_test(conv0, rois)
    net = HipAZNet(cm.az_head_from_layers(layers), ctx=ctx)
    net.set_conv(conv0)
    zp, ap, bb = ctx.head_forward(rois)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    assert np.abs(zp.reshape(-1) - sig(z)).max() <= 1e-4 and np.abs(ap - sig(a)).max() <= 1e-4
    assert np.abs(bb - (b.astype(np.float64) * sw.bbox_stds + sw.bbox_means)).max() <= 1e-4
