"""GPU: the AZ-net trainer (csrc/az_solver.hip, detect/train_az.py) against the float64 restatement tests/train_step_ref.py.

Tolerances (non-integer cases).  Per tensor the error is max|got - ref64| / max|ref64|; the bound is the same quantity for
the restatement run in float32 on the CPU against float64, computed here, times 8, floor 1e-6 (R.bound).  Integer-valued
GEMM cases are bit-exact.  ReLU gates: the device's gates may differ from float64's only where |pre-activation_64| is within
the forward bound, at most 1e-4 of a layer's units; the device's gates are then given to the restatement.  Every figure is
printed before it is asserted (run with -s to see the table)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import train_step_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ((6, 0, "b6"), (71, 1, "b71"), (72, 2, "b72"))


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def check(name, got, r64, r32, rows=None):
    e_dev, e_cpu = R.rel_err(got, r64), R.rel_err(r32, r64)
    b = R.bound(e_cpu)
    print("  %-14s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (name, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    if rows is not None:
        rows.append((name, e_dev, e_cpu, b))
    return e_dev <= b


DEFAULT_RATIOS = (0.5, 0.5, 0.5)


def device_masks(sol, seed, it, n, ratios=DEFAULT_RATIOS):
    """The fetched masks of the layers that have dropout (ratio > 0), each equal to the NumPy form of the generator."""
    from aznet_hip import ffi
    masks = {}
    for t, l, k in LAYERS:
        if ratios[l] > 0:
            m = sol.fetch("mask%d" % t)
            assert np.array_equal(m, ffi.dropout_mask(seed, it, l, m.size, ratio=ratios[l]).reshape(m.shape)), "mask of layer %d" % t
            masks[t] = m
    return masks


def device_gates(sol, head, pool, blobs, masks, ratios=DEFAULT_RATIOS, count=None):
    """The device's ReLU gates, checked against float64 as the issue allows, for the restatement to use.  count: a list
    that receives the number of gates that differed."""
    gates = {t: sol.fetch("pre%d" % t) > 0 for t, _, _ in LAYERS}
    r64 = R.step(head, pool, blobs, masks, gates=gates, ratios=ratios, want_dpool=False)
    r32 = R.step(head, pool, blobs, masks, gates=gates, dtype=np.float32, ratios=ratios, want_dpool=False)
    for t, _, _ in LAYERS:
        pre64 = r64["pre%d" % t]
        fwd = R.bound(R.rel_err(r32["pre%d" % t], pre64)) * np.abs(pre64).max()
        diff = gates[t] != (pre64 > 0)
        print("  gates of layer %d: %d of %d differ from float64" % (t, int(diff.sum()), diff.size))
        assert np.all(np.abs(pre64[diff]) <= fwd), "a gate differs where the pre-activation is not within rounding of zero"
        assert diff.mean() <= 1e-4
        if count is not None:
            count.append(int(diff.sum()))
    return gates


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run_and_compare(ctx, head, fmap, blobs, seed, it, channels_last=False, max_rois=256, update=True, ratios=None, lr_mult=None,
                    decay_mult=None):
    """ratios / lr_mult / decay_mult (dicts by parameter name): hyper-parameters other than az_solver_create's, set after a
    step at the defaults, so that a layer whose ratio is 0 finds a stale mask in its buffer that it must not look at."""
    import torch
    from aznet_hip import ffi
    N, C, H, W = fmap.shape
    n6, n71, n72 = head["W6"].shape[0], head["W71"].shape[0], head["W72"].shape[0]
    sol = ffi.AzSolver(ctx, C, n6, n71, n72, max_rois=max_rois, seed=1, head=head)
    conv = torch.from_numpy(fmap).cuda()
    if channels_last:
        conv = conv.contiguous(memory_format=torch.channels_last)
    dmap = torch.empty_like(conv)
    args = (conv, blobs["rois"], blobs["adj_labels"], blobs["adj_targets"], blobs["adj_loss_weights"], blobs["zoom_labels"])
    other = not (ratios is None and lr_mult is None and decay_mult is None)
    ratios = DEFAULT_RATIOS if ratios is None else tuple(ratios)
    lr_mult, decay_mult = lr_mult or R.LR_MULT, decay_mult or R.DECAY_MULT
    stale = {}
    if other:
        sol.step(*args, seed + 1, it, dmap=dmap)
        stale = {t: sol.fetch("mask%d" % t) for t, _, _ in LAYERS}
        assert all(0.4 < m.mean() < 0.6 for m in stale.values())
        sol.set_hyper([lr_mult[k] for k in R.KEYS], [decay_mult[k] for k in R.KEYS], ratios)
    losses, sumsq = sol.step(*args, seed, it, dmap=dmap)
    pool, arg = R.roi_pool(fmap, blobs["rois"])
    assert np.array_equal(sol.fetch("pool5"), pool), "pool5"
    assert np.array_equal(sol.fetch("argmax"), arg), "argmax"
    n = pool.shape[0]
    masks = device_masks(sol, seed, it, n, ratios)
    ngates = []
    gates = device_gates(sol, head, pool, blobs, masks, ratios, ngates)
    for t, l, _ in LAYERS:                                            # ReLU + dropout: exact given the pre-activation
        pre, a, dp = sol.fetch("pre%d" % t), sol.fetch("a%d" % t), sol.fetch("d_pre%d" % t)
        relu = np.maximum(pre, np.float32(0))
        if ratios[l] > 0:
            scale = np.float32(1) / (np.float32(1) - np.float32(ratios[l]))
            assert same_bits(a, np.where(masks[t] > 0, relu * scale, np.float32(0)).astype(np.float32)), "a%d" % t
            assert not dp[(pre <= 0) | (masks[t] == 0)].any()
        else:                                                         # no dropout: the stale mask is neither read nor written
            assert same_bits(a, relu), "a%d without dropout is not relu(pre%d)" % (t, t)
            assert not dp[pre <= 0].any()
            if stale:
                assert same_bits(sol.fetch("mask%d" % t), stale[t])
                dropped = (pre > 0) & (stale[t] == 0)
                print("  layer %d without dropout: %d of %d units with a zero in the stale mask have d_pre != 0"
                      % (t, int(np.count_nonzero(dp[dropped])), int(dropped.sum())))
                assert dropped.any() and np.count_nonzero(dp[dropped]) > 0        # gated by pre > 0 alone (values: d_pre below)
    r64 = R.step(head, pool, blobs, masks, gates=gates, ratios=ratios)
    r32 = R.step(head, pool, blobs, masks, gates=gates, dtype=np.float32, ratios=ratios)
    rows, ok = [("gates that differ", float(sum(ngates)), 0.0, 0.0)], True
    for name in ("pre6", "a6", "pre71", "pre72", "adj_score", "adj_bbox", "zoom_score", "d_adj_score", "d_adj_bbox",
                 "d_zoom_score", "d_pre71", "d_pre72", "d_pre6", "d_pool5"):
        ok &= check(name, sol.fetch(name).reshape(np.shape(r64[name])), r64[name], r32[name], rows)
    ok &= check("losses", losses, r64["losses"], r32["losses"], rows)
    for k in R.KEYS:
        ok &= check("g_" + k, sol.fetch("g_" + k), r64["grads"][k], r32["grads"][k], rows)
    ok &= check("sumsq", [sumsq], [r64["sumsq"]], [r32["sumsq"]], rows)
    d64 = R.roi_pool_backward(r64["d_pool5"], arg, blobs["rois"], fmap.shape)
    d32 = R.roi_pool_backward(r32["d_pool5"], arg, blobs["rois"], fmap.shape)
    ok &= check("d_conv5_3", dmap.cpu().numpy(), d64, d32, rows)
    if update:
        rate, mom, wd = 0.001, 0.9, 0.0005
        mult = dict(lr_mult=lr_mult, decay_mult=decay_mult)
        for rep, clip_at in ((0, 1e-3), (1, None)):                 # a clipped step, then an unclipped one on top of its history
            cs = R.clip_scale(sumsq, clip_at)
            if rep == 0:
                p64, h64 = R.sgd(head, r64["grads"], {k: np.zeros_like(v) for k, v in head.items()}, rate, mom, wd, R.clip_scale(r64["sumsq"], clip_at), **mult)
                p32, h32 = R.sgd(head, r32["grads"], {k: np.zeros_like(v) for k, v in head.items()}, rate, mom, wd, R.clip_scale(r32["sumsq"], clip_at), dtype=np.float32, **mult)
                assert cs < 1.0
            else:
                p64, h64 = R.sgd(p64, r64["grads"], h64, rate, mom, wd, 1.0, **mult)
                p32, h32 = R.sgd(p32, r32["grads"], h32, rate, mom, wd, 1.0, dtype=np.float32, **mult)
            sol.update(rate, mom, wd, cs)
            for k in R.KEYS:
                ok &= check("w_%s/%d" % (k, rep), sol.fetch("w_" + k), p64[k], p32[k], rows)
                ok &= check("h_%s/%d" % (k, rep), sol.fetch("h_" + k), h64[k], h32[k], rows)
        got = sol.read()
        assert all(np.array_equal(got[k], sol.fetch("w_" + k)) for k in R.KEYS)
        for k in R.KEYS:                                              # lr_mult 0: after the two updates not a bit has moved
            if lr_mult[k] == 0:
                assert np.abs(sol.fetch("g_" + k)).max() > 0, k
                assert same_bits(sol.fetch("w_" + k), head[k]) and same_bits(sol.fetch("h_" + k), np.zeros_like(head[k])), k
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error: " + ", ".join(r[0] for r in rows[1:] if r[1] > r[3])
    return rows


# ---- 1. pieces ----------------------------------------------------------------------------------------------------------
def test_roi_pool_equals_az_roi_pool_per_image(ctx):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = R.small_case(R=96, seed=13)
    d = {k: head[k].shape[0] for k in ("W6", "W71", "W72")}
    sol = ffi.AzSolver(ctx, fmap.shape[1], d["W6"], d["W71"], d["W72"], max_rois=128, head=head)
    ctx.load_head(head)
    for cl in (False, True):
        conv = torch.from_numpy(fmap).cuda()
        if cl:
            conv = conv.contiguous(memory_format=torch.channels_last)
        sol.forward_test(conv, blobs["rois"])
        pool, arg = sol.fetch("pool5"), sol.fetch("argmax")
        rp, ra = R.roi_pool(fmap, blobs["rois"])
        assert np.array_equal(arg, ra) and np.array_equal(pool, rp)
        for i in range(fmap.shape[0]):
            rows = np.where(blobs["rois"][:, 0] == i)[0]
            assert rows.size > 0
            ctx.set_feature_map(fmap[i:i + 1])
            rois = blobs["rois"][rows].copy()
            rois[:, 0] = 0
            assert np.array_equal(ctx.roi_pool(rois), pool[rows]), "image %d" % i
    sol.close()


@pytest.mark.parametrize("rows", [1, 5, 128, 130])
def test_gemm_forms_integer_exact_and_random(ctx, rows):
    from aznet_hip import ffi
    rng = np.random.Generator(np.random.PCG64(rows))
    ok = True
    for n_out, k_in in ((63, 200), (31, 1027), (256, 96)):           # odd n71 / n72, K not a multiple of the tile
        # form 0: y = x W^T; 1: dx = dy W; 2: dW = dy^T x   (x [rows, k_in], W [n_out, k_in], dy [rows, n_out])
        for form in (0, 1, 2):
            def operands(draw):
                x, W, dy = draw((rows, k_in)), draw((n_out, k_in)), draw((rows, n_out))
                return {0: (x, W, x @ W.T.astype(np.float64)), 1: (dy, W, dy @ W.astype(np.float64)),
                        2: (dy, x, dy.T.astype(np.float64) @ x)}[form]
            a, b, want = operands(lambda s: rng.integers(-8, 9, s).astype(np.float32))     # |sum| < 2^24: exact in fp32
            got = ffi.gemm_unit(ctx, form, a, b)
            assert got.shape == want.shape and np.array_equal(got, want.astype(np.float32)), (form, rows, n_out, k_in)
            a, b, want = operands(lambda s: rng.standard_normal(s).astype(np.float32))
            cpu = {0: lambda: a @ b.T, 1: lambda: a @ b, 2: lambda: a.T @ b}[form]()
            ok &= check("form %d %dx%dx%d" % (form, rows, n_out, k_in), ffi.gemm_unit(ctx, form, a, b), want, cpu)
    assert ok


def test_losses_and_activations_alone(ctx):
    """Each loss, ReLU / dropout and RoIPool backward from the DEVICE's own inputs: the restatement's functions applied to
    the tensors the device fetched, so that only the one piece is between the two."""
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = R.small_case(R=37, seed=17)
    blobs["adj_labels"][0, :3] = (0.0, 1.0, 0.37)
    head["bas"][:] = (-60, 60, 0, 30, -30, 90, -90, 1, -1, 5, -5)     # large |x|: no overflow
    d = {k: head[k].shape[0] for k in ("W6", "W71", "W72")}
    sol = ffi.AzSolver(ctx, fmap.shape[1], d["W6"], d["W71"], d["W72"], max_rois=64, head=head)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.empty_like(conv)
    losses, _ = sol.step(conv, blobs["rois"], blobs["adj_labels"], blobs["adj_targets"], blobs["adj_loss_weights"],
                         blobs["zoom_labels"], 5, 2, dmap=dmap)
    assert np.all(np.isfinite(losses))
    ok = True
    n = 37.0
    for name, fn, args in (("zoom", R.sigmoid_ce, (sol.fetch("zoom_score").reshape(-1), blobs["zoom_labels"])),
                           ("adj", R.sigmoid_ce, (sol.fetch("adj_score"), blobs["adj_labels"])),
                           ("bbox", R.smooth_l1, (sol.fetch("adj_bbox"), blobs["adj_targets"], blobs["adj_loss_weights"]))):
        l64, g64 = fn(*[np.asarray(a, np.float64) for a in args], n)
        l32, g32 = fn(*[np.asarray(a, np.float32) for a in args], np.float32(n))
        i = ("zoom", "adj", "bbox").index(name)
        ok &= check("loss_" + name, [losses[i]], [l64], [l32])
        ok &= check("d_" + name, sol.fetch(("d_zoom_score", "d_adj_score", "d_adj_bbox")[i]).reshape(g64.shape), g64, g32)
    for t, l, k in LAYERS:                                             # ReLU + dropout forward: exact given pre
        pre, m = sol.fetch("pre%d" % t), sol.fetch("mask%d" % t)
        assert np.array_equal(m, ffi.dropout_mask(5, 2, l, m.size).reshape(m.shape))
        assert np.array_equal(sol.fetch("a%d" % t), np.where(m > 0, np.maximum(pre, 0) * np.float32(2), 0).astype(np.float32))
        dp = sol.fetch("d_pre%d" % t)
        assert not dp[(pre <= 0) | (m == 0)].any()
    dp, arg = sol.fetch("d_pool5"), sol.fetch("argmax")
    ok &= check("roi_pool_bwd", dmap.cpu().numpy(), R.roi_pool_backward(dp.astype(np.float64), arg, blobs["rois"], fmap.shape),
                R.roi_pool_backward(dp, arg, blobs["rois"], fmap.shape))
    sol.close()
    assert ok


def test_bad_arguments_write_nothing(ctx):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = R.small_case(R=8)
    with pytest.raises(ffi.AzError):
        ffi.AzSolver(ctx, 18, 128, 64, 32)                            # C not a multiple of 4
    sol = ffi.AzSolver(ctx, 16, 128, 64, 32, max_rois=8, head=head)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.full_like(conv, 7.0)
    args = lambda b: (conv, b["rois"], b["adj_labels"], b["adj_targets"], b["adj_loss_weights"], b["zoom_labels"], 1, 0)
    bad = dict(blobs, rois=blobs["rois"].copy())
    bad["rois"][3, 0] = 2                                             # an image the batch does not have
    with pytest.raises(ffi.AzError) as e:
        sol.step(*args(bad), dmap=dmap)
    assert e.value.code == ffi.AZ_ERR_INVALID and float(dmap.min()) == 7.0 and float(dmap.max()) == 7.0
    head9, fmap9, blobs9 = R.small_case(R=9)
    with pytest.raises(ffi.AzError):
        sol.step(*args(blobs9), dmap=dmap)                            # more rows than max_rois
    with pytest.raises(ffi.AzError):
        sol.update(0.001, 0.9, 0.0005, 1.0)                           # no gradients yet
    with pytest.raises(ffi.AzError):
        sol.fetch("no_such_tensor")
    sol.step(*args(blobs), dmap=None)                                 # without d conv5_3
    sol.close()


# ---- 2. one step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,channels_last,dims", [(128, False, None), (130, True, None), (5, False, None), (1, True, None),
                                                     (37, False, (12, 132, 68, 36))],       # (odd sizes: no multiple of a tile)
                         ids=["128-False", "130-True", "5-False", "1-True", "37-False-12x132x68x36"])
def test_one_step_reduced_head(ctx, rows, channels_last, dims):
    head, fmap, blobs = R.small_case(R=rows, dims=dims)
    print("reduced head%s, R = %d, %s" % ("" if dims is None else " %s" % (dims,), rows, "channels_last" if channels_last else "NCHW"))
    run_and_compare(ctx, head, fmap, blobs, seed=3, it=0, channels_last=channels_last)


def test_one_step_full_size(ctx):
    head, fmap, blobs = R.full_size_case()
    print("full size: C = 512, n6 = 4096, R = 128, N = 2, 38 x 63")
    run_and_compare(ctx, head, fmap, blobs, seed=3, it=0, max_rois=128)


# ---- 3. determinism ------------------------------------------------------------------------------------------------------
def test_same_step_twice_same_bits(ctx):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = R.small_case(R=130, seed=23)
    conv = torch.from_numpy(fmap).cuda()
    names = ["pool5", "argmax", "pre6", "pre71", "pre72", "mask6", "a6", "adj_score", "adj_bbox", "zoom_score", "d_pre6",
             "d_pre71", "d_pre72", "d_pool5"] + [p + k for p in ("g_", "w_", "h_") for k in R.KEYS]
    runs = []
    for _ in range(2):
        sol = ffi.AzSolver(ctx, 16, 128, 64, 32, max_rois=130, head=head)
        dmap = torch.empty_like(conv)
        out = []
        for it in range(3):                                           # three steps: the history is part of the state
            losses, sq = sol.step(conv, blobs["rois"], blobs["adj_labels"], blobs["adj_targets"], blobs["adj_loss_weights"],
                                  blobs["zoom_labels"], 9, it, dmap=dmap)
            sol.update(0.01, 0.9, 0.0005, R.clip_scale(sq, 0.5))
            out.append([losses.copy(), np.float64(sq), dmap.cpu().numpy()] + [sol.fetch(n) for n in names])
        runs.append(out)
        sol.close()
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a, b):
            assert np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8))
    # the fillers are seeded: the same seed gives the same weights, another seed others, at Caffe's stds
    w = [ffi.AzSolver(ctx, 16, 128, 64, 32, max_rois=8, seed=s) for s in (4, 4, 5)]
    p = [s.read() for s in w]
    assert all(np.array_equal(p[0][k], p[1][k]) for k in R.KEYS) and not np.array_equal(p[0]["W6"], p[2]["W6"])
    assert abs(p[0]["W6"].std() / 1e-4 - 1) < 0.05 and abs(p[0]["W72"].std() / 1e-3 - 1) < 0.1 and not p[0]["b6"].any()
    assert abs(p[0]["W6"].mean()) < 1e-5
    for s in w:
        s.close()


# ---- 4 / 5. trajectories through SolverWrapper, the snapshot's round trip, the tools ---------------------------------------------
def _wrapper(ctx, tmp, frozen_all, edit_rows=None):
    from aznet_hip import ffi, synth
    from datasets.synthetic import SyntheticImdb
    from detect.train_az import SolverWrapper, get_training_roidb
    T = R.TRAJ
    ffi.set_default_context(ctx)
    imdb = SyntheticImdb(T["height"], T["width"], T["n_images"])
    np.random.seed(T["roidb_seed"])
    get_training_roidb(imdb)
    dims = {k: v for k, v in synth.SMALL_DIMS.items() if k != "C"}
    return SolverWrapper(R.traj_solver_files(str(tmp), frozen_all, edit_rows), imdb, str(tmp / "out"), backbone=R.traj_backbone("cuda:0"),
                         ctx=ctx, dims=dims, seed=T["solver_seed"])


def test_frozen_trajectory_and_round_trip(ctx, tmp_path):
    from aznet_hip import caffemodel as cm
    T = R.TRAJ
    sw = _wrapper(ctx, tmp_path, True)
    assert sw.conv_train == []
    start = sw.trainer.read()
    ref64, ref32 = R.RefTrajectory(start, np.float64), R.RefTrajectory(start, np.float32)
    ok, tot = True, []
    for it in range(T["steps"]):
        before = sw.trainer.read()
        losses = sw.step()
        conv, blobs = sw.last_conv.cpu().numpy(), sw.last_blobs
        pool, _ = R.roi_pool(conv, blobs["rois"])
        print("step %d" % it)
        masks = device_masks(sw.trainer, T["solver_seed"], it, pool.shape[0])
        gates = device_gates(sw.trainer, before, pool, blobs, masks)
        r64, r32 = ref64.step(conv, blobs, T["solver_seed"], gates), ref32.step(conv, blobs, T["solver_seed"], gates)
        ok &= check("losses[%d]" % it, losses, r64["losses"], r32["losses"])
        tot.append(float(np.sum(losses)))
    assert ok, "a step's losses exceed 8 x the float32-CPU error"
    print("summed loss: first five %.4f, last five %.4f" % (sum(tot[:5]), sum(tot[-5:])))
    assert sum(tot[-5:]) < sum(tot[:5])
    # round trip: the snapshot in HipAZNet against the trainer's test-mode forward after the same un-normalisation
    path = sw.snapshot()
    assert os.path.basename(path) == "az_small_iter_20.caffemodel"
    layers = cm.load_caffemodel(path)
    assert set(layers) >= set(["conv1_1", "conv5_3", "int6", "zoom_score"])
    from aznet_hip.net import HipAZNet
    conv0 = sw.last_conv[0:1].contiguous()
    rois = sw.last_blobs["rois"][sw.last_blobs["rois"][:, 0] == 0].copy()
    z, a, b = sw.trainer.forward_test(conv0, rois)
    net = HipAZNet(cm.az_head_from_layers(layers), ctx=ctx)
    net.set_conv(conv0)
    zp, ap, bb = ctx.head_forward(rois)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    assert np.abs(zp.reshape(-1) - sig(z)).max() <= 1e-4 and np.abs(ap - sig(a)).max() <= 1e-4
    assert np.abs(bb - (b.astype(np.float64) * sw.bbox_stds + sw.bbox_means)).max() <= 1e-4
    bk = cm.backbone_from_layers(layers)
    assert all(np.array_equal(bk[l[0]][0], l[1].detach().cpu().numpy()) for l in sw.backbone.layers if l is not None)


def test_convolutions_train_with_the_same_update(ctx, tmp_path):
    import torch
    from aznet_hip import ffi
    from detect import prototxt as P
    T = R.TRAJ
    sw = _wrapper(ctx, tmp_path, False)
    names = [c[0] for c in sw.conv_train]
    assert names == list(P.CONV_LAYERS[4:])
    w0 = {l[0]: (l[1].detach().cpu().numpy().copy(), l[2].detach().cpu().numpy().copy()) for l in sw.backbone.layers if l is not None}
    tot = [float(np.sum(sw.step()))]
    sp = sw.solver_param
    norm = np.sqrt(sw.last_sumsq)
    assert sw.last_sumsq > sw.last_head_sumsq > 0
    assert sw.last_clip == (sp["clip_gradients"] / norm if norm > sp["clip_gradients"] else 1.0)
    worst = 0
    for name, w, b, hw, hb, lr, dc in sw.conv_train:
        for p, h, q in ((w, hw, 0), (b, hb, 1)):
            want_w, want_h = ffi.sgd_update_numpy(w0[name][q], p.grad.cpu().numpy(), np.zeros_like(w0[name][q]),
                                                  sw.last_rate * lr[q], sp["momentum"], sp["weight_decay"] * dc[q], sw.last_clip)
            got_w, got_h = p.detach().cpu().numpy(), h.cpu().numpy()
            assert np.abs(p.grad.cpu().numpy()).max() > 0, name
            for got, want in ((got_w, want_w), (got_h, want_h)):
                ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                worst = max(worst, float(ulp.max()))
    print("trainable convolution parameters after step 1: at most %.1f ulp from the NumPy form" % worst)
    assert worst <= 1.0
    for l in sw.backbone.layers:
        if l is not None and l[0] not in names:
            assert np.array_equal(l[1].detach().cpu().numpy(), w0[l[0]][0]) and np.array_equal(l[2].detach().cpu().numpy(), w0[l[0]][1])
    for _ in range(T["steps"] - 1):
        tot.append(float(np.sum(sw.step())))
    print("summed loss: first five %.4f, last five %.4f" % (sum(tot[:5]), sum(tot[-5:])))
    assert sum(tot[-5:]) < sum(tot[:5])
    for l in sw.backbone.layers:
        if l is not None and l[0] not in names:
            assert np.array_equal(l[1].detach().cpu().numpy(), w0[l[0]][0])


def test_train_tool_then_prop_az(tmp_path):
    tools = os.path.join(REPO, "az-net_amd", "tools")
    exp = "train_tool_test_%d" % os.getpid()
    out = subprocess.run([sys.executable, os.path.join(tools, "train_az_net.py"), "--net", "synthetic:8", "--imdb",
                          "synthetic_600x1000_8", "--iters", "4", "--exp", exp], capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:], out.stderr[-3000:])
    assert out.returncode == 0
    snap = os.path.join(REPO, "az-net_amd", "output", exp, "synthetic_600x1000_8", "vgg16_az_net_iter_4.caffemodel")
    assert os.path.exists(snap) and "Iteration 0, loss" in out.stdout
    out = subprocess.run([sys.executable, os.path.join(tools, "prop_az.py"), "--net", snap, "--imdb", "synthetic_600x1000_8",
                          "--tz", "0.0", "--exp", exp], capture_output=True, text=True, timeout=900)
    print(out.stdout[-2000:], out.stderr[-3000:])
    assert out.returncode == 0
    import shutil
    shutil.rmtree(os.path.join(REPO, "az-net_amd", "output", exp), ignore_errors=True)
