"""GPU: detection-net training -- the box-regression targets (csrc/az_det_train.hip) against what the reference recorded
(tests/golden/g21_train_det.npz), the trainer (csrc/az_det_solver.hip) against the float64 restatement tests/det_step_ref.py,
and the front door (roi_data_layer, detect/train_det.py, tools/train_det_net.py).

Targets: labels, dx, dy and max_overlaps bit for bit; dw and dh within one float32 step (the device's f64 log may be a few
ulp of f64 off NumPy's, which can move the float32 rounding by at most one step); the statistics, fed the golden's own
un-normalised targets, bit for bit.

Tolerances are those of tests/test_gpu_train_step.py.  Per tensor the error is max|got - ref64| / max|ref64|; the bound is the
same quantity for the restatement run in float32 on the CPU against float64, computed here, times 8, floor 1e-6 (bound).
Integer-valued cases are bit-exact.  ReLU gates: the device's gates may differ from float64's only where
|pre-activation_64| is within the forward bound, at most 1e-4 of a layer's units; the device's gates are then given to the
restatement.  Every figure is printed before it is asserted (run with -s to see the table)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import det_step_ref as D
import det_train_ref as DR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g21_train_det.npz")
K = 21


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def check(name, got, r64, r32, rows=None):
    e_dev, e_cpu = D.rel_err(got, r64), D.rel_err(r32, r64)
    b = D.bound(e_cpu)
    print("  %-14s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (name, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    if rows is not None:
        rows.append((name, e_dev, e_cpu, b))
    return e_dev <= b


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def device_masks(sol, seed, it, ratios=(0.5, 0.5)):
    from aznet_hip import ffi
    masks = {}
    for t, l, _ in D.LAYERS:
        if ratios[l] > 0:
            m = sol.fetch("mask%d" % t)
            assert np.array_equal(m, ffi.dropout_mask(seed, it, l, m.size, ratio=ratios[l]).reshape(m.shape)), "mask of layer %d" % t
            masks[t] = m
    return masks


def device_gates(sol, head, pool, blobs, masks, count=None, ratios=(0.5, 0.5)):
    gates = {t: sol.fetch("pre%d" % t) > 0 for t, _, _ in D.LAYERS}
    r64 = D.step(head, pool, blobs, masks, gates=gates, ratios=ratios, want_dpool=False)
    r32 = D.step(head, pool, blobs, masks, gates=gates, dtype=np.float32, ratios=ratios, want_dpool=False)
    for t, _, _ in D.LAYERS:
        pre64 = r64["pre%d" % t]
        fwd = D.bound(D.rel_err(r32["pre%d" % t], pre64)) * np.abs(pre64).max()
        diff = gates[t] != (pre64 > 0)
        print("  gates of layer %d: %d of %d differ from float64" % (t, int(diff.sum()), diff.size))
        assert np.all(np.abs(pre64[diff]) <= fwd), "a gate differs where the pre-activation is not within rounding of zero"
        assert diff.mean() <= 1e-4
        if count is not None:
            count.append(int(diff.sum()))
    return gates


def make_solver(ctx, head, max_rois=256, seed=1):
    from aznet_hip import ffi
    n6, n7, ncls = head["W6"].shape[0], head["W7"].shape[0], head["Wc"].shape[0]
    return ffi.AzDetSolver(ctx, head["W6"].shape[1] // 49, n6, n7, ncls, max_rois=max_rois, seed=seed, head=head)


def step_args(conv, blobs):
    return (conv, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"])


# ---- targets -------------------------------------------------------------------------------------------------------------
def ulp_steps(a, b):
    """How many float32 values apart two float32 arrays are, element by element."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 31) - i, i)
    return np.abs(key(a) - key(b))


def check_targets(got, want, what):
    """labels, dx, dy bit for bit; dw, dh within one float32 step."""
    assert got.shape == want.shape and got.dtype == np.float32
    assert same_bits(got[:, :3], want[:, :3]), "%s: labels / dx / dy" % what
    steps = ulp_steps(got[:, 3:], want[:, 3:])
    print("  %s: %d of %d dw / dh values differ at all, the furthest by %d float32 step(s)"
          % (what, int((steps > 0).sum()), steps.size, int(steps.max()) if steps.size else 0))
    assert steps.size == 0 or steps.max() <= 1, what
    return int((steps > 0).sum())


def test_targets_on_the_golden_cases(ctx, g):
    n = int(g["n_cases"])
    ex = [g["c%d_ex" % i] for i in range(n)]
    off = np.concatenate([[0], np.cumsum([e.shape[0] for e in ex])]).astype(np.int32)
    # one launch for all the images of the call, the one without objects among them
    t, mo = ctx.det_targets(np.vstack(ex), off, [g["c%d_gt" % i] for i in range(n)], [g["c%d_labels" % i] for i in range(n)],
                            0.5, 0.1, 1e-14)
    for i in range(n):
        ti, mi = t[off[i]:off[i + 1]], mo[off[i]:off[i + 1]]
        check_targets(ti, g["c%d_targets" % i], "case %d" % i)
        want = g["c%d_max_overlaps" % i]
        assert same_bits(mi, want.astype(np.float64)), "max_overlaps of case %d" % i
    one = ctx.det_targets(ex[3], [0, ex[3].shape[0]], [g["c3_gt"]], [g["c3_labels"]], 0.5, 0.1, 1e-14)
    assert same_bits(one[0], t[off[3]:off[4]]) and one[1][0] == 0.5 and one[0][0, 0] == 1 and one[0][1, 0] == 0


def test_target_stats_bit_for_bit(ctx, g):
    n = int(g["n_cases"])
    raw = [g["c%d_targets" % i] for i in range(n)]
    off = np.concatenate([[0], np.cumsum([t.shape[0] for t in raw])]).astype(np.int32)
    runs = []
    for _ in range(2):
        t = np.ascontiguousarray(np.vstack(raw))
        counts, means, stds = ctx.det_target_stats(t, off, K, 1e-14, True)
        runs.append((t, counts, means, stds))
    t, counts, means, stds = runs[0]
    assert same_bits(means.ravel(), g["set_means"]), "means"
    assert same_bits(stds.ravel(), g["set_stds"]), "stds"
    for i in range(n):
        assert same_bits(t[off[i]:off[i + 1]], g["c%d_norm" % i]), "normalised targets of case %d" % i
    want_counts = 1e-14 + np.array([sum(int((r[:, 0] == c).sum()) for r in raw) if c else 0 for c in range(K)], np.float64)
    assert same_bits(counts, want_counts)
    assert all(same_bits(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ"
    # without normalisation the targets come back untouched; the synthetic set (16 images) as well
    t = np.ascontiguousarray(np.vstack(raw))
    _, m2, s2 = ctx.det_target_stats(t, off, K, 1e-14, False)
    assert same_bits(t, np.vstack(raw)) and same_bits(m2, means) and same_bits(s2, stds)


def test_roidb_and_layer_against_the_reference(ctx, g, tmp_path, monkeypatch):
    """add_bbox_regression_targets and RoIDataLayer.forward() on the GPU against the golden set and minibatches, np.random's
    state included."""
    from aznet_hip import ffi
    from roi_data_layer import roidb as rdl
    from roi_data_layer.minibatch import get_minibatch
    ffi.set_default_context(ctx)
    imdb, means, stds = DR.synthetic_roidb(rdl, g, tmp_path, monkeypatch)
    differ = 0
    for i, e in enumerate(imdb.roidb):
        for k in ("ex_boxes", "gt_boxes", "max_overlaps"):
            assert same_bits(e[k], g["syn%d_%s" % (i, k)]), (i, k)
        assert e["bbox_targets"].dtype == np.float32 and same_bits(e["bbox_targets"][:, 0], g["syn%d_bbox_targets" % i][:, 0])
    # the un-normalised targets of the set, by the device, against the reference's (recovered from the restatement, which
    # equals the reference bit for bit on the CPU)
    ex = [e["ex_boxes"] for e in imdb.roidb]
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in ex])]).astype(np.int32)
    t, _ = ctx.det_targets(np.vstack(ex), off, [e["gt_boxes"] for e in imdb.roidb], [e["gt_labels"] for e in imdb.roidb], 0.5, 0.1, 1e-14)
    raw = np.vstack([DR.compute_targets(e["ex_boxes"], e["gt_boxes"], e["gt_labels"])[0] for e in imdb.roidb])
    differ = check_targets(t, raw, "synthetic set")
    # fed the reference's un-normalised targets, the statistics and the normalised set are the golden's bits
    t = np.ascontiguousarray(raw.copy())
    _, m, s = ctx.det_target_stats(t, off, K, 1e-14, True)
    assert same_bits(m.ravel(), g["syn_means"]) and same_bits(s.ravel(), g["syn_stds"])
    for i in range(len(ex)):
        assert same_bits(t[off[i]:off[i + 1]], g["syn%d_bbox_targets" % i]), i
    if differ == 0:                                  # the device's log gave NumPy's float32 everywhere: then the front door too
        assert same_bits(means, g["syn_means"]) and same_bits(stds, g["syn_stds"])
        assert all(same_bits(e["bbox_targets"], g["syn%d_bbox_targets" % i]) for i, e in enumerate(imdb.roidb))
    else:
        # one float32 step of a |dw| < 2 is at most 1.2e-7: a mean moves by no more than that; a variance by
        # 2 (|x| + |mean|) 1.2e-7 < 1e-6, a std (all > 0.05 here) by that over 2 std < 1e-5
        assert g["syn_stds"].reshape(K, 4)[1:][g["syn_stds"].reshape(K, 4)[1:] > 0].min() > 0.05
        assert np.abs(means - g["syn_means"]).max() <= 1.2e-7 and np.abs(stds - g["syn_stds"]).max() <= 1e-5
    # minibatches: sampling reads labels and max_overlaps only; targets compared through the golden's own values
    for e, i in zip(imdb.roidb, range(len(ex))):
        e["bbox_targets"] = g["syn%d_bbox_targets" % i].copy()
    for b in range(int(g["n_batches"])):
        inds = [int(i) for i in g["mb%d_inds" % b]]
        np.random.seed(int(g["mb%d_seed" % b]))
        blobs = get_minibatch([imdb.roidb[i] for i in inds], K, ctx)
        for k in ("rois", "labels", "bbox_targets", "bbox_loss_weights"):
            assert same_bits(np.asarray(blobs[k]).astype(np.float32), g["mb%d_%s" % (b, k)]), (b, k)
        st = np.random.get_state()
        assert np.array_equal(st[1], g["mb%d_state_keys" % b]) and int(st[2]) == int(g["mb%d_state_pos" % b][0]), b
        assert blobs["data"].shape == (len(inds), 3, 600, 800) and np.abs(blobs["data"]).max() > 1
    from detect.config import cfg
    from roi_data_layer.layer import RoIDataLayer
    np.random.seed(5)
    layer = RoIDataLayer(K, ctx=ctx)
    layer.set_roidb(imdb.roidb)
    blobs = layer.forward()
    assert all(v.dtype == np.float32 for v in blobs.values()) and blobs["data"].shape[0] == cfg.TRAIN.IMS_PER_BATCH
    assert blobs["rois"].shape[0] == blobs["labels"].shape[0] <= 128


# ---- one step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["small", "voc", "coco"])
def test_one_step(ctx, name, channels_last):
    import torch
    head, fmap, blobs = D.case(name)
    d = D.HEADS[name]
    print("%s head C=%d n6=%d n7=%d ncls=%d, R = %d, %s" % (name, d["C"], d["n6"], d["n7"], d["ncls"], d["R"],
                                                           "channels_last" if channels_last else "NCHW"))
    seed, it = 3, 0
    sol = make_solver(ctx, head)
    conv = torch.from_numpy(fmap).cuda()
    if channels_last:
        conv = conv.contiguous(memory_format=torch.channels_last)
    dmap = torch.empty_like(conv)
    losses, sumsq = sol.step(*step_args(conv, blobs), seed, it, dmap=dmap)
    pool, arg = D.roi_pool(fmap, blobs["rois"])
    assert np.array_equal(sol.fetch("pool5"), pool), "pool5"
    assert np.array_equal(sol.fetch("argmax"), arg), "argmax"
    masks = device_masks(sol, seed, it)
    ngates = []
    gates = device_gates(sol, head, pool, blobs, masks, ngates)
    for t, l, _ in D.LAYERS:                                          # ReLU + dropout: exact given the pre-activation
        pre, a, dp = sol.fetch("pre%d" % t), sol.fetch("a%d" % t), sol.fetch("d_pre%d" % t)
        relu = np.maximum(pre, np.float32(0))
        assert same_bits(a, np.where(masks[t] > 0, relu * np.float32(2), np.float32(0)).astype(np.float32)), "a%d" % t
        assert not dp[(pre <= 0) | (masks[t] == 0)].any()
    r64 = D.step(head, pool, blobs, masks, gates=gates)
    r32 = D.step(head, pool, blobs, masks, gates=gates, dtype=np.float32)
    rows, ok = [("gates that differ", float(sum(ngates)), 0.0, 0.0)], True
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
    rate, mom, wd = 0.001, 0.9, 0.0005
    mult = dict(lr_mult=D.LR_MULT, decay_mult=D.DECAY_MULT)
    zeros = {k: np.zeros_like(v) for k, v in head.items()}
    for rep, clip_at in ((0, 1e-3), (1, None)):                       # a clipped step, then an unclipped one on top of its history
        cs = D.clip_scale(sumsq, clip_at)
        if rep == 0:
            assert cs < 1.0
            p64, h64 = D.sgd(head, r64["grads"], zeros, rate, mom, wd, D.clip_scale(r64["sumsq"], clip_at), **mult)
            p32, h32 = D.sgd(head, r32["grads"], zeros, rate, mom, wd, D.clip_scale(r32["sumsq"], clip_at), dtype=np.float32, **mult)
        else:
            p64, h64 = D.sgd(p64, r64["grads"], h64, rate, mom, wd, 1.0, **mult)
            p32, h32 = D.sgd(p32, r32["grads"], h32, rate, mom, wd, 1.0, dtype=np.float32, **mult)
        sol.update(rate, mom, wd, cs)
        for k in D.KEYS:
            ok &= check("w_%s/%d" % (k, rep), sol.fetch("w_" + k), p64[k], p32[k], rows)
            ok &= check("h_%s/%d" % (k, rep), sol.fetch("h_" + k), h64[k], h32[k], rows)
    got = sol.read()
    assert all(np.array_equal(got[k], sol.fetch("w_" + k)) for k in D.KEYS)
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error: " + ", ".join(r[0] for r in rows[1:] if r[1] > r[3])


# ---- softmax edges ---------------------------------------------------------------------------------------------------------
def test_softmax_edges(ctx):
    """R = 5, ncls = 21: logits of +-80, a row of equal logits, labels 0 and ncls - 1.  The logits are put there through the
    bias and a zero weight, so the loss layer sees exactly them."""
    import torch
    from aznet_hip import ffi
    ncls, n = 21, 5
    head = D.filler_head(11, 4, 8, 8, ncls)
    head["Wc"][:] = 0
    rng = np.random.Generator(np.random.PCG64(5))
    logits = rng.standard_normal((n, ncls)).astype(np.float32)
    logits[0, :] = 80.0
    logits[0, 3] = -80.0
    logits[1, :] = -80.0
    logits[1, 20] = 80.0
    logits[2, :] = 1.25
    logits[3, 0] = 80.0
    # cls_score's weights are zero, so a row's logits are the bias: the five rows run one by one (R = 1 each) ...
    fmap = np.abs(np.random.RandomState(3).standard_normal((1, 4, 6, 8))).astype(np.float32) + 0.5
    conv = torch.from_numpy(fmap).cuda()
    rois = np.array([[0, 0, 0, 127, 95]] * n, np.float32)
    labels = np.array([3, ncls - 1, 7, 0, ncls - 1], np.float32)      # (row 0: p[label] underflows to 0: the FLT_MIN clamp)
    sol = make_solver(ctx, head, max_rois=8)
    sol.set_hyper(dropout_ratio=[0.0, 0.0])
    tgt = np.zeros((n, 4 * ncls), np.float32)
    ok = True
    for r in range(n):
        sol.load({"bc": logits[r]})
        losses, _ = sol.step(conv, rois[:1], labels[r:r + 1], tgt[:1], tgt[:1], 1, 0)
        x = sol.fetch("cls_score")
        assert same_bits(x, logits[r:r + 1]), "the bias alone must be the logit row"
        p, d = sol.fetch("cls_prob"), sol.fetch("d_cls_score")
        l64, d64, p64 = D.softmax_loss(x.astype(np.float64), labels[r:r + 1], 1.0)
        l32, d32, p32 = D.softmax_loss(x, labels[r:r + 1], np.float32(1.0))
        err = float(np.abs(p - p64).max())
        print("  row %d: label %d loss %.6g (float64 %.6g), max |p - p64| = %.3e" % (r, int(labels[r]), losses[0], l64, err))
        assert np.all(np.isfinite(p)) and np.all(np.isfinite(d)) and np.isfinite(losses[0])
        assert err <= 1e-6
        ok &= check("d_cls_score[%d]" % r, d, d64, d32)
        ok &= check("loss_cls[%d]" % r, [losses[0]], [l64], [l32])
    assert ok
    # ... and five rows at once (R = 5: the 1 / R of the loss and of d) with large logits through the weights
    head5 = D.filler_head(12, 4, 8, 8, ncls)
    head5["Wc"] *= 60.0                                               # large logits
    sol.load(head5)
    rois5 = np.array([[0, 0, 0, 127, 95], [0, 16, 16, 60, 60], [0, 40, 0, 127, 40], [0, 0, 50, 50, 95], [0, 70, 30, 120, 90]], np.float32)
    losses, _ = sol.step(conv, rois5, labels, tgt, tgt, 1, 0)
    x = sol.fetch("cls_score")
    print("  joint run: logits in [%.1f, %.1f]" % (x.min(), x.max()))
    l64, d64, p64 = D.softmax_loss(x.astype(np.float64), labels, float(n))
    l32, d32, p32 = D.softmax_loss(x, labels, np.float32(n))
    p = sol.fetch("cls_prob")
    err = float(np.abs(p - p64).max())
    print("  joint run: max |p - p64| = %.3e" % err)
    assert np.all(np.isfinite(p)) and err <= 1e-6
    assert check("d_cls_score", sol.fetch("d_cls_score"), d64, d32) & check("loss_cls", [losses[0]], [l64], [l32])
    # a label of ncls: AZ_ERR_INVALID and nothing enqueued (d conv5_3 keeps its fill, the saved tensors their bits)
    before = sol.fetch("cls_prob")
    dmap = torch.full_like(conv, 7.0)
    bad = labels.copy()
    bad[2] = ncls
    with pytest.raises(ffi.AzError) as e:
        sol.step(conv, rois5, bad, tgt, tgt, 1, 0, dmap=dmap)
    assert e.value.code == ffi.AZ_ERR_INVALID
    assert float(dmap.min()) == 7.0 and float(dmap.max()) == 7.0 and same_bits(sol.fetch("cls_prob"), before)
    for v in (-1.0, 0.5):
        bad[2] = v
        with pytest.raises(ffi.AzError):
            sol.step(conv, rois5, bad, tgt, tgt, 1, 0)
    sol.close()


def test_bad_arguments(ctx):
    import torch
    from aznet_hip import ffi
    with pytest.raises(ffi.AzError):
        ffi.AzDetSolver(ctx, 18, 8, 8, 21)                            # C not a multiple of 4
    with pytest.raises(ffi.AzError):
        ffi.AzDetSolver(ctx, 4, 8, 6, 21)                             # n7 not a multiple of 4
    for ncls in (1, 257):
        with pytest.raises(ffi.AzError):
            ffi.AzDetSolver(ctx, 4, 8, 8, ncls)
    head, fmap, blobs = D.case("voc")
    sol = make_solver(ctx, head, max_rois=36)
    conv = torch.from_numpy(fmap).cuda()
    with pytest.raises(ffi.AzError):
        sol.step(*step_args(conv, blobs), 1, 0)                       # 37 rows, max_rois 36
    with pytest.raises(ffi.AzError):
        sol.update(0.001, 0.9, 0.0005, 1.0)                           # no gradients yet
    with pytest.raises(ffi.AzError):
        sol.fetch("no_such_tensor")
    sol.close()


# ---- integer heads: every partial sum an integer below 2^24 -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["voc", "coco"])
def test_integer_heads_bit_for_bit(ctx, name):
    """Integer maps, weights and biases: whatever the order of a sum, each of its partial sums is an integer of magnitude at
    most sum |a| |w| + |b|; where that is below 2^24, float32 is exact and the device must give float64's bits."""
    import torch
    d = D.HEADS[name]
    rng = np.random.Generator(np.random.PCG64(41))
    C, n6, n7, ncls, n = d["C"], d["n6"], d["n7"], d["ncls"], d["R"]
    ints = lambda shape, lo, hi: rng.integers(lo, hi + 1, shape).astype(np.float32)
    head = {"W6": ints((n6, C * 49), -1, 1), "b6": ints(n6, -3, 3), "W7": ints((n7, n6), -1, 1), "b7": ints(n7, -3, 3),
            "Wc": ints((ncls, n7), -1, 1), "bc": ints(ncls, -3, 3), "Wb": ints((4 * ncls, n7), -1, 1), "bb": ints(4 * ncls, -3, 3)}
    fmap = ints((2, C, D.MAP_H, D.MAP_W), 0, 2)
    blobs = D.random_blobs(9, n, 2, D.MAP_H, D.MAP_W, ncls)
    pool, _ = D.roi_pool(fmap, blobs["rois"])
    r = D.step(head, pool, blobs, None, want_dpool=False)
    x = pool.astype(np.float64)
    for nm, wk, bk, nxt in (("fc6", "W6", "b6", "a6"), ("fc7", "W7", "b7", "a7"), ("cls_score", "Wc", "bc", None), ("bbox_pred", "Wb", "bb", None)):
        worst = float((np.abs(x) @ np.abs(head[wk]).T.astype(np.float64) + np.abs(head[bk])).max())
        print("  %s: largest possible |partial sum| %.0f (2^24 = %d)" % (nm, worst, 2 ** 24))
        assert worst < 2 ** 24
        if nxt is not None:
            x = r[nxt]
    assert np.abs(r["cls_score"]).max() > 100 and np.abs(r["bbox_pred"]).max() > 100
    sol = make_solver(ctx, head)
    sol.set_hyper(dropout_ratio=[0.0, 0.0])
    conv = torch.from_numpy(fmap).cuda()
    _, b = sol.forward_test(conv, blobs["rois"])
    assert same_bits(sol.fetch("cls_score"), r["cls_score"].astype(np.float32)), "cls_score of forward_test"
    assert same_bits(b, r["bbox_pred"].astype(np.float32)), "bbox_pred of forward_test"
    sol.step(*step_args(conv, blobs), 1, 0)
    assert same_bits(sol.fetch("cls_score"), r["cls_score"].astype(np.float32)), "cls_score of the step"
    assert same_bits(sol.fetch("bbox_pred"), r["bbox_pred"].astype(np.float32)), "bbox_pred of the step"
    sol.close()


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_three_steps_of_two_trainers_same_bits(ctx):
    import torch
    head, fmap, blobs = D.case("coco", seed=23)
    conv = torch.from_numpy(fmap).cuda()
    names = ["pool5", "argmax", "pre6", "pre7", "mask6", "mask7", "a6", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score",
             "d_bbox_pred", "d_pre6", "d_pre7", "d_pool5"] + [p + k for p in ("g_", "w_", "h_") for k in D.KEYS]
    runs = []
    for _ in range(2):
        sol = make_solver(ctx, head)
        dmap = torch.empty_like(conv)
        out = []
        for it in range(3):                                           # three steps: the history is part of the state
            losses, sq = sol.step(*step_args(conv, blobs), 9, it, dmap=dmap)
            sol.update(0.01, 0.9, 0.0005, D.clip_scale(sq, 0.5))
            out.append([losses.copy(), np.float64(sq), dmap.cpu().numpy()] + [sol.fetch(n) for n in names])
        runs.append(out)
        sol.close()
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a, b):
            assert np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8))
    assert not np.array_equal(runs[0][0][0], runs[0][2][0])           # (the steps do differ from one another)
    # the fillers: seeded, at train.prototxt's stds
    from aznet_hip import ffi
    w = [ffi.AzDetSolver(ctx, 16, 128, 64, 21, max_rois=8, seed=s) for s in (4, 4, 5)]
    p = [s.read() for s in w]
    assert all(np.array_equal(p[0][k], p[1][k]) for k in D.KEYS) and not np.array_equal(p[0]["W6"], p[2]["W6"])
    for k, std in (("W6", 5e-3), ("W7", 5e-3), ("Wc", 1e-2), ("Wb", 1e-3)):
        print("  filler %s: std %.4g (wanted %g)" % (k, p[0][k].std(), std))
        assert abs(p[0][k].std() / std - 1) < 0.1
    assert not any(p[0][k].any() for k in ("b6", "b7", "bc", "bb"))
    for s in w:
        s.close()


# ---- the front door ----------------------------------------------------------------------------------------------------------
def test_solver_wrapper_trajectory_and_round_trip(ctx, g, tmp_path, monkeypatch):
    """SolverWrapper on synthetic_375x500_8 (the golden's recorded proposals), width-reduced backbone frozen: 20 steps at the
    base_lr recorded in det_step_ref.TRAJ, every step's two losses against the float64 restatement; then the snapshot through
    det_head_from_layers / az_load_det_head against the trainer's own TEST-phase forward."""
    from aznet_hip import caffemodel as cm, ffi
    from detect.train_det import SolverWrapper
    from roi_data_layer import roidb as rdl
    T = D.TRAJ
    ffi.set_default_context(ctx)
    imdb, _, _ = DR.synthetic_roidb(rdl, g, tmp_path, monkeypatch)
    np.random.seed(T["np_seed"])
    sw = SolverWrapper(D.traj_solver_files(str(tmp_path)), imdb, str(tmp_path / "out"), backbone=D.traj_backbone("cuda:0"), ctx=ctx,
                       dims=dict(n6=T["n6"], n7=T["n7"]), seed=T["solver_seed"])
    assert sw.conv_train == [] and sw.num_classes == K
    start = sw.trainer.read()
    ref64, ref32 = D.RefTrajectory(start, np.float64, T["solver"]), D.RefTrajectory(start, np.float32, T["solver"])
    ok, tot = True, []
    for it in range(T["steps"]):
        before = sw.trainer.read()
        losses = sw.step()
        conv, blobs = sw.last_conv.cpu().numpy(), sw.last_blobs
        pool, _ = D.roi_pool(conv, blobs["rois"])
        print("step %d (%d rows)" % (it, pool.shape[0]))
        masks = device_masks(sw.trainer, T["solver_seed"], it)
        gates = device_gates(sw.trainer, before, pool, blobs, masks)
        r64, r32 = ref64.step(conv, blobs, T["solver_seed"], gates), ref32.step(conv, blobs, T["solver_seed"], gates)
        ok &= check("losses[%d]" % it, losses, r64["losses"], r32["losses"])
        tot.append(float(np.sum(losses)))
    assert ok, "a step's losses exceed 8 x the float32-CPU error"
    print("summed loss: first five %.4f, last five %.4f" % (sum(tot[:5]), sum(tot[-5:])))
    assert sum(tot[-5:]) < sum(tot[:5])
    # round trip
    path = sw.snapshot()
    assert os.path.basename(path) == "frcnn_small_iter_20.caffemodel"
    layers = cm.load_caffemodel(path)
    assert set(layers) >= set(["conv1_1", "conv5_3", "fc6", "fc7", "cls_score", "bbox_pred"])
    head = cm.det_head_from_layers(layers)
    conv0 = sw.last_conv[0:1].contiguous()
    rois = sw.last_blobs["rois"][sw.last_blobs["rois"][:, 0] == 0].copy()
    p_tr, b_tr = sw.trainer.forward_test(conv0, rois)
    from aznet_hip import synth
    ctx.load_head(synth.make_head(seed=1, **synth.SMALL_DIMS))       # (a context takes a map once it has an AZ head: C = 16 too)
    ctx.load_det_head(head)
    ctx.set_feature_map(conv0.cpu().numpy())
    p_inf, b_inf = ctx.det_forward(rois)
    # the yardstick: the float64 restatement on the trainer's weights, un-normalised as the snapshot is; the bound from its
    # float32 run
    now = sw.trainer.read()
    pool, _ = D.roi_pool(conv0.cpu().numpy(), rois)
    p64, b64 = D.forward_test(now, pool)
    p32, b32 = D.forward_test(now, pool, dtype=np.float32)
    un = lambda b: b.astype(np.float64) * sw.bbox_stds + sw.bbox_means
    ok = check("cls_prob (trainer)", p_tr, p64, p32) & check("cls_prob (az_det_forward)", p_inf, p64, p32)
    ok &= check("bbox_pred (trainer)", un(b_tr), un(b64), un(b32)) & check("bbox_pred (az_det_forward)", b_inf, un(b64), un(b32))
    assert ok
    assert np.array_equal(head["Wb"], (now["Wb"] * sw.bbox_stds[:, None]).astype(np.float32))
    bk = cm.backbone_from_layers(layers)
    assert all(np.array_equal(bk[l[0]][0], l[1].detach().cpu().numpy()) for l in sw.backbone.layers if l is not None)


def test_train_det_tool_then_test_det_net_loads_it():
    """The command of the issue in a fresh child process under its own time limit: no files present, an AZ-net makes the
    proposals, four steps, the snapshot; then HipFrcnnNet loads that snapshot the way tools/test_det_net.py --net does."""
    import shutil
    tools = os.path.join(REPO, "az-net_amd", "tools")
    exp = "train_det_tool_test_%d" % os.getpid()
    out_dir = os.path.join(REPO, "az-net_amd", "output", exp)
    try:
        out = subprocess.run([sys.executable, os.path.join(tools, "train_det_net.py"), "--net", "synthetic:8", "--imdb",
                              "synthetic_375x500_8", "--iters", "4", "--exp", exp], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:], out.stderr[-3000:])
        assert out.returncode == 0
        snap = os.path.join(out_dir, "synthetic_375x500_8", "vgg16_frcnn_iter_4.caffemodel")
        assert os.path.exists(snap) and "Iteration 0, loss" in out.stdout and "2000 proposals, evaluate" in out.stdout
        assert os.path.exists(os.path.join(out_dir, "synthetic_375x500_8", "vgg16_az_net_synthetic_div8", "proposals.pkl"))
        sys.path.insert(0, tools)
        try:
            import test_det_net
        finally:
            sys.path.remove(tools)
        net = test_det_net.load_frcnn_net(snap, 0)
        assert net.name == "vgg16_frcnn_iter_4" and net.ctx.det_dims["ncls"] == K and net.ctx.det_dims["n6"] == 4096 // 8
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
