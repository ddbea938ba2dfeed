"""GPU: training the skip-connection detector (csrc/az_skip_train.hip behind az_det_solver_*_skip) against the float64
restatement tests/skip_train_ref.py, whose hand-written backward tests/test_skip_train_host.py checks against autograd.

Tolerances are the project's own (tests/test_gpu_det_train.py): per tensor the error is max|got - ref64| / max|ref64|; the
bound is the same figure of the restatement run in float32 on the CPU, times 8, floor 1e-6 (train_step_ref.bound).  What is
exact is compared bit for bit: the arg-max cells, the pooled values (max is exact), `cat` against az_skip_pool, the gather on
integer gradients, integer fronts and heads, two runs from one state.  ReLU gates (relu_pool handled like fc6 / fc7): the
device's gates may differ from float64's only where |pre-activation_64| is within the forward bound, at most 1e-4 of the
elements; the device's gates are then given to the restatement.  Every figure is printed before it is asserted.

Sizes: SMALL = skip_ref.SMALL_CS (20, 36, 12: channel-quad counts 5, 9, 3) on maps of 24x32 / 12x16 / 6x8, Cout 12, n6 260,
n7 516; EDGE = Cs (68, 132, 60): sumC 260 (one k-step past 256), Cout 132 (one tile edge in N), N = 2 images, R = 130: 6370
GEMM rows (a partial last tile) and a split K for g_Wp; FULL Cs (256, 512, 512: 64 and 128 quads), pool only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import det_step_ref as D
import det_train_ref as DR
import skip_ref as S
import skip_train_ref as T

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g21_train_det.npz")
SKIP_YML = os.path.join(REPO, "tests", "golden", "voc_skip.yml")
K = 21
TEN = T.KEYS


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def check(name, got, r64, r32, rows=None):
    e_dev, e_cpu = T.rel_err(got, r64), T.rel_err(r32, r64)
    b = T.bound(e_cpu)
    print("  %-14s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (name, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    if rows is not None:
        rows.append((name, e_dev, e_cpu, b))
    return e_dev <= b


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def make_trainer(ctx, head, front, Cs, max_rois=256, seed=1):
    from aznet_hip import ffi
    n6, n7, ncls = head["W6"].shape[0], head["W7"].shape[0], head["Wc"].shape[0]
    sol = ffi.AzDetSolver(ctx, head["W6"].shape[1] // 49, n6, n7, ncls, max_rois=max_rois, seed=seed, head=head)
    if front is not None:
        sol.attach_skip(Cs, S.SCALES, gain=front["gain"], eps=front["eps"], seed=seed, front=front)
    return sol


def to_dev(maps, channels_last=False):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]
    return [t.contiguous(memory_format=torch.channels_last) for t in out] if channels_last else out


def skip_args(maps, blobs):
    return (maps, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"])


def tiny_head(Cout, ncls=K, seed=5):
    return D.filler_head(seed, Cout, 8, 8, ncls)


def map_variants(kind, Cs, N=1, seed=3):
    maps = T.make_batch_maps(seed, Cs, N)
    if kind == "plateau":                       # every window is one tie: the first cell must win
        for m in maps:
            m[:] = 1.5
    elif kind == "zero":
        for m in maps:
            m[:] = 0.0
    return maps


ROIS = np.vstack([S.hostile_rois(), S.random_rois(40)])


# ---- 1. arg-max and pooled bits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "plateau", "zero", "full"])
def test_argmax_and_pooled_bits(ctx, kind):
    from aznet_hip import ffi
    Cs = S.FULL_CS if kind == "full" else S.SMALL_CS
    rois = ROIS[[5, 7, 12]] if kind == "full" else ROIS
    maps = map_variants("normal" if kind == "full" else kind, Cs)
    Cout = 12
    head, front = tiny_head(Cout), T.make_front(4, Cs, Cout)
    raw, arg = T.pool_argmax(maps, rois)
    if kind == "normal":
        assert (raw == 0).mean() > 0.05 and (arg == -1).any()                  # ties among zeros and empty bins are in the set
    # what the inference front computes for the same rois and maps (az_skip_pool)
    from aznet_hip import synth
    ictx = ffi.AzContext(0, max_regions=512)
    try:
        ictx.load_head(synth.make_head(seed=3, C=Cout, n6=4, n71=4, n72=4))   # (a context takes maps once it has an AZ head)
        ictx.load_det_head(head)
        ictx.load_skip_front(dict(front, Cs=Cs, scales=S.SCALES))
        ictx.set_skip_maps(to_dev(maps))
        cat_inf = ictx.skip_pool(rois, normalise=True)
        raw_inf = ictx.skip_pool(rois, normalise=False)
    finally:
        ictx.close()
    assert same_bits(raw_inf, raw)
    sol = make_trainer(ctx, head, front, Cs, max_rois=64)
    for cl in (False, True):
        sol.forward_test_skip(to_dev(maps, cl), rois)
        got_arg, got_cat = sol.fetch("skip_argmax"), sol.fetch("cat")
        bad = int((got_arg != arg).sum())
        print("  %s %s: %d of %d arg-max cells differ; %d empty" % (kind, "nhwc" if cl else "nchw", bad, arg.size, int((arg == -1).sum())))
        assert got_arg.dtype == np.int32 and same_bits(got_arg, arg)
        assert same_bits(got_cat, cat_inf), "cat differs from az_skip_pool's bits"
        pooled, uarg, _ = ffi.skip_pool_bwd_unit(ctx, maps, S.SCALES, rois, channels_last=cl)
        assert same_bits(pooled, raw) and same_bits(uarg, arg)
    sol.close()


# ---- 2. the gather, bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "plateau", "zero"])
def test_gather_bit_for_bit(ctx, kind):
    from aznet_hip import ffi
    Cs = S.SMALL_CS
    maps = map_variants(kind, Cs, N=2)
    rois = ROIS.copy()
    rois[:, 0] = np.arange(rois.shape[0]) % 2                                   # the two images' rois interleaved
    raw, arg = T.pool_argmax(maps, rois)
    rng = np.random.Generator(np.random.PCG64(8))
    d_raw = rng.integers(-8, 9, raw.shape).astype(np.float32)                   # every sum exact in any order
    want = T.scatter(d_raw, arg, Cs, rois, [m.shape for m in maps])
    for cl in (False, True):
        _, uarg, dm = ffi.skip_pool_bwd_unit(ctx, maps, S.SCALES, rois, d_raw=d_raw, channels_last=cl)
        assert same_bits(uarg, arg)
        for i in range(3):
            print("  %s %s map %d: |d| max %.0f, %d cells hit" % (kind, "nhwc" if cl else "nchw", i, np.abs(want[i]).max(), int((want[i] != 0).sum())))
            assert same_bits(dm[i], want[i])
    # two rois only: the cells outside both are exactly 0; a source not asked for gives nothing
    two = np.array([[0, 33.0, 21.0, 64.0, 52.0], [1, 5.5, 6.5, 77.5, 41.5]], np.float32)
    raw2, arg2 = T.pool_argmax(maps, two)
    d2 = rng.integers(-8, 9, raw2.shape).astype(np.float32)
    want2 = T.scatter(d2, arg2, Cs, two, [m.shape for m in maps])
    _, _, dm2 = ffi.skip_pool_bwd_unit(ctx, maps, S.SCALES, two, d_raw=d2, want=[True, False, True])
    assert dm2[1] is None and same_bits(dm2[0], want2[0]) and same_bits(dm2[2], want2[2])
    assert not dm2[0][0, :, 20:, :].any() and not dm2[0][1, :, :, 24:].any() and not dm2[0][0, :, :, 20:].any()


# ---- 3. one step -----------------------------------------------------------------------------------------------------------------
def device_masks(sol, seed, it):
    from aznet_hip import ffi
    masks = {}
    for t, l, _ in D.LAYERS:
        m = sol.fetch("mask%d" % t)
        assert np.array_equal(m, ffi.dropout_mask(seed, it, l, m.size, ratio=0.5).reshape(m.shape)), "mask of layer %d" % t
        masks[t] = m
    return masks


def device_gates(sol, Rn):
    g = {t: sol.fetch("pre%d" % t) > 0 for t, _, _ in D.LAYERS}
    g["pool"] = T.unflatten_caffe(sol.fetch("pool5"), Rn) > 0
    return g


def check_gates(gates, r64, r32, count=None):
    for t, key in (("pool", "pre_pool"), (6, "pre6"), (7, "pre7")):
        pre64 = r64[key]
        fwd = T.bound(T.rel_err(r32[key], pre64)) * np.abs(pre64).max()
        diff = gates[t] != (pre64 > 0)
        print("  gates of %s: %d of %d differ from float64" % (key, int(diff.sum()), diff.size))
        assert np.all(np.abs(pre64[diff]) <= fwd), "a gate differs where the pre-activation is not within rounding of zero"
        assert diff.mean() <= 1e-4
        if count is not None:
            count.append(int(diff.sum()))


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["small", "edge"])
def test_one_step(ctx, name, channels_last):
    import torch
    head, front, maps, blobs = T.case(name)
    Cs = tuple(m.shape[1] for m in maps)
    Rn = blobs["rois"].shape[0]
    print("%s: Cs %s, Cout %d, N %d, R %d (%d rows), %s" % (name, Cs, front["Wp"].shape[0], maps[0].shape[0], Rn, Rn * 49,
                                                          "channels_last" if channels_last else "NCHW"))
    seed, it = 3, 0
    sol = make_trainer(ctx, head, front, Cs)
    dev = to_dev(maps, channels_last)
    dmaps = [torch.empty_like(m) for m in dev]
    losses, sumsq = sol.step_skip(*skip_args(dev, blobs), seed, it, dmaps=dmaps)
    pooled = T.pool_argmax(maps, blobs["rois"])
    assert same_bits(sol.fetch("skip_argmax"), pooled[1]), "skip_argmax"
    masks = device_masks(sol, seed, it)
    gates = device_gates(sol, Rn)
    r64 = T.step(head, front, maps, blobs, masks, gates=gates, pooled=pooled)
    r32 = T.step(head, front, maps, blobs, masks, gates=gates, dtype=np.float32, pooled=pooled)
    ngates = []
    check_gates(gates, r64, r32, ngates)
    rows, ok = [("gates that differ", float(sum(ngates)), 0.0, 0.0)], True
    for nm in ("cat", "pool5", "pre6", "a6", "pre7", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score", "d_bbox_pred", "d_pre7",
               "d_pre6", "d_pool5", "d_y", "d_cat", "d_raw"):
        ok &= check(nm, sol.fetch(nm).reshape(np.shape(r64[nm])), r64[nm], r32[nm], rows)
    fac = sol.fetch("skip_factor")
    assert fac.dtype == np.float64 and fac.shape == (Rn * 49, 3)
    for i in range(3):
        ok &= check("d map %d" % i, dmaps[i].cpu().numpy(), r64["dmaps"][i], r32["dmaps"][i], rows)
    ok &= check("losses", losses, r64["losses"], r32["losses"], rows)
    fetched = {k: sol.fetch("g_" + k) for k in TEN}
    for k in TEN:
        ok &= check("g_" + k, fetched[k], r64["grads"][k], r32["grads"][k], rows)
    total = float(sum(np.sum(v.astype(np.float64) ** 2) for v in fetched.values()))
    print("  sumsq %.17g, f64 sum over the ten fetched gradients %.17g" % (sumsq, total))
    assert abs(sumsq - total) <= 1e-12 * total
    rate, mom, wd = 0.001, 0.9, 0.0005
    start = dict(head, Wp=front["Wp"], bp=front["bp"])
    zeros = {k: np.zeros_like(v) for k, v in start.items()}
    for rep, clip_at in ((0, 1e-3), (1, None)):                       # a clipped step, then an unclipped one on top of its history
        cs = D.clip_scale(sumsq, clip_at)
        if rep == 0:
            assert cs < 1.0
            p64, h64 = T.sgd(start, r64["grads"], zeros, rate, mom, wd, D.clip_scale(r64["sumsq"], clip_at))
            p32, h32 = T.sgd(start, r32["grads"], zeros, rate, mom, wd, D.clip_scale(r32["sumsq"], clip_at), dtype=np.float32)
        else:
            p64, h64 = T.sgd(p64, r64["grads"], h64, rate, mom, wd, 1.0)
            p32, h32 = T.sgd(p32, r32["grads"], h32, rate, mom, wd, 1.0, dtype=np.float32)
        sol.update(rate, mom, wd, cs)
        for k in TEN:
            ok &= check("w_%s/%d" % (k, rep), sol.fetch("w_" + k), p64[k], p32[k], rows)
            ok &= check("h_%s/%d" % (k, rep), sol.fetch("h_" + k), h64[k], h32[k], rows)
    got = sol.read_skip()
    assert np.array_equal(got["Wp"], sol.fetch("w_Wp")) and np.array_equal(got["bp"], sol.fetch("w_bp"))
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error: " + ", ".join(r[0] for r in rows[1:] if r[1] > r[3])


# ---- 4. an integer front: every partial sum a whole number of 1 / R below 2^24 -------------------------------------------------
def test_integer_front_bit_for_bit(ctx):
    """gain 1, eps 0 and maps with ONE live channel per source (value 4 or 0): every normalised vector is a unit vector or
    zero, so `cat` holds 0 and 1 exactly.  Integer Wp / bp / W6 .. bb; cls_score's weights and bias zero, so cls_prob is 1 / 16
    (16 classes) and d_cls_score a multiple of 1 / (16 R); integer box targets, so SmoothL1's gradient is -1, 0 or 1 over R.
    With R = 64 every gradient is an integer over 1024 of magnitude far below 2^24: float32 is exact whatever the order of a
    sum, and the device must give float64's bits for cat, pool5, the scores, d_pool5, d_y, g_Wp, g_bp and d_cat."""
    import torch
    rng = np.random.Generator(np.random.PCG64(41))
    Cs, Cout, n6, n7, ncls, Rn, N = S.SMALL_CS, 12, 32, 32, 16, 64, 2
    ints = lambda shape, lo, hi: rng.integers(lo, hi + 1, shape).astype(np.float32)
    maps = []
    for C, (h, w) in zip(Cs, S.MAP_HW):
        m = np.zeros((N, C, h, w), np.float32)
        for n in range(N):
            m[n, int(rng.integers(0, C))] = 4.0 * (rng.random((h, w)) < 0.6)
        maps.append(m)
    front = {"Wp": ints((Cout, sum(Cs)), -2, 2), "bp": ints(Cout, -1, 2), "gain": 1.0, "eps": 0.0}
    head = {"W6": ints((n6, Cout * 49), -1, 1), "b6": ints(n6, -3, 3), "W7": ints((n7, n6), -1, 1), "b7": ints(n7, -3, 3),
            "Wc": np.zeros((ncls, n7), np.float32), "bc": np.zeros(ncls, np.float32), "Wb": ints((4 * ncls, n7), -1, 1),
            "bb": ints(4 * ncls, -3, 3)}
    blobs = T.make_blobs(9, Rn, N, ncls)
    blobs["bbox_targets"] = np.where(blobs["bbox_loss_weights"] > 0, ints(blobs["bbox_targets"].shape, -5, 5), 0).astype(np.float32)
    r = T.step(head, front, maps, blobs, None, ratios=(0.0, 0.0))
    assert set(np.unique(r["cat"])) <= {0.0, 1.0} and r["cat"].sum() > 100 and (r["pool5"] > 0).mean() > 0.1
    worst = {k: float(np.abs(np.asarray(v)).max()) * 16 * Rn for k, v in (("d_pool5", r["d_pool5"]), ("g_Wp", r["grads"]["Wp"]),
                                                                        ("g_bp", r["grads"]["bp"]), ("d_cat", r["d_cat"]))}
    worst["bbox_pred"] = float((np.abs(r["a7"]) @ np.abs(head["Wb"]).T.astype(np.float64) + np.abs(head["bb"])).max())
    worst["g_Wp"] = float((np.abs(r["d_y"]).T @ r["cat"]).max()) * 16 * Rn
    print("  largest |numerator| per tensor:", {k: int(v) for k, v in worst.items()}, "(2^24 = %d)" % 2 ** 24)
    assert max(worst.values()) < 2 ** 24 and np.abs(r["grads"]["Wp"]).max() > 0 and np.abs(r["d_cat"]).max() > 0
    sol = make_trainer(ctx, head, front, Cs, max_rois=Rn)
    sol.set_hyper(dropout_ratio=[0.0, 0.0])
    dev = to_dev(maps)
    _, b = sol.forward_test_skip(dev, blobs["rois"])
    assert same_bits(b, r["bbox_pred"].astype(np.float32)), "bbox_pred of forward_test_skip"
    dmaps = [torch.empty_like(m) for m in dev]
    sol.step_skip(*skip_args(dev, blobs), 1, 0, dmaps=dmaps)
    for nm in ("cat", "pool5", "cls_score", "bbox_pred", "cls_prob", "d_pool5", "d_y", "d_cat"):
        assert same_bits(sol.fetch(nm).reshape(np.shape(r[nm])), np.asarray(r[nm]).astype(np.float32)), nm
    assert same_bits(sol.fetch("g_Wp"), r["grads"]["Wp"].astype(np.float32)), "g_Wp"
    assert same_bits(sol.fetch("g_bp"), r["grads"]["bp"].astype(np.float32)), "g_bp"
    assert all(np.isfinite(d.cpu().numpy()).all() for d in dmaps)
    sol.close()


# ---- 5. determinism and isolation -------------------------------------------------------------------------------------------------
def test_determinism_and_isolation(ctx):
    import torch
    head, front, maps, blobs = T.case("edge", seed=23)
    Cs = tuple(m.shape[1] for m in maps)
    dev = to_dev(maps, True)
    names = ["cat", "skip_argmax", "skip_factor", "pool5", "d_y", "d_cat", "d_raw"] + [p + k for p in ("g_", "w_", "h_") for k in TEN]
    runs = []
    for _ in range(2):
        sol = make_trainer(ctx, head, front, Cs)
        dmaps = [torch.empty_like(m) for m in dev]
        out = []
        for it in range(3):                                           # three steps: the history is part of the state
            losses, sq = sol.step_skip(*skip_args(dev, blobs), 9, it, dmaps=dmaps)
            sol.update(0.01, 0.9, 0.0005, D.clip_scale(sq, 0.5))
            out.append([losses.copy(), np.float64(sq)] + [d.cpu().numpy() for d in dmaps] + [sol.fetch(n) for n in names])
        runs.append(out)
        sol.close()
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a, b):
            assert same_bits(np.atleast_1d(x), np.atleast_1d(y))
    assert not np.array_equal(runs[0][0][0], runs[0][2][0])           # (the steps do differ from one another)
    # without dmaps: the ten gradients (and the losses) have the bits of the run with them
    a, b = make_trainer(ctx, head, front, Cs), make_trainer(ctx, head, front, Cs)
    la, sa = a.step_skip(*skip_args(dev, blobs), 9, 0, dmaps=[torch.empty_like(m) for m in dev])
    lb, sb = b.step_skip(*skip_args(dev, blobs), 9, 0, dmaps=None)
    assert same_bits(la, lb) and sa == sb and all(same_bits(a.fetch("g_" + k), b.fetch("g_" + k)) for k in TEN)
    from aznet_hip import ffi
    for nm in ("d_cat", "d_raw"):                                     # not computed without a map gradient: refused, not stale
        assert a.fetch(nm).any()
        with pytest.raises(ffi.AzError) as e:
            b.fetch(nm)
        assert e.value.code == ffi.AZ_ERR_STATE
    b.close()
    # the plain step on a trainer with a front: the bits of a trainer without one
    plain = make_trainer(ctx, head, None, None)
    from aznet_hip import synth
    h5, w5 = S.MAP_HW[2]
    conv = torch.from_numpy(np.concatenate([synth.make_feature_map(s, T.EDGE["Cout"], h5, w5) for s in (51, 52)], axis=0)).cuda()
    outs = []
    for sol in (a, plain):
        dmap = torch.empty_like(conv)
        steps = []
        for it in range(2):
            l, sq = sol.step(conv, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"], 9, it, dmap=dmap)
            sol.update(0.01, 0.9, 0.0005, D.clip_scale(sq, 0.5))
            steps.append([l.copy(), np.float64(sq), dmap.cpu().numpy()] + [sol.fetch(p + k) for p in ("g_", "w_", "h_") for k in D.KEYS] +
                         [sol.fetch(n) for n in ("pool5", "argmax", "d_pool5", "cls_prob")])
        outs.append(steps)
    for x, y in zip(outs[0], outs[1]):
        for p, q in zip(x, y):
            assert same_bits(np.atleast_1d(p), np.atleast_1d(q))
    # ... and that update left conv_pool5 alone (the last gradients were the plain step's)
    assert same_bits(a.fetch("w_Wp"), front["Wp"]) and same_bits(a.fetch("w_bp"), front["bp"])
    a.close()
    plain.close()


# ---- 6. frozen conv_pool5, a source without a gradient ---------------------------------------------------------------------------
def test_frozen_front_and_null_dmap(ctx):
    import torch
    head, front, maps, blobs = T.case("small")
    Cs = tuple(m.shape[1] for m in maps)
    dev = to_dev(maps)
    sol = make_trainer(ctx, head, front, Cs)
    sol.set_skip_hyper(lr_mult=[0.0, 0.0])
    ref = make_trainer(ctx, head, front, Cs)
    full = [torch.full_like(m, 7.0) for m in dev]
    part = [torch.full_like(m, 7.0) for m in dev]
    for it in range(2):
        _, sq = sol.step_skip(*skip_args(dev, blobs), 2, it, dmaps=[part[0], None, part[2]])
        sol.update(0.01, 0.9, 0.0005, 1.0)
        ref.step_skip(*skip_args(dev, blobs), 2, it, dmaps=full)
        ref.update(0.01, 0.9, 0.0005, 1.0)
        if it == 0:
            assert same_bits(part[0].cpu().numpy(), full[0].cpu().numpy()) and same_bits(part[2].cpu().numpy(), full[2].cpu().numpy())
    assert float(part[1].min()) == 7.0 and float(part[1].max()) == 7.0, "the source without a gradient was written"
    assert same_bits(sol.fetch("w_Wp"), front["Wp"]) and same_bits(sol.fetch("w_bp"), front["bp"])
    assert not sol.fetch("h_Wp").any() and not sol.fetch("h_bp").any()
    assert not same_bits(ref.fetch("w_Wp"), front["Wp"]) and ref.fetch("h_bp").any()
    assert not same_bits(sol.fetch("w_W6"), head["W6"])                # (the head did train)
    sol.close()
    ref.close()


# ---- 7. bad arguments ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx):
    import torch
    from aznet_hip import ffi
    head, front, maps, blobs = T.case("small")
    Cs = tuple(m.shape[1] for m in maps)
    dev = to_dev(maps)
    bare = make_trainer(ctx, head, None, None)
    with pytest.raises(ffi.AzError) as e:                              # no front attached
        bare.step_skip(*skip_args(dev, blobs), 1, 0)
    assert e.value.code == ffi.AZ_ERR_STATE
    for bad_Cs, bad_sc in (((20, 36, 10), S.SCALES), ((20, 36, 12, 4), S.SCALES + (0.5,)), ((20, 36, 12), (0.25, 0.0, 0.0625)),
                           ((20, 36, 12), (0.25, 0.125))):
        with pytest.raises(ffi.AzError) as e:
            bare.attach_skip(bad_Cs, bad_sc)
        assert e.value.code == ffi.AZ_ERR_INVALID
    with pytest.raises(ffi.AzError):
        bare.attach_skip(Cs, S.SCALES, gain=float("inf"))
    with pytest.raises(ffi.AzError) as e:                              # a refused attach left no front behind
        bare.step_skip(*skip_args(dev, blobs), 1, 0)
    assert e.value.code == ffi.AZ_ERR_STATE
    bare.close()
    sol = make_trainer(ctx, head, front, Cs)
    with pytest.raises(ffi.AzError) as e:
        sol.attach_skip(Cs, S.SCALES)                                  # one front per trainer
    assert e.value.code == ffi.AZ_ERR_STATE
    with pytest.raises(ffi.AzError) as e:
        sol.update(0.001, 0.9, 0.0005, 1.0)                            # no gradients yet
    assert e.value.code == ffi.AZ_ERR_STATE
    dmaps = [torch.full_like(m, 7.0) for m in dev]
    good = sol.step_skip(*skip_args(dev, blobs), 1, 0, dmaps=[torch.empty_like(m) for m in dev])
    keep = {n: sol.fetch(n) for n in ("cat", "cls_prob", "g_Wp", "g_W6")}

    def refused(code, maps_, blobs_, dm=dmaps):
        with pytest.raises(ffi.AzError) as e:
            sol.step_skip(*skip_args(maps_, blobs_), 1, 0, dmaps=dm)
        assert e.value.code == code, e.value
        assert all(float(d.min()) == 7.0 and float(d.max()) == 7.0 for d in dmaps), "something was enqueued"
        assert all(same_bits(sol.fetch(n), v) for n, v in keep.items())

    refused(ffi.AZ_ERR_INVALID, dev[1:], blobs, dmaps[1:])                                      # another n_src
    other = [dev[0], torch.zeros((1, 40, 12, 16), device="cuda"), dev[2]]
    refused(ffi.AZ_ERR_INVALID, other, blobs, [dmaps[0], torch.full_like(other[1], 7.0), dmaps[2]])   # other channel counts
    b2 = dict(blobs, rois=blobs["rois"].copy())
    b2["rois"][3, 0] = 1                                                                        # an image >= N
    refused(ffi.AZ_ERR_INVALID, dev, b2)
    b3 = dict(blobs, labels=blobs["labels"].copy())
    b3["labels"][0] = K
    refused(ffi.AZ_ERR_INVALID, dev, b3)
    big = dict(blobs, rois=np.repeat(blobs["rois"], 5, axis=0)[:257])                           # R > max_rois
    with pytest.raises(ffi.AzError):
        sol.step_skip(dev, big["rois"], np.zeros(257), np.zeros((257, 4 * K)), np.zeros((257, 4 * K)), 1, 0)
    # a null map, through the C entry itself
    n, Cs_a, ptrs, Hs, Ws, N, cl, _ = sol._maps(dev)
    ptrs[1] = None
    f, ci = ctypes.c_float, ctypes.c_int
    rois = np.ascontiguousarray(blobs["rois"], np.float32)
    lab, bt, bw = (np.ascontiguousarray(blobs[k], np.float32) for k in ("labels", "bbox_targets", "bbox_loss_weights"))
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    rc = sol.L.az_det_solver_step_skip(sol.h, n, P(Cs_a, ci), ptrs, P(Hs, ci), P(Ws, ci), N, cl, P(rois, f), rois.shape[0], P(lab, f),
                                       P(bt, f), P(bw, f), 1, 0, None, None, None)
    assert rc == ffi.AZ_ERR_INVALID and all(same_bits(sol.fetch(n_), v) for n_, v in keep.items())
    with pytest.raises(ffi.AzError):
        sol.forward_test_skip(dev[1:], blobs["rois"])
    # a good step afterwards: the usual bits
    again = sol.step_skip(*skip_args(dev, blobs), 1, 0, dmaps=[torch.empty_like(m) for m in dev])
    assert same_bits(again[0], good[0]) and again[1] == good[1] and all(same_bits(sol.fetch(n_), v) for n_, v in keep.items())
    sol.close()


# ---- 8. the filler ----------------------------------------------------------------------------------------------------------------
def test_xavier_filler(ctx):
    from aznet_hip import ffi
    d = T.EDGE
    sumC = sum(d["Cs"])
    sols = [ffi.AzDetSolver(ctx, d["Cout"], 8, 8, K, max_rois=8, seed=1) for _ in range(3)]
    for s, seed in zip(sols, (4, 4, 5)):
        s.attach_skip(d["Cs"], S.SCALES, seed=seed)
    p = [s.read_skip() for s in sols]
    Wp = p[0]["Wp"]
    assert Wp.shape == (d["Cout"], sumC) and Wp.size == 34320
    a = np.sqrt(3.0 / sumC)
    var = float(np.mean(Wp.astype(np.float64) ** 2))
    print("  xavier: |Wp| max %.6f (bound %.6f), mean %.2e, variance x sumC %.4f" % (np.abs(Wp).max(), a, Wp.mean(), var * sumC))
    assert np.abs(Wp).max() <= np.float32(a) and not p[0]["bp"].any()
    assert abs(var * sumC - 1.0) <= 0.05 and abs(float(Wp.mean())) < 0.01 * a
    assert np.array_equal(Wp, p[1]["Wp"]) and not np.array_equal(Wp, p[2]["Wp"])
    assert not sols[0].fetch("h_Wp").any() and not sols[0].fetch("g_bp").any()
    for s in sols:
        s.close()


# ---- 9. the front door ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def skip_cfg():
    import copy
    from detect import config as C
    saved = copy.deepcopy(dict(C.cfg))
    C.cfg_from_file(SKIP_YML)
    yield C
    S.restore_tree(C.cfg, saved)


def test_solver_wrapper_trajectory_and_round_trip(ctx, skip_cfg, tmp_path, monkeypatch):
    """SolverWrapper under the skip configuration on synthetic_375x500_8 (the golden's recorded proposals), width-reduced
    backbone frozen: 20 steps at the base_lr recorded in skip_train_ref.TRAJ, every step's two losses against the float64
    restatement; then the snapshot through det_head_from_layers / az_load_skip_front against the trainer's own TEST-phase
    forward and the restatement; then three steps with conv3_1 .. conv5_3 trainable."""
    import torch
    from aznet_hip import caffemodel as cm, ffi, synth
    from detect.train_det import SolverWrapper
    from roi_data_layer import roidb as rdl
    g = np.load(GOLD)
    tr = T.TRAJ
    ffi.set_default_context(ctx)
    imdb, _, _ = DR.synthetic_roidb(rdl, g, tmp_path, monkeypatch)
    np.random.seed(tr["np_seed"])
    sw = SolverWrapper(T.traj_solver_files(str(tmp_path)), imdb, str(tmp_path / "out"), backbone=T.traj_backbone("cuda:0"), ctx=ctx,
                       dims=dict(n6=tr["n6"], n7=tr["n7"]), seed=tr["solver_seed"])
    assert sw.conv_train == [] and sw.num_classes == K and sw.skip["sources"] == list(S.NAMES) and sw.skip["gain"] == 1000.0
    assert sw.trainer.skip["scales"] == S.SCALES and sw.trainer.skip["eps"] == 1e-10
    start, front0 = sw.trainer.read(), dict(sw.trainer.read_skip(), gain=1000.0, eps=1e-10)
    assert np.abs(front0["Wp"]).max() <= np.float32(np.sqrt(3.0 / front0["Wp"].shape[1])) and not front0["bp"].any()
    ref64, ref32 = T.RefTrajectory(start, front0, np.float64, tr["solver"]), T.RefTrajectory(start, front0, np.float32, tr["solver"])
    ok, tot = True, []
    for it in range(tr["steps"]):
        losses = sw.step()
        maps, blobs = [m.cpu().numpy() for m in sw.last_maps], sw.last_blobs
        Rn = blobs["rois"].shape[0]
        print("step %d (%d rows)" % (it, Rn))
        pooled = T.pool_argmax(maps, blobs["rois"])
        device_masks(sw.trainer, tr["solver_seed"], it)
        gates = device_gates(sw.trainer, Rn)
        r64, r32 = ref64.step(maps, blobs, tr["solver_seed"], gates, pooled), ref32.step(maps, blobs, tr["solver_seed"], gates, pooled)
        check_gates(gates, r64, r32)
        ok &= check("losses[%d]" % it, losses, r64["losses"], r32["losses"])
        tot.append(float(np.sum(losses)))
    assert ok, "a step's losses exceed 8 x the float32-CPU error"
    print("summed loss: first five %.4f, last five %.4f" % (sum(tot[:5]), sum(tot[-5:])))
    assert sum(tot[-5:]) < sum(tot[:5])
    # round trip
    path = sw.snapshot()
    assert os.path.basename(path) == "frcnn_skip_small_iter_20.caffemodel"
    layers = cm.load_caffemodel(path)
    assert set(layers) >= set(["conv1_1", "conv5_3", "conv_pool5", "fc6", "fc7", "cls_score", "bbox_pred"])
    now, fnow = sw.trainer.read(), sw.trainer.read_skip()
    assert layers["conv_pool5"][0].shape == fnow["Wp"].shape + (1, 1)
    head = cm.det_head_from_layers(layers)
    assert "skip_front" in head and np.array_equal(head["skip_front"]["Wp"], fnow["Wp"]) and head["skip_front"]["Cs"] == sw.trainer.skip["Cs"]
    maps0 = [m[0:1].contiguous() for m in sw.last_maps]
    rois = sw.last_blobs["rois"][sw.last_blobs["rois"][:, 0] == 0].copy()
    p_tr, b_tr = sw.trainer.forward_test_skip(maps0, rois)
    ictx = ffi.AzContext(0, max_regions=512)
    try:
        ictx.load_head(synth.make_head(seed=3, C=head["W6"].shape[1] // 49, n6=4, n71=4, n72=4))
        ictx.load_det_head({k: v for k, v in head.items() if k != "skip_front"})
        ictx.load_skip_front(head["skip_front"])
        ictx.set_skip_maps(maps0)
        p_inf, b_inf = ictx.det_forward_skip(rois)
    finally:
        ictx.close()
    fr = dict(fnow, gain=1000.0, eps=1e-10)
    np_maps = [m.cpu().numpy() for m in maps0]
    p64, b64 = T.forward_test(now, fr, np_maps, rois)
    p32, b32 = T.forward_test(now, fr, np_maps, rois, dtype=np.float32)
    un = lambda b: b.astype(np.float64) * sw.bbox_stds + sw.bbox_means
    ok = check("cls_prob (trainer)", p_tr, p64, p32) & check("cls_prob (az_det_forward_skip)", p_inf, p64, p32)
    ok &= check("bbox_pred (trainer)", un(b_tr), un(b64), un(b32)) & check("bbox_pred (az_det_forward_skip)", b_inf, un(b64), un(b32))
    assert ok
    # three steps with conv3_1 .. conv5_3 trainable: all three taps get gradients; the convolutions' update is
    # ffi.sgd_update_numpy on torch's gradients to 0 ulp
    np.random.seed(tr["np_seed"])
    sw2 = SolverWrapper(T.traj_solver_files(str(tmp_path), frozen_all=False), imdb, str(tmp_path / "out2"),
                        backbone=T.traj_backbone("cuda:0"), ctx=ctx, dims=dict(n6=tr["n6"], n7=tr["n7"]), seed=tr["solver_seed"])
    assert [c[0] for c in sw2.conv_train] == list(sw2_names())
    sp = sw2.solver_param
    for it in range(3):
        before = {c[0]: (c[1].detach().clone(), c[2].detach().clone(), c[3].clone(), c[4].clone()) for c in sw2.conv_train}
        sw2.step()
        assert all(d is not None and float(d.abs().max()) > 0 for d in sw2.last_dmaps), "a tap got no gradient"
        for name, w, b, hw, hb, lr, dc in sw2.conv_train:
            for p, h, q, (p0, h0) in ((w, hw, 0, (before[name][0], before[name][2])), (b, hb, 1, (before[name][1], before[name][3]))):
                wn, hn = ffi.sgd_update_numpy(p0.cpu().numpy(), p.grad.cpu().numpy(), h0.cpu().numpy(), sw2.last_rate * lr[q], sp["momentum"],
                                              sp["weight_decay"] * dc[q], sw2.last_clip)
                assert same_bits(p.detach().cpu().numpy(), wn) and same_bits(h.cpu().numpy(), hn), (name, q, it)
    assert np.isfinite(np.asarray(sw2.losses)).all()


def sw2_names():
    from detect import prototxt as P
    return P.CONV_LAYERS[4:]


# ---- 10. the tool -----------------------------------------------------------------------------------------------------------------------
def test_train_det_tool_under_the_skip_cfg_then_test_det_net_loads_it():
    """The command of the issue in a fresh child process under its own time limit; then HipFrcnnNet loads the snapshot, front
    attached, the way tools/test_det_net.py --net does under the skip --cfg."""
    import shutil
    tools = os.path.join(REPO, "az-net_amd", "tools")
    exp = "train_det_skip_tool_test_%d" % os.getpid()
    out_dir = os.path.join(REPO, "az-net_amd", "output", exp)
    try:
        out = subprocess.run([sys.executable, os.path.join(tools, "train_det_net.py"), "--net", "synthetic:8", "--imdb",
                              "synthetic_375x500_8", "--iters", "4", "--cfg", SKIP_YML, "--exp", exp], capture_output=True, text=True,
                             timeout=600)
        print(out.stdout[-3000:], out.stderr[-3000:])
        assert out.returncode == 0
        snap = os.path.join(out_dir, "synthetic_375x500_8", "vgg16_fast_rcnn_skip_iter_4.caffemodel")
        assert os.path.exists(snap) and "Iteration 0, loss" in out.stdout
        assert os.path.exists(os.path.join(out_dir, "synthetic_375x500_8", "train_det_skip.prototxt"))
        sys.path.insert(0, tools)
        try:
            import test_det_net
        finally:
            sys.path.remove(tools)
        net = test_det_net.load_frcnn_net(snap, 0)
        assert net.name == "vgg16_fast_rcnn_skip_iter_4" and net.ctx.det_dims["ncls"] == K and net.ctx.det_dims["n6"] == 4096 // 8
        assert net.skip_front is not None and tuple(net.skip_names) == S.NAMES and net.skip_front["Wp"].shape == (512 // 8, 1280 // 8)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
