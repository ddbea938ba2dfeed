"""GPU: the AZ-net trainer (csrc/az_solver.hip) off its defaults, against tests/train_step_ref.py; the cases are built in
tests/solver_edges_ref.py and their conditions asserted without a GPU in tests/test_solver_edges_host.py.

1. Hyper-parameters: dropout ratios that are no float32 (0.3, 0.6, 0.8: the mask's threshold is the float32 ratio's), that
   are 0 (no mask is drawn, the stale buffer is not read) or give a scale that is no power of two; lr_mult 0 on a head layer
   (not a bit moves), 0.1 and 3; decay on a bias and none on a weight; the same through SolverWrapper from an edited
   train net.
2. RoIPool and its backward gather on 43 hostile rois (empty bins, off-map / degenerate / oversized rois, bins narrower
   than a cell, unsorted batch indices) on a plateau map, an all-negative map and a normal one: bit for bit.
3. The GEMM kernel at tile and slab edges of M, N and K, integer operands: bit for bit.
4. SmoothL1 with weights 0 / 0.5 / 1 / 2 and w (x - t) on 0, +-0.5, +-1 and the floats next to +-1: the gradient bit for bit.

Tolerances: the trainer's rule (tests/test_gpu_train_step.py): 8 x the float32-CPU restatement's own error against float64,
floor 1e-6, gates as device_gates allows.  Every figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest

import solver_edges_ref as E
import train_step_ref as R
from test_gpu_train_step import LAYERS, _wrapper, check, device_gates, device_masks, run_and_compare, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def worst(title, rows):
    """The line DESIGN.md's table is written from: the largest device / float32-CPU error ratio (where the float32-CPU error
    is above float32's epsilon; below it the ratio is noise) and the number of ReLU gates that differed from float64."""
    r = [(e_dev / e_cpu, name) for name, e_dev, e_cpu, b in rows[1:] if e_cpu > 6e-8]
    top = max(r) if r else (0.0, "-")
    print("%s: worst device / float32-CPU error ratio %.2f (%s), largest device error %.3e, %d gates differ"
          % (title, top[0], top[1], max(x[1] for x in rows[1:]), int(rows[0][1])))


# ---- 1. hyper-parameters ------------------------------------------------------------------------------------------------
def test_mask_threshold_is_the_float32_ratios(ctx):
    """The device thresholds the generator's 24 bits at (unsigned)((double)(float)ratio * 2^24): 5033165 for 0.3, where the
    double 0.3 gives 5033164.  Element (21, 78) of int6's mask at seed 276 has exactly the word 5033164."""
    import torch
    from aznet_hip import ffi
    M = E.MASK_CASE
    head, fmap, blobs = R.small_case(R=M["rows"])
    sol = ffi.AzSolver(ctx, 16, 128, 64, 32, max_rois=M["rows"], head=head)
    sol.set_hyper(dropout_ratio=M["ratios"])
    sol.step(torch.from_numpy(fmap).cuda(), blobs["rois"], blobs["adj_labels"], blobs["adj_targets"], blobs["adj_loss_weights"],
             blobs["zoom_labels"], M["seed"], M["iteration"])
    got = {t: sol.fetch("mask%d" % t) for t, _, _ in LAYERS}
    sol.close()
    print("mask6[%d, %d] = %d" % (M["row"], M["unit"], got[6][M["row"], M["unit"]]))
    assert got[6][M["row"], M["unit"]] == 0
    for t, l, _ in LAYERS:
        want = ffi.dropout_mask(M["seed"], M["iteration"], l, got[t].size, ratio=M["ratios"][l]).reshape(got[t].shape)
        print("mask%d at ratio %g: %d of %d elements differ from ffi.dropout_mask, kept %.4f"
              % (t, M["ratios"][l], int(np.sum(got[t] != want)), want.size, got[t].mean()))
        assert np.array_equal(got[t], want)


@pytest.mark.parametrize("rows", E.HYPER_ROWS)
@pytest.mark.parametrize("ratios", E.RATIO_SETS, ids=lambda r: "-".join("%g" % x for x in r))
def test_one_step_with_other_hyper_parameters(ctx, ratios, rows):
    head, fmap, blobs = R.small_case(R=rows)
    lr, dc = E.hyper_multipliers()
    print("reduced head, R = %d, dropout %s, int7_1 frozen, lr_mult Was 0.1 / bz 3, decay_mult b6 1 / W72 0" % (rows, ratios))
    out = run_and_compare(ctx, head, fmap, blobs, seed=3, it=0, channels_last=(rows == 130), ratios=ratios, lr_mult=lr, decay_mult=dc)
    worst("hyper-parameters %s R %d" % (ratios, rows), out)


def test_other_hyper_parameters_through_solver_wrapper(ctx, tmp_path):
    """Three steps of SolverWrapper on a train net with dropout 0.3 on int6, no Dropout block on int7_1, 0.6 on int7_2 and
    int7_1's lr_mult 0 0, beside RefTrajectory with the same ratios and multipliers."""
    T, F = R.TRAJ, E.FRONT_DOOR
    sw = _wrapper(ctx, tmp_path, True, E.front_door_rows)
    start = sw.trainer.read()
    lr, dc = E.front_door_multipliers()
    ref64, ref32 = (R.RefTrajectory(start, dt, ratios=F["ratios"], lr_mult=lr, decay_mult=dc) for dt in (np.float64, np.float32))
    ok, ngates = True, []
    for it in range(F["steps"]):
        before = sw.trainer.read()
        losses = sw.step()
        conv, blobs = sw.last_conv.cpu().numpy(), sw.last_blobs
        pool, _ = R.roi_pool(conv, blobs["rois"])
        print("step %d" % it)
        masks = device_masks(sw.trainer, T["solver_seed"], it, pool.shape[0], F["ratios"])
        assert sorted(masks) == [6, 72]
        gates = device_gates(sw.trainer, before, pool, blobs, masks, F["ratios"], ngates)
        pre, a = sw.trainer.fetch("pre71"), sw.trainer.fetch("a71")
        assert same_bits(a, np.maximum(pre, np.float32(0)))                 # no Dropout block: a71 = relu(pre71)
        r64, r32 = ref64.step(conv, blobs, T["solver_seed"], gates), ref32.step(conv, blobs, T["solver_seed"], gates)
        ok &= check("losses[%d]" % it, losses, r64["losses"], r32["losses"])
    print("front door: %d gates differ over %d steps" % (sum(ngates), F["steps"]))
    assert ok, "a step's losses exceed 8 x the float32-CPU error"
    end = sw.trainer.read()
    for k in R.KEYS:
        moved = not same_bits(end[k], start[k])
        print("  %s %s" % (k, "moved" if moved else "unchanged"))
        assert moved == (k not in ("W71", "b71")), k


# ---- 2. RoIPool forward and backward on hostile rois ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def roi_refs():
    """Per map: (pool5, argmax) of the restatement, computed once."""
    rois = E.hostile_rois()
    return {kind: R.roi_pool(E.hostile_map(kind), rois) for kind in E.MAP_KINDS}


def _roi_step(ctx, kind, channels_last, reverse=False, ratios=None):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs = E.roi_case(kind, reverse)
    C, n6, n71, n72 = E.ROI_DIMS
    sol = ffi.AzSolver(ctx, C, n6, n71, n72, max_rois=43, head=head)
    if ratios is not None:
        sol.set_hyper(dropout_ratio=ratios)
    conv = torch.from_numpy(fmap).cuda()
    if channels_last:
        conv = conv.contiguous(memory_format=torch.channels_last)
    dmap = torch.full_like(conv, 7.0)
    sol.step(conv, blobs["rois"], blobs["adj_labels"], blobs["adj_targets"], blobs["adj_loss_weights"], blobs["zoom_labels"], 3, 0, dmap=dmap)
    out = {k: sol.fetch(k) for k in ("pool5", "argmax", "d_pool5")}
    sol.close()
    out["d_conv5_3"] = dmap.cpu().numpy()
    return head, fmap, blobs, out


@pytest.mark.parametrize("channels_last", [False, True], ids=["NCHW", "channels_last"])
@pytest.mark.parametrize("kind", E.MAP_KINDS)
def test_roi_pool_and_backward_on_hostile_rois(ctx, roi_refs, kind, channels_last):
    head, fmap, blobs, got = _roi_step(ctx, kind, channels_last)
    rois = blobs["rois"]
    pool, arg = roi_refs[kind]
    print("%s map: pool5 differs in %d, argmax in %d of %d" % (kind, int(np.sum(got["pool5"] != pool)), int(np.sum(got["argmax"] != arg)), arg.size))
    assert same_bits(got["argmax"], arg) and same_bits(got["pool5"], pool)
    ctx.load_head(head)
    for i in range(fmap.shape[0]):                                    # the inference kernel, image by image
        rows = np.where(rois[:, 0] == i)[0]
        assert rows.size > 0
        ctx.set_feature_map(fmap[i:i + 1])
        one = rois[rows].copy()
        one[:, 0] = 0
        assert np.array_equal(ctx.roi_pool(one), pool[rows]), "az_roi_pool, image %d" % i
    # backward: the gather adds rows ascending, bins ascending -- np.add.at's order per (channel, cell)
    assert np.abs(got["d_pool5"]).max() > 0
    want = R.roi_pool_backward(got["d_pool5"], arg, rois, fmap.shape)
    dmap = got["d_conv5_3"]
    print("d_conv5_3: %d of %d cells differ, max |diff| %.3e" % (int(np.sum(dmap != want)), want.size, float(np.abs(dmap - want).max())))
    assert same_bits(dmap, want)
    outside = ~E.window_cover(rois, fmap.shape)
    print("cells outside every window: %d" % int(outside.sum()))
    assert outside.any() and not dmap.transpose(0, 2, 3, 1)[outside].any()


def test_roi_pool_backward_does_not_need_sorted_rows(ctx, roi_refs):
    """The same 43 rows in reversed order (blobs permuted to match), dropout off so that a row's units do not depend on its
    position: d_conv5_3 is the same sum in another order."""
    kind = "plateau"
    head, fmap, blobs, a = _roi_step(ctx, kind, False, ratios=(0.0, 0.0, 0.0))
    _, _, rblobs, b = _roi_step(ctx, kind, False, reverse=True, ratios=(0.0, 0.0, 0.0))
    pool, arg = roi_refs[kind]
    assert same_bits(b["pool5"], pool[::-1]) and same_bits(b["argmax"], arg[::-1])
    r64, r32 = (R.step(head, pool, blobs, None, dtype=dt) for dt in (np.float64, np.float32))
    d64, d32 = (R.roi_pool_backward(r["d_pool5"], arg, blobs["rois"], fmap.shape) for r in (r64, r32))
    bound = R.bound(R.rel_err(d32, d64))
    diff = R.rel_err(b["d_conv5_3"], a["d_conv5_3"])
    print("reversed rows: d_conv5_3 moves by %.3e of its largest entry (bound %.3e)" % (diff, bound))
    assert diff <= bound


# ---- 3. GEMM unit sweep ---------------------------------------------------------------------------------------------------
def _exact_case(ctx, form, M, N, K, rng, skipped):
    from aznet_hip import ffi
    a, b, want = E.gemm_operands(form, M, N, K, E.integer_draw(rng))
    if E.gemm_abs_sum(form, a, b) >= 2.0 ** 24:
        skipped.append((form, M, N, K))
        return
    got = ffi.gemm_unit(ctx, form, a, b)
    bad = int(np.sum(got != want.astype(np.float32))) if got.shape == want.shape else -1
    if bad:
        print("  form %d  %d x %d x %d: %d outputs differ" % (form, M, N, K, bad))
    assert got.shape == want.shape and np.array_equal(got, want.astype(np.float32)), (form, M, N, K)


@pytest.mark.parametrize("M,N", E.GEMM_MN)
def test_gemm_integer_exact_at_tile_and_slab_edges(ctx, M, N):
    rng = np.random.Generator(np.random.PCG64(1000 * M + N))
    skipped = []
    for K in E.GEMM_K:
        for form in (0, 1, 2):
            _exact_case(ctx, form, M, N, K, rng, skipped)
    print("%d x %d: K in %s, forms 0 1 2 bit for bit; skipped %s" % (M, N, E.GEMM_K, skipped))
    assert not skipped


def test_gemm_integer_exact_past_256_tiles(ctx):
    M, N, K = E.GEMM_BIG
    rng = np.random.Generator(np.random.PCG64(5))
    skipped = []
    for form in (0, 1):
        _exact_case(ctx, form, M, N, K, rng, skipped)
    assert not skipped


def test_gemm_random_operands_at_the_edges(ctx):
    from aznet_hip import ffi
    M, N, K = E.GEMM_RANDOM
    rng = np.random.Generator(np.random.PCG64(6))
    ok, rows = True, [("", 0.0, 0.0, 0.0)]
    for form in (0, 1, 2):
        a, b, want = E.gemm_operands(form, M, N, K, lambda s: rng.standard_normal(s).astype(np.float32))
        cpu = {0: lambda: a @ b.T, 1: lambda: a @ b, 2: lambda: a.T @ b}[form]()
        ok &= check("form %d %dx%dx%d" % (form, M, N, K), ffi.gemm_unit(ctx, form, a, b), want, cpu, rows)
    worst("GEMM, random operands", rows)
    assert ok


# ---- 4. SmoothL1 with weights that are not 0 / 1 -------------------------------------------------------------------------------
def test_smooth_l1_with_other_weights(ctx):
    import torch
    from aznet_hip import ffi
    head, fmap, blobs, x = E.loss_case()
    n = blobs["rois"].shape[0]
    sol = ffi.AzSolver(ctx, 16, 128, 64, 32, max_rois=64, head=head)
    losses, _ = sol.step(torch.from_numpy(fmap).cuda(), blobs["rois"], blobs["adj_labels"], blobs["adj_targets"],
                         blobs["adj_loss_weights"], blobs["zoom_labels"], 5, 2)
    s_ab, d_ab = sol.fetch("adj_bbox"), sol.fetch("d_adj_bbox")
    sol.close()
    assert same_bits(s_ab, np.broadcast_to(x, s_ab.shape))            # Wab = 0: adj_bbox is its bias
    args = (s_ab, blobs["adj_targets"], blobs["adj_loss_weights"])
    l64, g64 = R.smooth_l1(*[np.asarray(v, np.float64) for v in args], np.float64(n))
    l32, g32 = R.smooth_l1(*args, np.float32(n))
    bad = g32.view(np.uint32) != d_ab.view(np.uint32)
    print("d_adj_bbox: %d of %d elements differ in bits from the float32 restatement" % (int(bad.sum()), bad.size))
    for r, j in np.argwhere(bad)[:8]:
        print("  [%d, %d] w %g  w (x - t) %r: device %r, float32 %r" % (r, j, args[2][r, j], float(E.smooth_l1_landing(x, args[1], args[2])[r, j]), float(d_ab[r, j]), float(g32[r, j])))
    ok = check("loss_bbox", [losses[2]], [l64], [l32])
    assert not bad.any()
    assert ok
