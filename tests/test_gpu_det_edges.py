"""GPU: the detection trainer (csrc/az_det_solver.hip) and the box-target kernels (csrc/az_det_train.hip) at their edges,
against tests/det_step_ref.py and tests/det_train_ref.py; the cases are built in tests/det_edges_ref.py and their conditions
asserted without a GPU in tests/test_det_edges_host.py.

1. k_solver_softmax_loss at lane-group and wave edges: rows that are exact in float32 (p = 1 / k or 0 on columns either side
   of every lane-group boundary, labels in every lane group, R a power of two) bit for bit; random rows with logits over
   +-30 at 65 .. 256 classes and 1 .. 257 rows; forward_test after a step.
2. The size contract's upper edge: 256 classes x 4096 rows (bbox_pred's unsplit product fills the slab buffer exactly),
   integer operands, bit for bit; what is refused beyond it; az_det_solver_fetch's states and capacity.
3. Hyper-parameters: per-layer dropout ratios that are no float32, that are 0 (the stale mask buffer is not read) or differ
   between fc6 and fc7, set after a step at the defaults; lr_mult 0 (fc7 frozen: not a bit moves and, lr_mult multiplying the
   decay too, its history stays zero although its decay_mult is 1), 0.1 and 3, decay on a bias and none on a weight; the
   step without d conv5_3; the same through SolverWrapper from an edited train net.
4. SolverWrapper with training convolutions: d conv5_3 into conv.backward, the joint clipping norm, az_sgd_update.
5. The target kernels on a set with images without example boxes, a tie at the threshold, identical objects, degenerate
   boxes, coordinates near 1e4 and other thresholds / eps; the statistics at 2 .. 300 classes with one-row and identical-row
   classes (nan, 0 or tiny stds as the reference gives them) and labels no kernel may count.

Tolerances: the trainer's rule (tests/test_gpu_det_train.py): 8 x the float32-CPU restatement's own error against float64,
floor 1e-6, gates as device_gates allows; probabilities within 1e-6 of float64.  Every figure is printed before it is
asserted (run with -s)."""
import ctypes
import os

import numpy as np
import pytest

import det_edges_ref as E
import det_step_ref as D
import det_train_ref as DR
from test_gpu_det_train import check, check_targets, device_gates, device_masks, make_solver, same_bits, step_args
from test_gpu_solver_edges import worst

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENSORS = ("pre6", "a6", "pre7", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score", "d_bbox_pred", "d_pre7", "d_pre6", "d_pool5")


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def g21():
    return np.load(os.path.join(REPO, "tests", "golden", "g21_train_det.npz"))


def softmax_refs(x, labels):
    """(float64, float32) restatements of the loss layer on the device's own logits."""
    n = x.shape[0]
    return D.softmax_loss(x.astype(np.float64), labels, float(n)), D.softmax_loss(x, labels, np.float32(n))


# ---- 1. softmax-with-loss at lane-group and wave edges ---------------------------------------------------------------------
@pytest.mark.parametrize("ncls", E.SM_NCLS)
def test_softmax_exact_rows_bit_for_bit(ctx, ncls):
    import torch
    head = D.filler_head(11, E.SM_DIMS["C"], E.SM_DIMS["n6"], E.SM_DIMS["n7"], ncls)
    head["Wc"][:] = 0                                                 # cls_score is its bias in every row
    sol = make_solver(ctx, head, max_rois=8)
    sol.set_hyper(dropout_ratio=[0.0, 0.0])
    ok = True
    for k in E.SM_K:
        if k > ncls:
            continue
        bias, labels, p_want, d_want = E.exact_case(ncls, k)
        n = labels.size
        fmap, rois = E.softmax_map(n)
        tgt = np.zeros((n, 4 * ncls), np.float32)
        sol.load({"bc": bias})
        losses, _ = sol.step(torch.from_numpy(fmap).cuda(), rois, labels, tgt, tgt, 1, 0)
        x = sol.fetch("cls_score")
        assert same_bits(x, np.tile(bias, (n, 1))), "the bias alone must be the logit row"
        p, d = sol.fetch("cls_prob"), sol.fetch("d_cls_score")
        print("ncls %d, columns %s at 3.5, R %d, labels %s: cls_prob differs in %d, d_cls_score in %d of %d"
              % (ncls, E.hot_columns(ncls, k), n, labels.astype(int).tolist(), int(np.sum(p != p_want)), int(np.sum(d != d_want)), p.size))
        assert same_bits(p, p_want), "cls_prob, ncls %d k %d" % (ncls, k)
        assert same_bits(d, d_want), "d_cls_score, ncls %d k %d" % (ncls, k)
        (l64, _, _), (l32, _, _) = softmax_refs(x, labels)
        ok &= check("loss_cls k=%d" % k, [losses[0]], [l64], [l32])
    sol.close()
    assert ok


@pytest.mark.parametrize("ncls", E.SMR_NCLS)
def test_softmax_random_rows(ctx, ncls):
    import torch
    from aznet_hip import ffi
    ok, rows = True, [("gates that differ", 0.0, 0.0, 0.0)]
    for n in E.SMR_ROWS:
        head, fmap, blobs, pool, seed = E.random_case(ncls, n)
        sol = make_solver(ctx, head, max_rois=n)
        sol.set_hyper(dropout_ratio=[0.0, 0.0])
        conv = torch.from_numpy(fmap).cuda()
        losses, _ = sol.step(*step_args(conv, blobs), 1, 0)
        assert np.array_equal(sol.fetch("pool5"), pool)
        x, p, d = sol.fetch("cls_score"), sol.fetch("cls_prob"), sol.fetch("d_cls_score")
        (l64, d64, p64), (l32, d32, p32) = softmax_refs(x, blobs["labels"])
        err = float(np.abs(p - p64).max())
        print("ncls %d, R %d: logits in [%.1f, %.1f], max |p - p64| = %.3e (float32-CPU %.3e)"
              % (ncls, n, x.min(), x.max(), err, float(np.abs(p32 - p64).max())))
        assert x.shape == (n, ncls) and np.abs(x).max() > 0.8 * E.SMR_SPAN
        assert np.all(np.isfinite(p)) and np.all(np.isfinite(d)) and err <= 1e-6
        ok &= check("d_cls_score R=%d" % n, d, d64, d32, rows)
        ok &= check("loss_cls R=%d" % n, [losses[0]], [l64], [l32], rows)
        if n in (3, 257):                                             # c. the TEST-phase forward after the step: the same bits
            p_test, _ = sol.forward_test(conv, blobs["rois"])
            assert same_bits(p_test, p) and same_bits(sol.fetch("cls_prob"), p)
            with pytest.raises(ffi.AzError) as e:
                sol.update(0.001, 0.9, 0.0005, 1.0)                   # forward_test leaves no gradients to apply
            assert e.value.code == ffi.AZ_ERR_STATE
        sol.close()
    worst("softmax, random rows, %d classes" % ncls, rows)
    assert ok


# ---- 2. the size contract's upper edge -------------------------------------------------------------------------------------
def test_size_contract_upper_edge(ctx):
    import torch
    from aznet_hip import ffi
    S = E.SIZE
    head, fmap, blobs, pool = E.size_case()
    with pytest.raises(ffi.AzError) as e:
        ffi.AzDetSolver(ctx, S["C"], S["n6"], S["n7"], S["ncls"], max_rois=S["R"] + 1)
    assert e.value.code == ffi.AZ_ERR_INVALID
    sol = make_solver(ctx, head, max_rois=S["R"])
    with pytest.raises(ffi.AzError) as e:                             # no pass yet: no activation, but the parameters
        sol.fetch("pool5")
    assert e.value.code == ffi.AZ_ERR_STATE
    assert same_bits(sol.fetch("w_W6"), head["W6"])
    need, small = ctypes.c_longlong(0), np.full(8, 7.0, np.float32)
    rc = ctx.L.az_det_solver_fetch(sol.h, b"w_W6", small.ctypes.data_as(ctypes.c_void_p), small.nbytes, ctypes.byref(need))
    assert rc == ffi.AZ_ERR_CAPACITY and need.value == head["W6"].nbytes and np.all(small == 7.0)
    sol.set_hyper(dropout_ratio=[0.0, 0.0])
    r64 = D.step(head, pool, blobs, None, want_dpool=False)
    r32 = D.step(head, pool, blobs, None, dtype=np.float32, want_dpool=False)
    conv = torch.from_numpy(fmap).cuda()
    _, b = sol.forward_test(conv, blobs["rois"])
    assert same_bits(sol.fetch("cls_score"), r64["cls_score"].astype(np.float32)), "cls_score of forward_test"
    assert same_bits(b, r64["bbox_pred"].astype(np.float32)), "bbox_pred of forward_test"
    losses, _ = sol.step(*step_args(conv, blobs), 1, 0)
    for nm in ("cls_score", "bbox_pred", "pre6"):
        got = sol.fetch(nm)
        print("  %s of the step: %d of %d elements differ" % (nm, int(np.sum(got != r64[nm])), got.size))
        assert same_bits(got, r64[nm].astype(np.float32)), nm
    assert np.array_equal(sol.fetch("pool5"), pool), "pool5"
    p = sol.fetch("cls_prob")
    err = float(np.abs(p - r64["cls_prob"]).max())
    print("  %d rows x %d classes: max |p - p64| = %.3e" % (S["R"], S["ncls"], err))
    assert np.all(np.isfinite(p)) and err <= 1e-6
    assert check("losses", losses, r64["losses"], r32["losses"])
    # one row more than max_rois: refused before anything is enqueued
    before = {k: sol.fetch(k) for k in ("cls_prob", "bbox_pred", "pre6")}
    more = {k: np.concatenate([v, v[:1]]) for k, v in blobs.items()}
    with pytest.raises(ffi.AzError) as e:
        sol.step(*step_args(conv, more), 1, 1)
    assert e.value.code == ffi.AZ_ERR_INVALID
    with pytest.raises(ffi.AzError):
        sol.forward_test(conv, more["rois"])
    assert all(same_bits(sol.fetch(k), v) for k, v in before.items())
    sol.close()


# ---- 3. hyper-parameters off the defaults ------------------------------------------------------------------------------------
def compare_step(sol, head, fmap, blobs, seed, it, ratios, losses, sumsq, dmap):
    """The tensors of test_one_step against the restatement at `ratios`; returns (ok, rows, r64, r32)."""
    pool, arg = D.roi_pool(fmap, blobs["rois"])
    assert np.array_equal(sol.fetch("pool5"), pool) and np.array_equal(sol.fetch("argmax"), arg)
    masks = device_masks(sol, seed, it, ratios)
    assert sorted(masks) == [t for t, l, _ in D.LAYERS if ratios[l] > 0]
    ngates = []
    gates = device_gates(sol, head, pool, blobs, masks, ngates, ratios)
    for t, l, _ in D.LAYERS:                                          # ReLU + dropout: exact given the pre-activation
        pre, a, dp = sol.fetch("pre%d" % t), sol.fetch("a%d" % t), sol.fetch("d_pre%d" % t)
        relu = np.maximum(pre, np.float32(0))
        if ratios[l] > 0:
            assert same_bits(a, np.where(masks[t] > 0, relu * E.f32_scale(ratios[l]), np.float32(0)).astype(np.float32)), "a%d" % t
            assert not dp[(pre <= 0) | (masks[t] == 0)].any()
        else:
            assert same_bits(a, relu), "a%d at ratio 0" % t
            assert not dp[pre <= 0].any()
    r64 = D.step(head, pool, blobs, masks, gates=gates, ratios=ratios)
    r32 = D.step(head, pool, blobs, masks, gates=gates, dtype=np.float32, ratios=ratios)
    rows, ok = [("gates that differ", float(sum(ngates)), 0.0, 0.0)], True
    for nm in TENSORS if dmap is not None else TENSORS[:-1]:         # (d_pool5 is computed only for d conv5_3)
        ok &= check(nm, sol.fetch(nm).reshape(np.shape(r64[nm])), r64[nm], r32[nm], rows)
    ok &= check("losses", losses, r64["losses"], r32["losses"], rows)
    for k in D.KEYS:
        ok &= check("g_" + k, sol.fetch("g_" + k), r64["grads"][k], r32["grads"][k], rows)
    ok &= check("sumsq", [sumsq], [r64["sumsq"]], [r32["sumsq"]], rows)
    if dmap is not None:
        d64, d32 = (D.roi_pool_backward(r["d_pool5"], arg, blobs["rois"], fmap.shape) for r in (r64, r32))
        ok &= check("d_conv5_3", dmap.cpu().numpy(), d64, d32, rows)
    return ok, rows, r64, r32


@pytest.mark.parametrize("name", E.HYPER_HEADS)
@pytest.mark.parametrize("ratios", E.RATIO_SETS, ids=lambda r: "-".join("%g" % x for x in r))
def test_one_step_with_other_ratios(ctx, ratios, name):
    import torch
    head, fmap, blobs = D.case(name)
    print("%s head, R = %d, one step at the defaults, then dropout %s" % (name, D.HEADS[name]["R"], ratios))
    seed = 3
    sol = make_solver(ctx, head)
    conv = torch.from_numpy(fmap).cuda()
    if name == "coco":
        conv = conv.contiguous(memory_format=torch.channels_last)
    dmap = torch.empty_like(conv)
    sol.step(*step_args(conv, blobs), seed, 0)                        # at (0.5, 0.5): both mask buffers now hold a mask
    stale = {t: sol.fetch("mask%d" % t) for t, _, _ in D.LAYERS}
    assert all((m == 0).any() and (m == 1).any() for m in stale.values())
    sol.set_hyper(dropout_ratio=list(ratios))
    losses, sumsq = sol.step(*step_args(conv, blobs), seed, 1, dmap=dmap)
    for t, l, _ in D.LAYERS:
        if ratios[l] == 0:                                            # no mask is drawn: the buffer keeps the stale one
            assert same_bits(sol.fetch("mask%d" % t), stale[t])
    ok, rows, _, _ = compare_step(sol, head, fmap, blobs, seed, 1, ratios, losses, sumsq, dmap)
    sol.close()
    worst("ratios %s, %s head" % (ratios, name), rows)
    assert ok, "a tensor exceeds 8 x the float32-CPU error: " + ", ".join(r[0] for r in rows[1:] if r[1] > r[3])


def test_multipliers_and_the_frozen_layer(ctx):
    """fc7 frozen by lr_mult 0 / 0 with its decay_mult left at 1 / 0 (the case tested: decay_mult NOT zero): the expected
    history comes from the restatement's sgd, where the local rate multiplies the decay too, so it is zero all the same."""
    import torch
    head, fmap, blobs = D.case("voc")
    lr, dc = E.hyper_multipliers()
    sol = make_solver(ctx, head)
    sol.set_hyper(lr_mult=[lr[k] for k in D.KEYS], decay_mult=[dc[k] for k in D.KEYS])
    conv = torch.from_numpy(fmap).cuda()
    seed, it, ratios = 3, 0, (0.5, 0.5)
    losses, sumsq = sol.step(*step_args(conv, blobs), seed, it)
    ok, rows, r64, r32 = compare_step(sol, head, fmap, blobs, seed, it, ratios, losses, sumsq, None)
    rate, mom, wd = 0.001, 0.9, 0.0005
    mult = dict(lr_mult=lr, decay_mult=dc)
    zeros = {k: np.zeros_like(v) for k, v in head.items()}
    for rep, clip_at in ((0, 1e-3), (1, None)):                       # a clipped update, then an unclipped one on its history
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
        for k in ("W7", "b7"):
            assert np.abs(sol.fetch("g_" + k)).max() > 0
            assert same_bits(sol.fetch("w_" + k), head[k]), "%s moved in update %d" % (k, rep)
            assert np.array_equal(sol.fetch("h_" + k), h32[k]) and not h32[k].any() and not h64[k].any(), "history of " + k
    for k in D.KEYS:
        if k not in ("W7", "b7"):
            assert not same_bits(sol.fetch("w_" + k), head[k]), k
    sol.close()
    worst("multipliers, voc head", rows)
    assert ok, "a tensor exceeds 8 x the float32-CPU error: " + ", ".join(r[0] for r in rows[1:] if r[1] > r[3])


def test_step_without_dmap_gives_the_same_bits(ctx):
    import torch
    head, fmap, blobs = D.case("coco")
    sol = make_solver(ctx, head)
    conv = torch.from_numpy(fmap).cuda()
    names = ["g_" + k for k in D.KEYS] + ["d_pre6", "d_pre7"]
    l0, s0 = sol.step(*step_args(conv, blobs), 5, 2)
    t0 = [sol.fetch(n) for n in names]
    dmap = torch.zeros_like(conv)
    l1, s1 = sol.step(*step_args(conv, blobs), 5, 2, dmap=dmap)
    t1 = [sol.fetch(n) for n in names]
    sol.close()
    assert float(dmap.abs().max()) > 0
    assert same_bits(l0, l1) and same_bits(np.float64(s0), np.float64(s1)) and s0 > 0
    for n, a, b in zip(names, t0, t1):
        assert same_bits(a, b), n


def _det_wrapper(ctx, g21, tmp_path, monkeypatch, frozen_all, edit_rows=None):
    from aznet_hip import ffi
    from detect.train_det import SolverWrapper
    from roi_data_layer import roidb as rdl
    T = D.TRAJ
    ffi.set_default_context(ctx)
    imdb, _, _ = DR.synthetic_roidb(rdl, g21, tmp_path, monkeypatch)
    np.random.seed(T["np_seed"])
    return SolverWrapper(D.traj_solver_files(str(tmp_path), frozen_all, edit_rows), imdb, str(tmp_path / "out"),
                         backbone=D.traj_backbone("cuda:0"), ctx=ctx, dims=dict(n6=T["n6"], n7=T["n7"]), seed=T["solver_seed"])


def test_other_hyper_parameters_through_solver_wrapper(ctx, g21, tmp_path, monkeypatch):
    """Three steps of SolverWrapper on a train net with dropout 0.3 on fc6, no Dropout block on fc7 and fc7's lr_mult 0 0,
    beside RefTrajectory with the same ratios and multipliers."""
    T, F = D.TRAJ, E.FRONT_DOOR
    sw = _det_wrapper(ctx, g21, tmp_path, monkeypatch, True, E.front_door_rows)
    assert sw.conv_train == []
    start = sw.trainer.read()
    lr, dc = E.front_door_multipliers()
    ref64, ref32 = (D.RefTrajectory(start, dt, T["solver"], ratios=F["ratios"], lr_mult=lr, decay_mult=dc) for dt in (np.float64, np.float32))
    ok, ngates, rows = True, [], [("gates that differ", 0.0, 0.0, 0.0)]
    for it in range(F["steps"]):
        before = sw.trainer.read()
        losses = sw.step()
        conv, blobs = sw.last_conv.cpu().numpy(), sw.last_blobs
        pool, _ = D.roi_pool(conv, blobs["rois"])
        print("step %d (%d rows)" % (it, pool.shape[0]))
        masks = device_masks(sw.trainer, T["solver_seed"], it, F["ratios"])
        assert sorted(masks) == [6]
        gates = device_gates(sw.trainer, before, pool, blobs, masks, ngates, F["ratios"])
        pre, a = sw.trainer.fetch("pre7"), sw.trainer.fetch("a7")
        assert same_bits(a, np.maximum(pre, np.float32(0)))                 # no Dropout block: a7 = relu(pre7)
        r64, r32 = ref64.step(conv, blobs, T["solver_seed"], gates), ref32.step(conv, blobs, T["solver_seed"], gates)
        ok &= check("losses[%d]" % it, losses, r64["losses"], r32["losses"], rows)
    rows[0] = ("gates that differ", float(sum(ngates)), 0.0, 0.0)
    worst("front door, %d steps" % F["steps"], rows)
    assert ok, "a step's losses exceed 8 x the float32-CPU error"
    end = sw.trainer.read()
    for k in D.KEYS:
        moved = not same_bits(end[k], start[k])
        print("  %s %s" % (k, "moved" if moved else "unchanged"))
        assert moved == (k not in ("W7", "b7")), k


# ---- 4. convolutions that train ------------------------------------------------------------------------------------------------
def test_convolutions_train_with_the_same_update(ctx, g21, tmp_path, monkeypatch):
    """conv3_1 .. conv5_3 trainable: d conv5_3 goes into conv.backward, the convolution gradients join the clipping norm,
    and every trainable convolution takes az_sgd_update's step; 20 steps at det_step_ref.TRAJ's base_lr (found on the CPU with
    the convolutions frozen: tests/test_det_train_host.py::test_frozen_run_restatement_lowers_the_loss)."""
    from aznet_hip import ffi
    from detect import prototxt as P
    T = D.TRAJ
    sw = _det_wrapper(ctx, g21, tmp_path, monkeypatch, False)
    names = [c[0] for c in sw.conv_train]
    assert names == list(P.CONV_LAYERS[4:])
    w0 = {l[0]: (l[1].detach().cpu().numpy().copy(), l[2].detach().cpu().numpy().copy()) for l in sw.backbone.layers if l is not None}
    tot = [float(np.sum(sw.step()))]
    sp = sw.solver_param
    norm = np.sqrt(sw.last_sumsq)
    print("step 1: sumsq %.6g, of the head %.6g, clip %.6g" % (sw.last_sumsq, sw.last_head_sumsq, sw.last_clip))
    assert sw.last_sumsq > sw.last_head_sumsq > 0
    assert sw.last_clip == (sp["clip_gradients"] / norm if norm > sp["clip_gradients"] else 1.0)
    far = 0.0
    for name, w, b, hw, hb, lr, dc in sw.conv_train:
        for p, h, q in ((w, hw, 0), (b, hb, 1)):
            want_w, want_h = ffi.sgd_update_numpy(w0[name][q], p.grad.cpu().numpy(), np.zeros_like(w0[name][q]),
                                                  sw.last_rate * lr[q], sp["momentum"], sp["weight_decay"] * dc[q], sw.last_clip)
            assert np.abs(p.grad.cpu().numpy()).max() > 0, name
            for got, want in ((p.detach().cpu().numpy(), want_w), (h.cpu().numpy(), want_h)):
                ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                far = max(far, float(ulp.max()))
    print("trainable convolution parameters after step 1: at most %.1f ulp from the NumPy form" % far)
    assert far <= 1.0
    for l in sw.backbone.layers:
        if l is not None and l[0] not in names:
            assert same_bits(l[1].detach().cpu().numpy(), w0[l[0]][0]) and same_bits(l[2].detach().cpu().numpy(), w0[l[0]][1])
    for _ in range(T["steps"] - 1):
        tot.append(float(np.sum(sw.step())))
    print("summed loss per step: " + " ".join("%.3f" % t for t in tot))
    print("summed loss: first five %.4f, last five %.4f" % (sum(tot[:5]), sum(tot[-5:])))
    assert sum(tot[-5:]) < sum(tot[:5])
    for l in sw.backbone.layers:
        if l is not None and l[0] not in names:
            assert same_bits(l[1].detach().cpu().numpy(), w0[l[0]][0]) and same_bits(l[2].detach().cpu().numpy(), w0[l[0]][1])


# ---- 5. target kernels on hostile sets -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def target_refs():
    return {key: E.reference_targets(key) for key in E.TARGET_SETTINGS}


@pytest.mark.parametrize("key", sorted(E.TARGET_SETTINGS))
def test_targets_on_the_hostile_set(ctx, target_refs, key):
    ex, gt, lab = E.offsets_case()
    s = E.TARGET_SETTINGS[key]
    args = (s["bbox_thresh"], s["bg_lo"], s["eps"])
    off = E.offsets_of(ex)
    print("bbox_thresh %g, bg_thresh_lo %g, eps %g; example offsets %s" % (args + (off.tolist(),)))
    t, mo = ctx.det_targets(np.vstack(ex), off, gt, lab, *args)      # one launch: empty first and last image, an empty run
    assert t.shape == (off[-1], 5) and mo.shape == (off[-1],) and mo.dtype == np.float64
    for i, (want_t, want_mo) in enumerate(target_refs[key]):
        ti, mi = t[off[i]:off[i + 1]], mo[off[i]:off[i + 1]]
        check_targets(ti, want_t, "image %d" % i)
        assert same_bits(mi, want_mo), "max_overlaps of image %d" % i
        one = ctx.det_targets(ex[i], [0, ex[i].shape[0]], [gt[i]], [lab[i]], *args)              # the same image alone
        assert same_bits(one[0], ti) and same_bits(one[1], mi), "image %d alone" % i


@pytest.fixture(scope="module")
def stats_refs():
    return {ncls: E.reference_stats(ncls) for ncls in E.STATS_NCLS}


@pytest.mark.parametrize("ncls", E.STATS_NCLS)
def test_target_stats_on_hostile_sets(ctx, stats_refs, ncls):
    raw = E.stats_case(ncls)
    off = E.offsets_of(raw)
    counts, means, stds, norm = stats_refs[ncls]
    runs = []
    for _ in range(2):
        t = np.ascontiguousarray(np.vstack(raw))
        runs.append((t,) + tuple(ctx.det_target_stats(t, off, ncls, DR.EPS, True)))
    t, c, m, s = runs[0]
    print("%d classes, %d images, %d rows: stds nan %d (yardstick %d), zero %d (%d), below 1e-6 %d (%d); normalised targets nan %d "
          "(%d), inf %d (%d)" % (ncls, len(raw), t.shape[0], int(np.isnan(s).sum()), int(np.isnan(stds).sum()), int((s == 0).sum()),
                                 int((stds == 0).sum()), int((s < 1e-6).sum()), int((stds < 1e-6).sum()), int(np.isnan(t).sum()),
                                 int(np.isnan(norm).sum()), int(np.isinf(t).sum()), int(np.isinf(norm).sum())))
    assert same_bits(c, counts), "counts"
    assert same_bits(m, means), "means"
    assert E.same_or_both_nan(s, stds), "stds"
    assert E.same_or_both_nan(t, norm), "normalised targets"
    assert all(same_bits(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ"
    t = np.ascontiguousarray(np.vstack(raw))
    c2, m2, s2 = ctx.det_target_stats(t, off, ncls, DR.EPS, False)
    assert same_bits(t, np.vstack(raw)) and same_bits(c2, c) and same_bits(m2, m) and same_bits(s2, s)
