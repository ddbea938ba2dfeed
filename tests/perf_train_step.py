#!/usr/bin/env python3
"""Times the full-size AZ-net head training step (C = 512, n6 = 4096, R = 128 rows over two 38 x 63 maps; forward + backward
+ update, conv5_3 resident): the HIP trainer (az_solver_step + az_solver_update) and, in the same process on the same card,
a torch-ROCm statement of the same step (torch.addmm, autograd, the same update) as the only available baseline.  Prints
both (warm-up, then the median of --reps), the per-kernel table (az_set_profiling), every GEMM against the fp32-MFMA rate
and the update against the copy rate az_measure_box reports on this card, and one full SolverWrapper iteration with the
VGG16 backbone.  Not collected by pytest; it lives under tests/ because it uses the tests' case builders.

  python tests/perf_train_step.py [--reps 20] [--warmup 3] [--no-wrapper]"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "az-net_amd", "lib"), REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_step(P, H, conv, blobs, masks, geom, rate, mom, wd, clip_at):
    """The same step in torch-ROCm: RoIPool by indexing with a precomputed arg-max (a gather; its backward an index_add),
    torch.addmm layers, autograd, then the update on every blob."""
    import torch
    flat = conv.reshape(conv.shape[0] * conv.shape[1], -1)
    x = torch.where(geom["ok"], flat.reshape(-1)[geom["idx"]], torch.zeros((), device=conv.device))
    a6 = torch.relu(torch.addmm(P["b6"], x, P["W6"].t())) * masks[0]
    a71 = torch.relu(torch.addmm(P["b71"], a6, P["W71"].t())) * masks[1]
    a72 = torch.relu(torch.addmm(P["b72"], a6, P["W72"].t())) * masks[2]
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    n = x.shape[0]
    loss = bce(torch.addmm(P["bz"], a72, P["Wz"].t()).reshape(-1), blobs["zoom_labels"], reduction="sum") / n
    loss = loss + bce(torch.addmm(P["bas"], a71, P["Was"].t()), blobs["adj_labels"], reduction="sum") / n
    d = blobs["adj_loss_weights"] * (torch.addmm(P["bab"], a71, P["Wab"].t()) - blobs["adj_targets"])
    loss = loss + torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum() / n
    for p in P.values():
        p.grad = None
    conv.grad = None
    loss.backward()
    with torch.no_grad():
        norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in P.values()))
        clip = torch.clamp(clip_at / norm, max=1.0).float()
        for k, p in P.items():
            bias = k.startswith("b")
            g = p.grad * clip + (0.0 if bias else wd) * p
            H[k].mul_(mom).add_(g, alpha=rate * (2.0 if bias else 1.0))
            p.sub_(H[k])
    return loss


def median_ms(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-wrapper", action="store_true")
    args = ap.parse_args()
    import torch
    import train_step_ref as R
    from aznet_hip import ffi
    ctx = ffi.AzContext(0)
    ffi.set_default_context(ctx)
    mfma, copy = ctx.measure_box()
    print("this card: %.1f TFLOP/s fp32 MFMA (register loop), %.2f TB/s float4 copy (read + written)" % (mfma, copy))
    head, fmap, blobs = R.full_size_case()
    d = R.FULL
    Rn, K6 = 128, d["C"] * 49
    sol = ffi.AzSolver(ctx, d["C"], d["n6"], d["n71"], d["n72"], max_rois=Rn, head=head)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.empty_like(conv)
    it = [0]

    def hip_step():
        _, sq = sol.step(conv, blobs["rois"], blobs["adj_labels"], blobs["adj_targets"], blobs["adj_loss_weights"],
                         blobs["zoom_labels"], 3, it[0], dmap=dmap)
        sol.update(0.001, 0.9, 0.0005, R.clip_scale(sq, 20.0))
        it[0] += 1
    hip_med, hip_min = median_ms(hip_step, args.reps, args.warmup, lambda: None)       # (both calls are synchronous)
    print("HIP trainer, full-size head step (forward + backward with d conv5_3 + update): median %.3f ms, best %.3f ms of %d"
          % (hip_med, hip_min, args.reps))
    ctx.set_profiling(2 | 4)
    hip_step()
    times = ctx.last_kernel_times()
    ctx.set_profiling(0)
    flops = {"int6_fwd": 2.0 * Rn * K6 * d["n6"], "int6_dx": 2.0 * Rn * K6 * d["n6"], "int6_dw": 2.0 * Rn * K6 * d["n6"],
             "int7_1_fwd": 2.0 * Rn * d["n6"] * d["n71"], "int7_1_dx": 2.0 * Rn * d["n6"] * d["n71"], "int7_1_dw": 2.0 * Rn * d["n6"] * d["n71"],
             "int7_2_fwd": 2.0 * Rn * d["n6"] * d["n72"], "int7_2_dx": 2.0 * Rn * d["n6"] * d["n72"], "int7_2_dw": 2.0 * Rn * d["n6"] * d["n72"]}
    nparam = sum(int(np.prod(v.shape)) for v in head.values())
    agg, order = {}, []
    for name, _, ms in times:
        if name not in agg:
            agg[name] = [0, 0.0]
            order.append(name)
        agg[name][0] += 1
        agg[name][1] += ms
    print("per launch group (HIP events on the trainer's stream, one step):")
    for name in order:
        n, ms = agg[name]
        note = ""
        if name in flops:
            tf = flops[name] / (ms * 1e-3) / 1e12
            note = "%6.1f TFLOP/s = %4.1f %% of the card's fp32-MFMA rate" % (tf, 100.0 * tf / mfma)
            if name == "int6_dw":
                note += "; writes %.0f MB = %.2f TB/s" % (4e-6 * K6 * d["n6"], 4.0 * K6 * d["n6"] / (ms * 1e-3) / 1e12)
            if name == "int6_fwd" or name == "int6_dx":
                note += "; streams %.0f MB = %.2f TB/s" % (4e-6 * K6 * d["n6"], 4.0 * K6 * d["n6"] / (ms * 1e-3) / 1e12)
        if name == "sgd_update":
            tb = 5.0 * 4.0 * nparam / (ms * 1e-3) / 1e12          # reads w, g, hist; writes w, hist
            note = "%.2f TB/s = %4.1f %% of the card's copy rate" % (tb, 100.0 * tb / copy)
        print("  %-16s x%-2d %9.3f ms  %s" % (name, n, ms, note))
    print("  sum %.3f ms in %d launch groups" % (sum(v[1] for v in agg.values()), sum(v[0] for v in agg.values())))
    sol.close()
    del sol

    # ---- the torch-ROCm statement of the same step -------------------------------------------------------------------
    dev = conv.device
    P = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in head.items()}
    Hh = {k: torch.zeros_like(v) for k, v in P.items()}
    pool, arg = R.roi_pool(fmap, blobs["rois"])
    C, HW = fmap.shape[1], fmap.shape[2] * fmap.shape[3]
    rows = (blobs["rois"][:, 0].astype(np.int64)[:, None] * C + np.repeat(np.arange(C), 49)[None, :]) * HW
    geom = {"idx": torch.from_numpy(rows + np.maximum(arg, 0)).to(dev), "ok": torch.from_numpy(arg >= 0).to(dev)}
    tb = {k: torch.from_numpy(v).to(dev) for k, v in blobs.items() if k != "rois" and k != "data"}
    masks = [torch.from_numpy(ffi.dropout_mask(3, 0, l, Rn * n).reshape(Rn, n).astype(np.float32) * 2).to(dev)
             for l, n in ((0, d["n6"]), (1, d["n71"]), (2, d["n72"]))]
    tconv = conv.clone().requires_grad_(True)
    t_med, t_min = median_ms(lambda: torch_step(P, Hh, tconv, tb, masks, geom, 0.001, 0.9, 0.0005, 20.0), args.reps, args.warmup,
                             torch.cuda.synchronize)
    print("torch-ROCm statement of the same step (addmm, autograd, same update; dropout masks and arg-max given): median %.3f ms, "
          "best %.3f ms of %d" % (t_med, t_min, args.reps))
    print("HIP / torch = %.2f" % (hip_med / t_med))
    del P, Hh
    torch.cuda.empty_cache()

    if not args.no_wrapper:
        import tempfile
        from datasets.synthetic import SyntheticImdb
        from detect import prototxt as Pt
        from detect.train_az import SolverWrapper, get_training_roidb
        tmp = tempfile.mkdtemp()
        net = os.path.join(tmp, "train.prototxt")
        Pt.write_train_prototxt(net, Pt.layer_table())
        solver = os.path.join(tmp, "solver.prototxt")
        Pt.write_solver_prototxt(solver, net, clip_gradients=20.0)
        imdb = SyntheticImdb(600, 1000, 4)
        np.random.seed(3)
        get_training_roidb(imdb)
        sw = SolverWrapper(solver, imdb, tmp, ctx=ctx, seed=3)
        w_med, w_min = median_ms(sw.step, max(5, args.reps // 2), 2, torch.cuda.synchronize)
        print("SolverWrapper iteration (data layer + VGG16 forward / backward of 2 images of 600 x 1000, conv3_1 .. conv5_3 training, "
              "+ head step + all updates): median %.1f ms, best %.1f ms" % (w_med, w_min))


if __name__ == "__main__":
    main()
