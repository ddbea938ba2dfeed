#!/usr/bin/env python3
"""Times the full-size training step of the skip-connection detector (Cs = 256 / 512 / 512 on a 600 x 1000 image's three
maps of 150 x 250, 75 x 125 and 38 x 63 cells, one image, R = 128 rois; Cout = 512, n6 = n7 = 4096, 21 classes; forward +
backward with all three map gradients + update, the maps resident): the HIP trainer (az_det_solver_step_skip +
az_det_solver_update) and, in the same process on the same card, a torch-ROCm autograd statement of the same front + head.
Prints both (warm-up, then the median of --reps), the per-kernel table (az_set_profiling) and the front's three GEMMs against
the fp32-MFMA rate az_measure_box reports on this card.  Not collected by pytest; it lives under tests/ because it uses the
tests' case builders.  It writes nothing into bench.py's line.

  python tests/perf_skip_train_step.py [--reps 10] [--warmup 2]"""
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

FULL = dict(C=512, n6=4096, n7=4096, ncls=21)
CS = (256, 512, 512)
HW = ((150, 250), (75, 125), (38, 63))
GAIN, EPS = 1000.0, 1e-10


def torch_step(P, H, maps, geoms, blobs, masks, offs, rate, mom, wd, clip_at):
    """The same step in torch-ROCm: the three RoIPools by indexing with a precomputed arg-max (their backward an index_add),
    GRN and scale as tensor ops, the 1x1 convolution and the fc layers as addmm, cross_entropy and SmoothL1, autograd, then
    the update on every blob."""
    import torch
    blocks = []
    for m, g in zip(maps, geoms):
        x = torch.where(g["ok"], m.reshape(-1)[g["idx"]], torch.zeros((), device=m.device))
        blocks.append(GAIN * x / torch.sqrt((x * x).sum(dim=1, keepdim=True) + EPS))
    cat = torch.cat(blocks, dim=1)
    y = torch.relu(torch.addmm(P["bp"], cat, P["Wp"].t()))
    n = y.shape[0] // 49
    x = y.reshape(n, 49, -1).permute(0, 2, 1).reshape(n, -1)
    a6 = torch.relu(torch.addmm(P["b6"], x, P["W6"].t())) * masks[0]
    a7 = torch.relu(torch.addmm(P["b7"], a6, P["W7"].t())) * masks[1]
    loss = torch.nn.functional.cross_entropy(torch.addmm(P["bc"], a7, P["Wc"].t()), blobs["labels"], reduction="sum") / n
    d = blobs["bbox_loss_weights"] * (torch.addmm(P["bb"], a7, P["Wb"].t()) - blobs["bbox_targets"])
    loss = loss + torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum() / n
    for p in P.values():
        p.grad = None
    for m in maps:
        m.grad = None
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import det_step_ref as D
    import skip_train_ref as T
    import train_step_ref as R
    from aznet_hip import ffi, synth
    ctx = ffi.AzContext(0)
    mfma, copy = ctx.measure_box()
    print("this card: %.1f TFLOP/s fp32 MFMA (register loop), %.2f TB/s float4 copy (read + written)" % (mfma, copy))
    d = FULL
    Rn, sumC, Cout = 128, sum(CS), FULL["C"]
    head = D.filler_head(5, **d)
    front = T.make_front(7, CS, Cout, GAIN, EPS)
    maps = [synth.make_feature_map(31 + i, C, h, w) for i, (C, (h, w)) in enumerate(zip(CS, HW))]
    blobs = D.random_blobs(11, Rn, 1, 38, 63, d["ncls"])
    sol = ffi.AzDetSolver(ctx, Cout, d["n6"], d["n7"], d["ncls"], max_rois=Rn, head=head)
    sol.attach_skip(CS, (0.25, 0.125, 0.0625), gain=GAIN, eps=EPS, seed=1, front=front)
    results = {}
    for cl in (True, False):
        dev = [torch.from_numpy(m).cuda() for m in maps]
        if cl:
            dev = [t.contiguous(memory_format=torch.channels_last) for t in dev]
        dmaps = [torch.empty_like(t) for t in dev]
        it = [0]

        def hip_step():
            _, sq = sol.step_skip(dev, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"], 3, it[0], dmaps=dmaps)
            sol.update(0.001, 0.9, 0.0005, R.clip_scale(sq, 20.0))
            it[0] += 1
        med, best = median_ms(hip_step, args.reps, args.warmup, lambda: None)         # (both calls are synchronous)
        results[cl] = med
        print("HIP trainer, full-size skip step, %s maps (forward + backward with three map gradients + update): median %.3f ms, "
              "best %.3f ms of %d" % ("channels-last" if cl else "NCHW", med, best, args.reps))
        ctx.set_profiling(2 | 4)
        hip_step()
        times = ctx.last_kernel_times()
        ctx.set_profiling(0)
        rows = Rn * 49
        fg = 2.0 * rows * sumC * Cout
        flops = {"conv_pool5_fwd": fg, "conv_pool5_dw": fg, "conv_pool5_dx": fg}
        agg, order = {}, []
        for name, _, ms in times:
            if name not in agg:
                agg[name] = [0, 0.0]
                order.append(name)
            agg[name][0] += 1
            agg[name][1] += ms
        total = sum(v[1] for v in agg.values())
        print("per launch group (HIP events on the trainer's stream, one step, %s maps):" % ("channels-last" if cl else "NCHW"))
        for name in order:
            n, ms = agg[name]
            note = ""
            if name in flops:
                tf = flops[name] / (ms * 1e-3) / 1e12
                note = "%6.1f TFLOP/s = %4.1f %% of the card's fp32-MFMA rate" % (tf, 100.0 * tf / mfma)
            if name.startswith("skip_pool_bwd"):
                note = "%4.1f %% of the step's kernel time" % (100.0 * ms / total)
            print("  %-18s x%-2d %9.3f ms  %s" % (name, n, ms, note))
        print("  sum %.3f ms in %d launch groups" % (total, sum(v[0] for v in agg.values())))
    sol.close()
    del sol

    # ---- the torch-ROCm statement of the same step -------------------------------------------------------------------
    device = torch.device("cuda:0")
    P = {k: torch.from_numpy(v).to(device).requires_grad_(True) for k, v in head.items()}
    P["Wp"] = torch.from_numpy(front["Wp"]).to(device).requires_grad_(True)
    P["bp"] = torch.from_numpy(front["bp"]).to(device).requires_grad_(True)
    Hh = {k: torch.zeros_like(v) for k, v in P.items()}
    raw, arg = T.pool_argmax(maps, blobs["rois"])
    offs = T.offsets(CS)
    geoms = []
    n_row = np.repeat(blobs["rois"][:, 0].astype(np.int64), 49)
    for i, (C, (h, w)) in enumerate(zip(CS, HW)):
        a = arg[:, offs[i]:offs[i + 1]].astype(np.int64)
        lin = (n_row[:, None] * C + np.arange(C)[None, :]) * (h * w) + np.maximum(a, 0)
        geoms.append({"idx": torch.from_numpy(lin).to(device), "ok": torch.from_numpy(a >= 0).to(device)})
    tb = {k: torch.from_numpy(v).to(device) for k, v in blobs.items() if k != "rois"}
    tb["labels"] = tb["labels"].long()
    masks = [torch.from_numpy(ffi.dropout_mask(3, 0, l, Rn * n).reshape(Rn, n).astype(np.float32) * 2).to(device)
             for l, n in ((0, d["n6"]), (1, d["n7"]))]
    tmaps = [torch.from_numpy(m).to(device).requires_grad_(True) for m in maps]
    t_med, t_min = median_ms(lambda: torch_step(P, Hh, tmaps, geoms, tb, masks, offs, 0.001, 0.9, 0.0005, 20.0), args.reps, args.warmup,
                             torch.cuda.synchronize)
    print("torch-ROCm statement of the same step (index gather, GRN, addmm, autograd, same update; dropout masks and arg-max given): "
          "median %.3f ms, best %.3f ms of %d" % (t_med, t_min, args.reps))
    print("HIP / torch = %.2f (channels-last), %.2f (NCHW)" % (results[True] / t_med, results[False] / t_med))


if __name__ == "__main__":
    main()
