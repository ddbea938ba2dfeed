#!/usr/bin/env python3
"""Times bf16-operand training (az_*solver_set_precision(AZ_TRAIN_BF16)) against fp32 mode in ONE process on one card: the
full-size detection step (R = 128, C = 512, n6 = n7 = 4096, 21 classes) and the full-size AZ step (n6 = 4096, n71 = 1024,
n72 = 256), forward + backward with d conv5_3 + update, conv5_3 resident; then, per mode, the per-kernel table
(az_set_profiling events, median over --prof-reps steps) with every GEMM of fc6's three shapes and fc7's against
  * its HBM floor: (both fp32 operands + the fp32 result) / the copy rate az_measure_box reports on this card, and
  * the same launch in fp32 mode in this run.
The GEMM rows are the events of the step's own launches: az_solver_gemm_unit_prec copies its operands from the host on every
call, so its wall time is the copy's, not the kernel's.  Each step figure is warm-up, then median, min and max of --reps; fp32
mode is measured before AND after bf16 mode, and the distance between its two medians is the run-to-run spread the ratios are
to be read against.  Not collected by pytest; it lives under tests/ because it uses the tests' case builders.

  python tests/perf_train_bf16.py [--reps 20] [--warmup 3] [--prof-reps 7]"""
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
MODES = (("fp32", 0), ("bf16", 1))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                          # (step and update are synchronous calls)
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def kernel_table(ctx, fn, reps):
    """{name: (launches per step, median ms per step)} in first-seen order."""
    per, order = {}, []
    for _ in range(reps):
        ctx.set_profiling(2 | 4)                                      # (4: step and update keep one list; 0 clears it)
        fn()
        times = ctx.last_kernel_times()
        ctx.set_profiling(0)
        agg = {}
        for name, _, ms in times:
            if name not in agg:
                agg[name] = [0, 0.0]
                if name not in per:
                    per[name] = []
                    order.append(name)
            agg[name][0] += 1
            agg[name][1] += ms
        for name, (n, ms) in agg.items():
            per[name].append((n, ms))
    return [(name, per[name][0][0], float(np.median([m for _, m in per[name]]))) for name in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof-reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import det_step_ref as D
    import train_step_ref as R
    from aznet_hip import ffi, synth
    ctx = ffi.AzContext(0)
    ffi.set_default_context(ctx)
    mfma, copy = ctx.measure_box()
    print("this card: %.1f TFLOP/s fp32 MFMA (register loop), %.2f TB/s float4 copy (read + written)" % (mfma, copy))
    d = FULL
    Rn, K6 = 128, d["C"] * 49
    # M, N, K and the fp32 bytes of both operands and the result
    shapes = {"fc6_fwd": (Rn, d["n6"], K6), "fc6_dx": (Rn, K6, d["n6"]), "fc6_dw": (d["n6"], K6, Rn),
              "fc7_fwd": (Rn, d["n7"], d["n6"]), "fc7_dx": (Rn, d["n6"], d["n7"]), "fc7_dw": (d["n7"], d["n6"], Rn)}
    nbytes = {k: 4.0 * (M * K + N * K + M * N) for k, (M, N, K) in shapes.items()}

    # ---- the detection step ----------------------------------------------------------------------------------------------
    head = D.filler_head(5, **d)
    fmap = np.concatenate([synth.make_feature_map(s, 512, 38, 63) for s in (31, 32)], axis=0)
    blobs = D.random_blobs(11, Rn, 2, 38, 63, d["ncls"])
    sol = ffi.AzDetSolver(ctx, d["C"], d["n6"], d["n7"], d["ncls"], max_rois=Rn, head=head)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.empty_like(conv)
    it = [0]

    def det_step():
        _, sq = sol.step(conv, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"], 3, it[0], dmap=dmap)
        sol.update(0.001, 0.9, 0.0005, R.clip_scale(sq, 20.0))
        it[0] += 1
    step_ms, tables = {}, {}
    for label, mode in (("fp32", 0), ("bf16", 1), ("fp32 again", 0)):
        sol.set_precision(mode)
        step_ms[label] = timed(det_step, args.reps, args.warmup)
        print("detection step, %-10s: median %.3f ms, min %.3f, max %.3f of %d" % ((label,) + step_ms[label] + (args.reps,)))
        if label != "fp32 again":
            tables[label] = kernel_table(ctx, det_step, args.prof_reps)
    spread = abs(step_ms["fp32"][0] - step_ms["fp32 again"][0]) / step_ms["fp32"][0]
    print("detection step: bf16 / fp32 = %.3f (fp32's two medians %.1f %% apart)" % (step_ms["bf16"][0] / step_ms["fp32"][0], 100 * spread))
    fp = {name: ms for name, _, ms in tables["fp32"]}
    for label, _ in MODES:
        print("per launch group, %s mode (HIP events, median of %d steps):" % (label, args.prof_reps))
        for name, n, ms in tables[label]:
            note = ""
            if name in shapes:
                M, N, K = shapes[name]
                floor = nbytes[name] / (copy * 1e12) * 1e3
                note = "%dx%dx%d  %6.1f TFLOP/s  HBM floor %.3f ms (x%.2f)" % (M, N, K, 2.0 * M * N * K / (ms * 1e-3) / 1e12, floor, ms / floor)
                if label == "bf16":
                    note += "  bf16 / fp32 = %.3f" % (ms / fp[name])
            print("  %-16s x%-2d %9.3f ms  %s" % (name, n, ms, note))
        print("  sum %.3f ms" % sum(ms for _, _, ms in tables[label]))
    sol.close()
    del sol

    # ---- the AZ step ---------------------------------------------------------------------------------------------------------
    ahead, afmap, ablobs = R.full_size_case()
    asol = ffi.AzSolver(ctx, 512, R.FULL["n6"], R.FULL["n71"], R.FULL["n72"], max_rois=128, head=ahead)
    aconv = torch.from_numpy(afmap).cuda()
    admap = torch.empty_like(aconv)

    def az_step():
        _, sq = asol.step(aconv, ablobs["rois"], ablobs["adj_labels"], ablobs["adj_targets"], ablobs["adj_loss_weights"],
                          ablobs["zoom_labels"], 3, it[0], dmap=admap)
        asol.update(0.001, 0.9, 0.0005, R.clip_scale(sq, 20.0))
        it[0] += 1
    az_ms = {}
    for label, mode in (("fp32", 0), ("bf16", 1), ("fp32 again", 0)):
        asol.set_precision(mode)
        az_ms[label] = timed(az_step, args.reps, args.warmup)
        print("AZ step, %-10s: median %.3f ms, min %.3f, max %.3f of %d" % ((label,) + az_ms[label] + (args.reps,)))
    spread = abs(az_ms["fp32"][0] - az_ms["fp32 again"][0]) / az_ms["fp32"][0]
    print("AZ step: bf16 / fp32 = %.3f (fp32's two medians %.1f %% apart)" % (az_ms["bf16"][0] / az_ms["fp32"][0], 100 * spread))
    asol.close()


if __name__ == "__main__":
    main()
