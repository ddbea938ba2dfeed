#!/usr/bin/env python3
"""Times online hard-example mining at full size (C = 512, n6 = n7 = 4096, ncls = 21, two 38 x 63 maps, a pool of 2 x 2000 rows,
128 mined rows), in fp32 and in bf16, conv5_3 resident: the mining call (az_det_solver_mine), its per-stage kernel table
(RoIPool, the four forward GEMMs against the fp32-MFMA rate az_measure_box reports on this card, k_det_row_loss, NMS, the
selection), the step on the mined rows, and a whole OHEM iteration (mine + host gather + step + update) against the plain
iteration (step + update on 128 rows) in the same process.  The plain iteration is measured before and after the mining
measurements (measuring-on-mi355x: a drifting clock shows as a difference between the two).  Warm-up, then the median of
--reps.  Not collected by pytest; it lives under tests/ because it uses the tests' case builders.

  python tests/perf_ohem.py [--reps 20] [--warmup 3] [--pool 2000]"""
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
MAP_H, MAP_W = 38, 63


def median_ms(fn, reps, warmup):
    """(median, best) of a synchronous call."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pool", type=int, default=2000)
    args = ap.parse_args()
    import torch
    import det_step_ref as D
    import ohem_ref as O
    import train_step_ref as R
    from aznet_hip import ffi, synth
    from roi_data_layer.minibatch import _get_bbox_regression_labels
    ctx = ffi.AzContext(0)
    mfma, copy = ctx.measure_box()
    print("this card: %.1f TFLOP/s fp32 MFMA (register loop), %.2f TB/s float4 copy (read + written)" % (mfma, copy))
    d = FULL
    Rn, Rp, K6, nb = 128, 2 * args.pool, d["C"] * 49, 4 * d["ncls"]
    head = D.filler_head(5, **d)
    fmap = np.concatenate([synth.make_feature_map(s, 512, MAP_H, MAP_W) for s in (31, 32)], axis=0)
    plain = D.random_blobs(11, Rn, 2, MAP_H, MAP_W, d["ncls"])
    pool = O.pool_blobs(12, (args.pool, args.pool), d["ncls"], H=MAP_H, W=MAP_W)
    sol = ffi.AzDetSolver(ctx, d["C"], d["n6"], d["n7"], d["ncls"], max_rois=Rp, head=head)
    conv = torch.from_numpy(fmap).cuda()
    dmap = torch.empty_like(conv)
    it = [0]

    def step_update(b):
        _, sq = sol.step(conv, b["rois"], b["labels"], b["bbox_targets"], b["bbox_loss_weights"], 3, it[0], dmap=dmap)
        sol.update(0.001, 0.9, 0.0005, R.clip_scale(sq, 20.0))
        it[0] += 1

    def mine():
        return sol.mine(conv, pool["rois"], pool["labels"], pool["targets"], 0.7, Rn // 2)

    def gather(sel):
        lab = pool["labels"][sel]
        bt, bw = _get_bbox_regression_labels(np.hstack((lab[:, None], pool["targets"][sel])), d["ncls"])
        return {"rois": np.ascontiguousarray(pool["rois"][sel]), "labels": lab, "bbox_targets": bt, "bbox_loss_weights": bw}

    def ohem_iteration():
        step_update(gather(mine()[0]))

    def timed(fn):
        sol.load(head)                          # (every measurement from the same weights: a run on noise must not drift to NaN)
        sol.load_history({k: np.zeros_like(v) for k, v in head.items()})
        return median_ms(fn, args.reps, args.warmup)

    f6, f7 = 2.0 * Rp * K6 * d["n6"], 2.0 * Rp * d["n6"] * d["n7"]
    flops = {"fc6_fwd": f6, "fc7_fwd": f7, "cls_score_fwd": 2.0 * Rp * d["n7"] * d["ncls"], "bbox_pred_fwd": 2.0 * Rp * d["n7"] * nb}
    for prec, pname in ((0, "fp32"), (1, "bf16")):
        sol.set_precision(prec)
        print("---- %s operands ----" % pname)
        p0 = timed(lambda: step_update(plain))
        print("plain iteration (step on %d rows with d conv5_3 + update), before: median %.3f ms, best %.3f ms of %d" % ((Rn,) + p0 + (args.reps,)))
        m = timed(mine)
        sel, n_sel, _ = mine()
        print("mining call, pool of %d rows -> %s rows kept of %s, %d selected: median %.3f ms, best %.3f ms of %d"
              % (Rp, sol.fetch("mine_nkeep").tolist(), [args.pool] * 2, sel.size, m[0], m[1], args.reps))
        ctx.set_profiling(2 | 4)
        mine()
        times = ctx.last_kernel_times()
        ctx.set_profiling(0)
        agg, order = {}, []
        for name, _, ms in times:
            if name not in agg:
                agg[name] = [0, 0.0]
                order.append(name)
            agg[name][0] += 1
            agg[name][1] += ms
        print("per launch group (HIP events on the trainer's stream, one mining call):")
        for name in order:
            n, ms = agg[name]
            note = ""
            if name in flops:
                tf = flops[name] / (ms * 1e-3) / 1e12
                note = "%6.1f TFLOP/s = %4.1f %% of the card's fp32-MFMA rate" % (tf, 100.0 * tf / mfma)
            print("  %-16s x%-2d %9.3f ms  %s" % (name, n, ms, note))
        print("  sum %.3f ms in %d launch groups" % (sum(v[1] for v in agg.values()), sum(v[0] for v in agg.values())))
        mined = gather(sel)
        s = timed(lambda: step_update(mined))
        print("step on the %d mined rows + update: median %.3f ms, best %.3f ms of %d" % (sel.size, s[0], s[1], args.reps))
        o = timed(ohem_iteration)
        print("OHEM iteration (mine + host gather + step + update): median %.3f ms, best %.3f ms of %d" % (o[0], o[1], args.reps))
        p1 = timed(lambda: step_update(plain))
        print("plain iteration, after: median %.3f ms, best %.3f ms of %d (before / after differ by %.1f %%)"
              % (p1[0], p1[1], args.reps, 100.0 * abs(p1[0] - p0[0]) / p0[0]))
        print("OHEM / plain = %.2f (mining is %.1f %% of the OHEM iteration)" % (o[0] / (0.5 * (p0[0] + p1[0])), 100.0 * m[0] / o[0]))
    sol.close()
    ctx.close()


if __name__ == "__main__":
    main()
