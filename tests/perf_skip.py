#!/usr/bin/env python3
"""Times the skip-connection detector's front (az_skip.hip) at the launch sizes: 300 proposals of a 600 x 1000 image, maps
conv3_3 [150][250][256], conv4_3 [75][125][512], conv5_3 [38][63][512], the 1280 -> 512 1x1 convolution, the full-size
Fast R-CNN head (fc6 4096, fc7 4096, 21 classes).  Kernel time per stage from the context's own events (az_set_profiling 2),
median of --reps calls after a warm-up.  With profiling on the pool-norm kernel runs as ONE LAUNCH PER SOURCE (grid
rows x 1) so that each source can be timed; az_detect_skip otherwise runs it as one launch over (rows x sources): the
per-source figures are of that other launch shape, and their sum is an upper estimate of the shipped launch.  The whole
call's wall time is taken in a separate pass with profiling off, i.e. on the shipped launches:

    pool-norm per source | the 1x1 convolution | the unchanged head (fc6 .. epilogue) | az_detect_skip, whole call

beside the plain az_detect on conv5_3 alone (RoIPool + the same head) as the reference point for the extra cost, and the 1x1
convolution's share of the fp32-MFMA rate that az_measure_box reports on this device (FLOPs from the shapes: unique rows x
49 x 2 x 1280 x 512).  No figure is asserted.  Not collected by pytest.

  python tests/perf_skip.py [--reps 20] [--proposals 300] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "az-net_amd", "lib"), REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def boxes_of(seed, n, h=600, w=1000):
    rng = np.random.RandomState(seed)
    x1 = rng.uniform(0, w - 40, n)
    y1 = rng.uniform(0, h - 40, n)
    return np.stack([x1, y1, np.minimum(x1 + rng.uniform(16, 600, n), w - 1), np.minimum(y1 + rng.uniform(16, 400, n), h - 1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--proposals", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from aznet_hip import ffi, synth
    ctx = ffi.AzContext(0)
    ctx.load_head(synth.make_head(seed=1234, **synth.FULL_DIMS))          # (az_detect's set_feature_map needs one)
    ctx.load_det_head(synth.make_det_head(seed=7, **synth.FULL_DET_DIMS))
    ctx.load_skip_front(synth.make_skip_front(seed=9))
    sizes = []
    h, w = 600, 1000
    for _ in range(4):
        h, w = (h + 1) // 2, (w + 1) // 2
        sizes.append((h, w))
    maps = [torch.from_numpy(synth.make_feature_map(30 + i, C, *sizes[k])).cuda().contiguous(memory_format=torch.channels_last)
            for i, (C, k) in enumerate(zip(synth.SKIP_CS, (1, 2, 3)))]
    boxes = boxes_of(100, args.proposals)
    P = boxes.shape[0]
    unique = {d: len(ctx.roi_dedup(boxes, 1.0, dedup=d)[1]) for d in (0.5, 1. / 16.)}
    tf_peak, _ = ctx.measure_box()

    def stages(call):
        """{kernel name: median ms} with per-launch profiling on, and the whole call's wall time (median) with it off."""
        call()
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            wall.append(time.perf_counter() - t0)
        ctx.set_profiling(2)
        per = {}
        for _ in range(args.reps):
            call()
            acc = {}
            for name, _, ms in ctx.last_kernel_times():
                acc[name] = acc.get(name, 0.0) + ms
            for name, ms in acc.items():
                per.setdefault(name, []).append(ms)
        ctx.set_profiling(0)
        return {k: float(np.median(v)) for k, v in per.items()}, float(np.median(wall)) * 1e3

    ctx.set_skip_maps(maps)
    skip, skip_wall = stages(lambda: ctx.detect_skip(boxes, 1.0, 600, 1000, dedup=0.5, batch_size=1000))
    ctx.set_feature_map(maps[2], producer_done=True)
    plain, plain_wall = stages(lambda: ctx.detect(boxes, 1.0, 600, 1000, dedup=1. / 16., batch_size=1000))
    head = ("det_fc6_gemm", "det_fc6_reduce", "det_fc7_gemm", "det_fc7_reduce", "det_tail_gemm", "det_epilogue")
    pool = [skip.get("skip_pool_norm_%d" % i, float("nan")) for i in range(3)]
    conv = skip.get("skip_conv_gemm", float("nan"))
    flop = 2.0 * unique[0.5] * 49 * sum(synth.SKIP_CS) * 512
    res = {"proposals": P, "unique_rois_dedup_0.5": unique[0.5], "unique_rois_dedup_1_16": unique[1. / 16.], "reps": args.reps,
           "pool_norm_ms": dict(zip(synth.SKIP_NAMES, pool)), "conv_ms": conv,
           "conv_tflops": flop / (conv * 1e-3) / 1e12, "mfma_f32_tflops_measured": tf_peak,
           "conv_share_of_measured_peak": flop / (conv * 1e-3) / 1e12 / tf_peak if tf_peak else float("nan"),
           "head_ms_skip": sum(skip.get(k, 0.0) for k in head), "head_ms_plain": sum(plain.get(k, 0.0) for k in head),
           "roi_pool_ms_plain": plain.get("det_roi_pool", float("nan")),
           "kernels_ms_skip": sum(skip.values()), "kernels_ms_plain": sum(plain.values()),
           "call_ms_skip": skip_wall, "call_ms_plain": plain_wall, "stages_skip": skip, "stages_plain": plain}
    print("%d proposals: %d unique rois at dedup 0.5 (skip), %d at 1/16 (plain)" % (P, unique[0.5], unique[1. / 16.]))
    for n, ms in zip(synth.SKIP_NAMES, pool):
        print("pool-norm %-8s          : %.3f ms   (its own launch; shipped: one launch for all sources)" % (n, ms))
    print("1x1 convolution             : %.3f ms = %.1f TF, %.2f of the measured fp32-MFMA rate (%.1f TF)"
          % (conv, res["conv_tflops"], res["conv_share_of_measured_peak"], tf_peak))
    print("head behind the front       : %.3f ms   (plain az_detect: %.3f ms + RoIPool %.3f ms)"
          % (res["head_ms_skip"], res["head_ms_plain"], res["roi_pool_ms_plain"]))
    print("all kernels                 : skip %.3f ms, plain %.3f ms" % (res["kernels_ms_skip"], res["kernels_ms_plain"]))
    print("whole call, profiling off   : skip %.3f ms, plain %.3f ms" % (skip_wall, plain_wall))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f)
    ctx.close()


if __name__ == "__main__":
    main()
