#!/usr/bin/env python3
"""Multi-scale test pyramids, timed (development tool): a 500x375 image through the full-size synthetic VGG16 and heads
at SCALES = (480, 576, 688, 864, 1200), MAX_SIZE = 2000 (S = 5) and at (600,), MAX_SIZE = 1000 (S = 1), Tz = 0.5:
  front-end + backbone ms (HipAZNet.compute_pyramid: the padded blob and one backbone pass per level),
  search ms (az_propose_pyramid) and head rows per level, projection + dedup us per level (k_first_rois with the
  pyramid projection + k_dedup_rois, device events), az_detect_pyramid ms at 300 proposals; medians of `reps` runs.
Usage: perf_pyramid.py [reps]"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "lib"))
sys.path.insert(0, HERE)
from aznet_hip import ffi, synth            # noqa: E402


def main():
    import torch
    from prop_az import load_net
    from aznet_hip.net import HipDetNet
    from detect.config import cfg
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    net = load_net("synthetic", 0)
    det = HipDetNet(synth.make_det_head(seed=7, **synth.FULL_DET_DIMS), net)
    im = synth.make_image(3, 375, 500)
    for targets, max_size in (((480, 576, 688, 864, 1200), 2000), ((600,), 1000)):
        sizes_min, sizes_max = 375.0, 500.0
        scales = []
        for t in targets:
            s = t / sizes_min
            if np.round(s * sizes_max) > max_size:
                s = max_size / sizes_max
            scales.append(s)
        fb, se, dt, pr_us = [], [], [], []
        p = ffi.AzContext.make_params(375, 500, scales[0], 0.5, batch_size=int(cfg.SEAR.BATCH_SIZE))
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            net.compute_pyramid(im, cfg.PIXEL_MEANS, scales)
            t1 = time.perf_counter()
            net.ctx.set_profiling(2)
            Y, st = net.propose_pyramid(p, scales, want_stats=True)
            t2 = time.perf_counter()
            kt = net.ctx.last_kernel_times()
            net.ctx.set_profiling(0)
            det.detect_pyramid(Y, scales, (375, 500), cfg.DEDUP_BOXES, int(cfg.SEAR.BATCH_SIZE), cfg.EPS)
            t3 = time.perf_counter()
            if r:
                fb.append(1e3 * (t1 - t0)); se.append(1e3 * (t2 - t1)); dt.append(1e3 * (t3 - t2))
                pr_us.append([1e3 * ms for name, lv, ms in kt if name == "rois_dedup"])
        n = st.depth if st.depth < ffi.AZ_MAX_LEVELS else ffi.AZ_MAX_LEVELS
        print("S=%d scales=%s padded blob %s" % (len(scales), ["%.3f" % s for s in scales],
                                                  tuple(net._conv[0].shape)))
        print("  front-end + backbone %.2f ms, search %.2f ms (profiled), detect(300) %.2f ms" %
              (np.median(fb), np.median(se), np.median(dt)))
        print("  rows per level", list(st.level_unique)[:n], "regions", list(st.level_regions)[:n])
        print("  projection + dedup us per level", [round(float(np.median([u[l] for u in pr_us])), 1)
                                                    for l in range(min(len(u) for u in pr_us))])


if __name__ == "__main__":
    main()
