#!/usr/bin/env python3
"""Times az_det_diag_eval on the VOC07-test-sized synthetic set of the README's VOC row (4952 images x 20 classes, about
40 detections and 1.2 boxes per class and image; ddiag_ref.voc07_case).  Median of --reps runs after a warm-up: the
kernels (events around the launches), the whole call, and in the same process az_voc_eval on the same inputs -- the
existing evaluation, the yardstick -- then the NumPy restatement (tests/ddiag_ref.py) on a set of 1/50 of the images
built the same way, which the device is checked against first.  No ratio is asserted.  Not collected by pytest; it lives
under tests/ because product code may not import test infrastructure.

  python tests/perf_ddiag.py [--images 4952] [--reps 5] [--out FILE]
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

CUTS = (0.25, 0.5, 1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ddiag_ref as R
    from aznet_hip import ffi
    ctx = ffi.AzContext(0)
    small = R.voc07_case(max(1, args.images // 50))
    t0 = time.perf_counter()
    want = R.diag_flat(*small, class_group=R.VOC_GROUPS, cuts=CUTS)
    t_ref = time.perf_counter() - t0
    got = ctx.det_diag_eval(*small, class_group=R.VOC_GROUPS, cuts=CUTS)
    for k in ("type", "arg_same", "other_class", "loc_fixed", "gt_claim", "type_table", "miss", "fp_at", "npos"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["ap_fix"], want["ap_fix"], equal_nan=True)
    case = R.voc07_case(args.images)
    D, G = int(case[4][-1]), int(case[7][-1])
    ctx.det_diag_eval(*case, class_group=R.VOC_GROUPS, cuts=CUTS)          # warm-up: the arena, the code objects
    ctx.voc_eval(*case)
    kern, whole, voc = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        d = ctx.det_diag_eval(*case, class_group=R.VOC_GROUPS, cuts=CUTS, want_kernel_ms=True)
        whole.append(time.perf_counter() - t0)
        kern.append(d["kernel_ms"] * 1e-3)
        t0 = time.perf_counter()
        v = ctx.voc_eval(*case)
        voc.append(time.perf_counter() - t0)
    assert np.array_equal(d["ap_fix"][:, 0], v["ap"], equal_nan=True) and np.array_equal(d["npos"], v["npos"])
    res = {"images": args.images, "classes": case[0], "detections": D, "boxes": G, "reps": args.reps,
           "kernels_s": float(np.median(kern)), "call_s": float(np.median(whole)), "voc_eval_call_s": float(np.median(voc)),
           "numpy_sample_images": small[1], "numpy_sample_detections": int(small[4][-1]), "numpy_sample_s": t_ref,
           "type_table": d["type_table"].sum(0).tolist(), "mean_ap_fix": np.nanmean(d["ap_fix"], axis=0).tolist(),
           "all": {"kernels_s": kern, "call_s": whole, "voc_eval_call_s": voc}}
    print("%d images x %d classes: %d detections, %d boxes" % (args.images, case[0], D, G))
    print("az_det_diag_eval kernels : median %.3f ms (min %.3f, max %.3f over %d runs)"
          % (1e3 * np.median(kern), 1e3 * min(kern), 1e3 * max(kern), len(kern)))
    print("az_det_diag_eval call    : median %.3f ms (min %.3f, max %.3f)" % (1e3 * np.median(whole), 1e3 * min(whole), 1e3 * max(whole)))
    print("az_voc_eval call         : median %.3f ms (min %.3f, max %.3f)" % (1e3 * np.median(voc), 1e3 * min(voc), 1e3 * max(voc)))
    print("NumPy restatement, %d images (%d detections): %.2f s" % (small[1], int(small[4][-1]), t_ref))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
