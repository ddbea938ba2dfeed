#!/usr/bin/env python3
"""Times az_coco_diag_eval on the val2014-sized synthetic set of the README's COCO row (coco_cases.big_set: 40 504 images x
80 categories).  Median of --reps runs after a warm-up: the kernels (events around the launches), the whole call through the
binding, and in the same process az_coco_eval's whole call on the same inputs -- the existing evaluation, the yardstick,
not a bound -- then the NumPy restatement (tests/cdiag_ref.py) on 1/50 of the images, which the device is checked against
first.  No ratio is asserted.  Not collected by pytest; it lives under tests/ because product code may not import test
infrastructure.

  python tests/perf_cdiag.py [--images 40504] [--reps 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=40504)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import cdiag_ref as C
    import coco_cases
    from aznet_hip import ffi
    ctx = ffi.AzContext(0)
    group = np.arange(80, dtype=np.int32) // 7                             # twelve groups, as COCO's supercategories are
    small = coco_cases.big_set(N=max(1, args.images // 50))
    t0 = time.perf_counter()
    want = C.diag(*C.args(small), class_group=group)
    t_ref = time.perf_counter() - t0
    C.same(ctx.coco_diag_eval(*C.args(small), class_group=group), want, "1/50 of the images")
    case = coco_cases.big_set(N=args.images)
    a = C.args(case)
    D, G = int(case["det_off"][-1]), int(case["gt_off"][-1])
    ctx.coco_diag_eval(*a, class_group=group)                              # warm-up: the arena, the code objects
    ctx.coco_eval(*a)
    kern, whole, coco = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        d = ctx.coco_diag_eval(*a, class_group=group, want_kernel_ms=True)
        whole.append(time.perf_counter() - t0)
        kern.append(d["kernel_ms"] * 1e-3)
        t0 = time.perf_counter()
        v = ctx.coco_eval(*a)
        coco.append(time.perf_counter() - t0)
    assert np.array_equal(d["prec_fix"][0], v["precision"][:, :, :, 0, 2]) and np.array_equal(d["stats_fix"][0], v["stats"][:3])
    res = {"images": args.images, "classes": case["n_classes"], "detections": D, "boxes": G, "reps": args.reps,
           "kernels_s": float(np.median(kern)), "call_s": float(np.median(whole)), "coco_eval_call_s": float(np.median(coco)),
           "numpy_sample_images": small["n_images"], "numpy_sample_detections": int(small["det_off"][-1]),
           "numpy_sample_s": t_ref, "type_table_iou50": d["type_table"][:, 0].sum(0).tolist(),
           "stats_fix": d["stats_fix"].tolist(), "all": {"kernels_s": kern, "call_s": whole, "coco_eval_call_s": coco}}
    print("%d images x %d categories: %d detections, %d boxes" % (args.images, case["n_classes"], D, G))
    print("az_coco_diag_eval kernels : median %.3f ms (min %.3f, max %.3f over %d runs)"
          % (1e3 * np.median(kern), 1e3 * min(kern), 1e3 * max(kern), len(kern)))
    print("az_coco_diag_eval call    : median %.3f ms (min %.3f, max %.3f)" % (1e3 * np.median(whole), 1e3 * min(whole), 1e3 * max(whole)))
    print("az_coco_eval call         : median %.3f ms (min %.3f, max %.3f)" % (1e3 * np.median(coco), 1e3 * min(coco), 1e3 * max(coco)))
    print("NumPy restatement, %d images (%d detections): %.2f s" % (small["n_images"], int(small["det_off"][-1]), t_ref))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
