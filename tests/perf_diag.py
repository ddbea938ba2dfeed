#!/usr/bin/env python3
"""Times az_diag_eval against its NumPy restatement (tests/diag_ref.py) on a VOC07-test-sized synthetic set: 4952 images,
300 proposals each, anchors (1-900) and objects (0-12) per image drawn as in diag_ref.random_case.  Median of --reps runs
after a warm-up: the two kernels (events around the launches), the whole call from per-image lists (packing, copies,
kernels, copies back), the call on arrays packed beforehand, and the restatement.  Checks first that both give the same
tables.  No ratio is asserted.  Not collected by pytest; it lives under tests/ because product code may not import test
infrastructure.

  python tests/perf_diag.py [--images 4952] [--reps 5] [--ref-reps 5] [--out FILE]
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
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import diag_ref as R
    from aznet_hip import ffi
    ctx = ffi.AzContext(0)
    case = R.perf_case(args.images)
    A, G, P = (sum(x.shape[0] for x in case[k]) for k in ("anchors", "gt", "props"))
    lists = (case["anchors"], case["zoom"], case["level"], case["gt"], case["props"])

    def call(ms=False):
        return ctx.diag_eval(*lists, R.TZ_EXACT, R.EMB_REG, R.EMB_OBJ, want_kernel_ms=ms)
    got = call()                                                  # warm-up: the arena, the code objects
    R.assert_same(got, R.diag_eval(case, R.TZ_EXACT), "perf set")
    packed = (np.vstack(case["anchors"]), np.concatenate(case["zoom"]), np.concatenate(case["level"]), got["anc_off"],
              np.vstack(case["gt"]), got["gt_off"], np.vstack(case["props"]), got["prop_off"])
    whole, kern, pre, ref = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        d = call(ms=True)
        whole.append(time.perf_counter() - t0)
        kern.append(d["kernel_ms"] * 1e-3)
        a, z, lv, ao, g, go, p, po = packed
        t0 = time.perf_counter()
        ctx.diag_eval_packed(a, z, lv, ao, g, go, p, po, R.TZ_EXACT, R.EMB_REG, R.EMB_OBJ, 0.5, R.CUTS, R.EDGES)
        pre.append(time.perf_counter() - t0)
    for _ in range(args.ref_reps):
        t0 = time.perf_counter()
        R.diag_eval(case, R.TZ_EXACT)
        ref.append(time.perf_counter() - t0)
    res = {"images": args.images, "anchors": A, "objects": G, "proposals": P, "reps": args.reps, "ref_reps": args.ref_reps,
           "kernels_s": float(np.median(kern)), "call_packed_s": float(np.median(pre)), "call_lists_s": float(np.median(whole)),
           "numpy_s": float(np.median(ref)),
           "all": {"kernels_s": kern, "call_packed_s": pre, "call_lists_s": whole, "numpy_s": ref}}
    print("%d images: %d anchors, %d objects, %d proposals" % (args.images, A, G, P))
    print("kernels (two launches)          : median %.3f ms (min %.3f, max %.3f over %d runs)"
          % (1e3 * np.median(kern), 1e3 * min(kern), 1e3 * max(kern), len(kern)))
    print("whole call, arrays packed before: median %.3f ms (min %.3f, max %.3f)" % (1e3 * np.median(pre), 1e3 * min(pre), 1e3 * max(pre)))
    print("whole call, per-image lists     : median %.3f ms (min %.3f, max %.3f)" % (1e3 * np.median(whole), 1e3 * min(whole), 1e3 * max(whole)))
    print("NumPy restatement               : median %.3f s  (min %.3f, max %.3f over %d runs)"
          % (np.median(ref), min(ref), max(ref), len(ref)))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
