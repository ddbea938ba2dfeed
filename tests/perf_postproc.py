#!/usr/bin/env python3
"""Times the detection post-processing on a VOC07-test-sized synthetic set: 4952 images x 20 classes, each group 0 .. 100
clustered boxes (--distinct different groups, drawn with repetition).  Per variant the kernel time (HIP events around the
launch groups, one call) and the whole call through the binding (list of arrays in, list of arrays out; median, fastest and
slowest of --reps after --warmup calls):
  hard NMS through az_nms_batched (the yardstick: the code apply_nms has always called), linear Soft-NMS, gaussian Soft-NMS,
  linear Soft-NMS + box voting (two calls), and the NumPy restatement (tests/postproc_ref.py) on the first --subset groups.
The yardstick is measured before and after the others (a drifting clock shows as a difference between the two).  Not
collected by pytest; it lives under tests/ because it uses the tests' case builders.

  python tests/perf_postproc.py [--reps 7] [--warmup 2] [--images 4952] [--classes 20] [--subset 200]"""
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


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=2000)
    ap.add_argument("--subset", type=int, default=200)
    args = ap.parse_args()
    import postproc_ref as P
    from aznet_hip import ffi
    ctx = ffi.AzContext(0)
    rng = np.random.Generator(np.random.PCG64(1))
    sizes = rng.integers(0, 101, args.distinct)
    distinct = [P.clustered_group(7000 + i, int(n), clusters=max(1, int(n) // 10)) for i, n in enumerate(sizes)]
    sets = [distinct[i] for i in rng.integers(0, args.distinct, args.images * args.classes)]
    total = sum(d.shape[0] for d in sets)
    print("%d groups (%d images x %d classes), %d boxes, %.1f per group, at most %d"
          % (len(sets), args.images, args.classes, total, total / len(sets), max(d.shape[0] for d in sets)))
    state = {}

    def nms():
        state["keeps"] = ctx.nms_batched(sets, 0.3)

    def soft(method):
        state["picked"] = ctx.soft_nms_batched(sets, method, 0.3, 0.5, 0.001)

    def soft_vote():
        soft("linear")
        state["voted"] = ctx.box_vote_batched(sets, [p[0] for p in state["picked"]], 0.8)

    def kernels(fn):
        ctx.set_profiling(2)
        fn()
        t = ctx.last_kernel_times()
        ctx.set_profiling(0)
        return ", ".join("%s %.3f ms" % (n, ms) for n, _, ms in t), sum(ms for _, _, ms in t)

    rows = [("hard NMS, az_nms_batched (before)", nms), ("linear Soft-NMS", lambda: soft("linear")),
            ("gaussian Soft-NMS", lambda: soft("gaussian")), ("linear Soft-NMS + box voting", soft_vote),
            ("hard NMS, az_nms_batched (after)", nms)]
    first = None
    for name, fn in rows:
        med, lo, hi = timed(fn, args.reps, args.warmup)
        kt, ks = kernels(fn)
        kept = sum(len(k) for k in state["keeps"]) if fn is nms else sum(len(p[0]) for p in state["picked"])
        print("%-36s whole call: median %8.2f ms (fastest %8.2f, slowest %8.2f of %d); kernels %8.3f ms [%s]; %d boxes kept"
              % (name, med, lo, hi, args.reps, ks, kt, kept))
        if fn is nms:
            if first is None:
                first = med
            else:
                print("the yardstick before / after differ by %.1f %%" % (100.0 * abs(med - first) / first))
    sub = sets[:args.subset]
    t0 = time.perf_counter()
    want = [P.soft_nms_ref(d, "linear", 0.3, 0.5, 0.001) for d in sub]
    t1 = time.perf_counter()
    votes = [P.box_vote_ref(d, w[0], 0.8) for d, w in zip(sub, want)]
    t2 = time.perf_counter()
    ok = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(state["picked"], want)) and \
        all(np.array_equal(a, b) for a, b in zip(state["voted"], votes))
    print("NumPy restatement on the first %d groups: linear Soft-NMS %.1f ms (%.3f ms per group: %.1f s for the set), voting "
          "%.1f ms (%.3f ms per group); the device's results on them %s"
          % (len(sub), (t1 - t0) * 1e3, (t1 - t0) * 1e3 / len(sub), (t1 - t0) / len(sub) * len(sets), (t2 - t1) * 1e3,
             (t2 - t1) * 1e3 / len(sub), "equal them" if ok else "DIFFER"))
    ctx.close()


if __name__ == "__main__":
    main()
