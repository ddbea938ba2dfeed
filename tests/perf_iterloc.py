#!/usr/bin/env python3
"""Iterative box localisation, timed (a script, not a test): the full-size detection head (C = 512, n6 = n7 = 4096, 21
classes), 300 proposals on the 38 x 63 map of a 600 x 1000 image, rounds 2 and 3, cfg.TEST's default score (0.05) and cap
(1000 rows a round) -- and once more with score 0, where the cap binds and every round runs 1000 rows.

In ONE process, per setting:
  * az_detect_iter with the rounds' 4-byte row counts read back (the default), host wall clock of the whole call;
  * az_detect_iter on a context created under AZ_ITERLOC_SYNC=0 (no read-back, every round enqueued at max_rows rows);
  * the host loop over az_detect that a caller had to write before the entry existed (tests/iterloc_ref.iter_ref:
    download, select in NumPy, az_detect on the selected boxes, take the class column) -- the yardstick, and what the
    parent commit can run;
  * one-shot az_detect, for scale;
  * the kernels of the read-back variant round by round from the context's own events.
The three loops are held bit for bit against each other before anything is timed.  The calls are host in, host out, so the
wall clock of a call is what its caller waits for.  Usage: perf_iterloc.py [reps]"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "az-net_amd", "lib"))
sys.path.insert(0, HERE)
from aznet_hip import ffi, synth            # noqa: E402
import iterloc_ref as R                     # noqa: E402

ROWS, IM_H, IM_W = 300, 600, 1000


def boxes_of(seed, n=ROWS, h=IM_H, w=IM_W):
    rng = np.random.RandomState(seed)
    x1 = rng.uniform(0, w - 40, n)
    y1 = rng.uniform(0, h - 40, n)
    return np.stack([x1, y1, np.minimum(x1 + rng.uniform(16, 600, n), w - 1), np.minimum(y1 + rng.uniform(16, 400, n), h - 1)], 1)


def make_context(head, fmap, sync):
    if not sync:
        os.environ["AZ_ITERLOC_SYNC"] = "0"                  # (read once, by az_create)
    try:
        ctx = ffi.AzContext(0, max_regions=4096, gemm_mode=0)
    finally:
        os.environ.pop("AZ_ITERLOC_SYNC", None)
    ctx.load_head(synth.make_head(seed=1234, **synth.FULL_DIMS))       # (set_feature_map needs one)
    ctx.load_det_head(head)
    ctx.set_feature_map(fmap, producer_done=True)
    return ctx


def wall(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return np.array(out)


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    head = synth.make_det_head(seed=7, **synth.FULL_DET_DIMS)
    fh, fw = synth.conv_out_size(IM_H), synth.conv_out_size(IM_W)
    fmap = torch.from_numpy(synth.make_feature_map(20, 512, fh, fw)).cuda().contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
    boxes = boxes_of(100)
    ctxs = {"read-back": make_context(head, fmap, True), "device count": make_context(head, fmap, False)}
    c0 = ctxs["read-back"]
    det = lambda b: c0.detect(b, 1.0, IM_H, IM_W)      # noqa: E731
    for _ in range(3):
        s1 = det(boxes)[0]
    t = wall(lambda: det(boxes), reps)
    print("one-shot az_detect of %d proposals: %.3f ms median (%.3f - %.3f, %d reps); class scores %.4f .. %.4f"
          % (ROWS, np.median(t), t.min(), t.max(), reps, s1[:, 1:].min(), s1[:, 1:].max()), flush=True)
    for ms, mr in ((0.05, 1000), (0.0, 1000)):
        for rounds in (2, 3):
            want = R.iter_ref(det, boxes, rounds, ms, mr)
            line = {}
            for tag, c in ctxs.items():
                fn = lambda c=c: c.detect_iter(boxes, 1.0, IM_H, IM_W, rounds, ms, mr)      # noqa: E731
                for _ in range(3):
                    got = fn()
                diff = R.same(got, want)
                assert diff is None, "%s differs from the host loop in %s" % (tag, diff)
                line[tag] = wall(fn, reps)
            line["host loop over az_detect"] = wall(lambda: R.iter_ref(det, boxes, rounds, ms, mr), reps)
            print("\n== rounds %d, min_score %.2f, max_rows %d: rows per extra round %s (bit for bit the host loop)"
                  % (rounds, ms, mr, want[2]["count"].tolist()))
            for tag, v in line.items():
                print("   %-28s %8.3f ms median (%.3f - %.3f)" % (tag, np.median(v), v.min(), v.max()))
            # the read-back variant's launches, round by round (level = the round the launch belongs to - 1; 0: round 1)
            c0.set_profiling(2)
            acc = {}
            for _ in range(reps):
                c0.detect_iter(boxes, 1.0, IM_H, IM_W, rounds, ms, mr)
                rnd = 1
                for name, _, k_ms in c0.last_kernel_times():
                    if name == "iter_select":
                        rnd += 1
                    acc.setdefault((rnd, name), []).append(k_ms)
            c0.set_profiling(0)
            for rnd in range(1, rounds + 1):
                names = [(k[1], float(np.median(v))) for k, v in acc.items() if k[0] == rnd]
                if names:
                    print("   round %d kernels (us): %s; sum %.1f" % (rnd, ", ".join("%s %.1f" % (n, 1e3 * v) for n, v in names),
                                                                   1e3 * sum(v for _, v in names)), flush=True)
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
