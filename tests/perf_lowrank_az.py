#!/usr/bin/env python3
"""The AZ head with int6 at rank r6 against the full head, timed (a script, not a test): full size (C = 512, n6 = 4096,
n7 = 1024 + 256), in ONE process.

The searches: the Tz = 0 search of a 600 x 1000 image (688 rows in one pass) and BASELINE config 4 (800 x 1200 at scale
     0.75, 2672 rows), full head, compressed head, full, compressed; per search the wall time (launch to fetch, one search in
     flight) and the per-stage medians from the context's events with each stage's FLOPs / bytes as a share of the
     fp32-MFMA peak (157.3 TF) or of the HBM rate a copy reaches (6.3 TB/s).

The factors of the 4096 x 25088 layer come from the Gram matrix, as tests/perf_lowrank.py's fc6.  The stream of distinct
images at a tuned threshold (bench.py: stream_tz) is not run here.
Usage: perf_lowrank_az.py [reps] [r6]"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "az-net_amd", "lib"))
sys.path.insert(0, HERE)
from aznet_hip import ffi, synth            # noqa: E402
from perf_lowrank import gram_factors, PEAK_TF, HBM_TBS            # noqa: E402

SEARCHES = (("Tz = 0 search, 600 x 1000 (688 rows)", (600, 1000, 1.0), 688),
            ("config 4, 800 x 1200 at 0.75 (2672 rows)", (800, 1200, 0.75), 2672))


def stage_model(r6, rows, low):
    """{stage: (FLOPs, bytes)} of one pass from the shapes (weights read once, activations and slabs written and read)."""
    from head_sizes_ref import fc_split
    d = synth.FULL_DIMS
    K6, n6, n7 = d["C"] * 49, d["n6"], d["n71"] + d["n72"]
    f = lambda m, nn, k: 2.0 * m * nn * k          # noqa: E731
    S6, S7 = fc_split(K6), fc_split(n6)
    m = {"roi_pool": (0.0, 4.0 * rows * K6), "fc7_gemm": (f(rows, n7, n6), 4.0 * (n7 * n6 + rows * n6 + S7 * rows * n7)),
         "tail": (f(rows, 56, n7), 4.0 * (S7 + 1) * rows * n7)}
    if low:
        SL = ffi.az_lowrank_split(K6, r6)
        m.update({"fc6_L": (f(rows, r6, K6), 4.0 * (r6 * K6 + rows * K6 + SL * rows * r6)),
                  "fc6_L_reduce": (0.0, 4.0 * (SL + 1) * rows * r6),
                  "fc6_U": (f(rows, n6, r6), 4.0 * (n6 * r6 + rows * r6 + rows * n6))})
    else:
        m.update({"fc6_gemm": (f(rows, n6, K6), 4.0 * (n6 * K6 + rows * K6 + S6 * rows * n6)),
                  "fc6_reduce": (0.0, 4.0 * (S6 + 1) * rows * n6)})
    return m


def stage_medians(ctx, run, reps):
    ctx.set_profiling(2)
    acc = {}
    for _ in range(reps):
        run()
        for name, _, ms in ctx.last_kernel_times():
            acc.setdefault(name, []).append(ms)
    ctx.set_profiling(0)
    return {k: float(np.median(v)) for k, v in acc.items()}


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    r6 = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    full = synth.make_head(seed=1234, **synth.FULL_DIMS)
    t0 = time.perf_counter()
    low = {k: v for k, v in full.items() if k != "W6"}
    low["L6"], low["U6"], err = gram_factors(full["W6"], r6)
    print("int6 -> rank %d (Gram matrix): ||W - U L|| / ||W|| = %.4f   (%.1f s); L-stage split %d"
          % (r6, err, time.perf_counter() - t0, ffi.az_lowrank_split(512 * 49, r6)), flush=True)
    fh, fw = synth.conv_out_size(600), synth.conv_out_size(1000)
    fmap = torch.from_numpy(synth.make_feature_map(20, 512, fh, fw)).cuda().contiguous(memory_format=torch.channels_last)

    # ---- the searches -------------------------------------------------------------------------------------------------
    ctx = ffi.AzContext(0, max_regions=4096)
    med = {}
    for rnd in (1, 2):
        for tag, head in (("full", full), ("low rank %d" % r6, low)):
            ctx.load_head(head)
            for name, (h, w, sc), rows in SEARCHES:
                mh, mw = synth.conv_out_size(int(round(h * sc))), synth.conv_out_size(int(round(w * sc)))
                fm = torch.from_numpy(synth.make_feature_map(4, 512, mh, mw)).cuda().contiguous(memory_format=torch.channels_last)
                p = ffi.AzContext.make_params(h, w, sc, 0.0)

                def run():
                    ctx.propose_launch(p, fmap=fm, producer_done=True)
                    return ctx.propose_fetch(want_stats=True)
                for _ in range(6):
                    _, st = run()
                t = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    a = time.perf_counter()
                    run()
                    t.append(1e3 * (time.perf_counter() - a))
                t = np.array(t)
                stg = stage_medians(ctx, run, max(4, reps // 4))
                med.setdefault((tag, name), []).append(float(np.median(t)))
                print("\n== %s, %s, round %d: %.3f ms median wall (%.3f - %.3f, %d reps); passes %s"
                      % (tag, name, rnd, np.median(t), t.min(), t.max(), reps, [int(st.pass_rows[i]) for i in range(st.n_passes)]))
                model = stage_model(r6, rows, tag != "full")
                print("   %-14s %9s %10s %10s" % ("stage", "us", "of MFMA", "of HBM"))
                for nm, ms in stg.items():
                    fl, by = model.get(nm, (0.0, 0.0))
                    if nm in model:
                        print("   %-14s %9.1f %9.1f%% %9.1f%%" % (nm, 1e3 * ms, 100 * fl / (ms * 1e-3) / 1e12 / PEAK_TF if ms else 0,
                                                                  100 * by / (ms * 1e-3) / 1e12 / HBM_TBS if ms else 0))
                sys.stdout.flush()
    print("\nwall medians (ms): " + "; ".join("%s, %s: %s" % (k[0], k[1], ", ".join("%.3f" % x for x in v)) for k, v in med.items()))
    ctx.close()


if __name__ == "__main__":
    main()
