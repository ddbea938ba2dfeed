#!/usr/bin/env python3
"""The truncated-SVD detection head against the full one, timed (a script, not a test): full size (C = 512, n6 = n7 =
4096, 21 classes), 300 proposals on the 38 x 63 map of a 600 x 1000 image, fc6 -> 1024 and fc7 -> 256 (the paper's ranks).

In ONE process: load the full head and time az_detect (whole call from device events on the context's stream, and per
stage from the context's own events), load the compressed head and time it the same way, and once more each (full,
compressed, full, compressed), so that drift of the card shows as a difference between the two rounds.  Prints both
per-stage tables with each stage's FLOPs / bytes as a share of the fp32-MFMA peak (157.3 TF) or of the HBM rate a copy
reaches (6.3 TB/s), the whole-call medians, and the largest difference of cls_prob between the two heads.

The factors of the 4096 x 25088 layer come from the Gram matrix (eigenvectors U of W W^T in float64, L = U_r^T W): the
truncation compress_layer computes, up to rounding, without a float64 SVD of that size.  fc7 (4096 x 4096) goes through
aznet_hip.compress.compress_layer itself, and the Gram route is compared with it there.
Usage: perf_lowrank.py [reps] [r6] [r7]"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "az-net_amd", "lib"))
from aznet_hip import ffi, synth            # noqa: E402

PEAK_TF, HBM_TBS = 157.3, 6.3
ROWS = 300


def boxes_of(seed, n=ROWS, h=600, w=1000):
    rng = np.random.RandomState(seed)
    x1 = rng.uniform(0, w - 40, n)
    y1 = rng.uniform(0, h - 40, n)
    return np.stack([x1, y1, np.minimum(x1 + rng.uniform(16, 600, n), w - 1), np.minimum(y1 + rng.uniform(16, 400, n), h - 1)], 1)


def gram_factors(W, r):
    """(L [r, in], U [out, r]) float32 and ||W - U L|| / ||W|| from the eigenvectors of W W^T (float64, on the GPU)."""
    import torch
    Wd = torch.from_numpy(np.ascontiguousarray(W)).cuda().double()
    ev, U = torch.linalg.eigh(Wd @ Wd.T)
    U = U[:, torch.argsort(ev, descending=True)[:r]].contiguous()
    Lf = U.T @ Wd
    err = float(torch.linalg.norm(Wd - U @ Lf) / torch.linalg.norm(Wd))
    return Lf.float().cpu().numpy(), U.float().cpu().numpy(), err


def stage_model(r6, r7, rows, low):
    """{stage: (FLOPs, bytes)} of one pass from the shapes (weights read once, activations and slabs written and read).
    The chunk counts are the library's: head_sizes_ref.fc_split restates azk_fc_split (the header's 1 / 2 / 8 / 16 rule,
    held to the device by tests/test_gpu_head_sizes.py), ffi.lowrank_split asks az_lowrank_split; the tail's 8 is
    AZK_TAIL_SPLIT (az_dev.h)."""
    from head_sizes_ref import fc_split
    d = synth.FULL_DET_DIMS
    K6, n6, n7, NO = d["C"] * 49, d["n6"], d["n7"], 5 * d["ncls"]
    f = lambda m, nn, k: 2.0 * m * nn * k          # noqa: E731
    S6, S7, ST = fc_split(K6), fc_split(n6), 8
    m = {"det_roi_pool": (0.0, 4.0 * rows * K6), "det_tail_gemm": (f(rows, NO, n7), 4.0 * (NO * n7 + rows * n7 + ST * rows * NO)),
         "det_epilogue": (0.0, 4.0 * ST * rows * NO)}
    if low:
        SL6, SL7 = ffi.lowrank_split(K6, r6), ffi.lowrank_split(n6, r7)
        m.update({"det_fc6_L": (f(rows, r6, K6), 4.0 * (r6 * K6 + rows * K6 + SL6 * rows * r6)),
                  "det_fc6_L_reduce": (0.0, 4.0 * (SL6 + 1) * rows * r6),
                  "det_fc6_U": (f(rows, n6, r6), 4.0 * (n6 * r6 + rows * r6 + rows * n6)),
                  "det_fc7_L": (f(rows, r7, n6), 4.0 * (r7 * n6 + rows * n6 + SL7 * rows * r7)),
                  "det_fc7_L_reduce": (0.0, 4.0 * (SL7 + 1) * rows * r7),
                  "det_fc7_U": (f(rows, n7, r7), 4.0 * (n7 * r7 + rows * r7 + rows * n7))})
    else:
        m.update({"det_fc6_gemm": (f(rows, n6, K6), 4.0 * (n6 * K6 + rows * K6 + S6 * rows * n6)),
                  "det_fc6_reduce": (0.0, 4.0 * (S6 + 1) * rows * n6),
                  "det_fc7_gemm": (f(rows, n7, n6), 4.0 * (n7 * n6 + rows * n6 + S7 * rows * n7)),
                  "det_fc7_reduce": (0.0, 4.0 * (S7 + 1) * rows * n7)})
    return m


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    r6 = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    r7 = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    full = synth.make_det_head(seed=7, **synth.FULL_DET_DIMS)
    t0 = time.perf_counter()
    low = {k: v for k, v in full.items() if k not in ("W6", "W7")}
    from aznet_hip import compress
    low["L6"], low["U6"], err = gram_factors(full["W6"], r6)
    print("fc6 -> rank %d (Gram matrix): ||W - U L|| / ||W|| = %.4f   (%.1f s)" % (r6, err, time.perf_counter() - t0), flush=True)
    # fc7 (4096 x 4096) through the shipped compressor, and the Gram route held against it through the products U L
    low["L7"], low["U7"] = compress.compress_layer(full["W7"], r7)
    print("fc7 -> rank %d (compress_layer): ||W - U L|| / ||W|| = %.4f   (%.1f s)"
          % (r7, compress.rel_error(full["W7"], low["L7"], low["U7"]), time.perf_counter() - t0), flush=True)
    Lg, Ug, _ = gram_factors(full["W7"], r7)
    ref = low["U7"].astype(np.float64) @ low["L7"].astype(np.float64)
    print("fc7: Gram-matrix factors against compress_layer's, max |U L - U L| / max |U L| = %.2e"
          % (np.abs(Ug.astype(np.float64) @ Lg.astype(np.float64) - ref).max() / np.abs(ref).max()), flush=True)
    ctx = ffi.AzContext(0)
    ctx.load_head(synth.make_head(seed=1234, **synth.FULL_DIMS))       # (set_feature_map needs one)
    fh, fw = synth.conv_out_size(600), synth.conv_out_size(1000)
    fmap = torch.from_numpy(synth.make_feature_map(20, 512, fh, fw)).cuda().contiguous(memory_format=torch.channels_last)
    boxes = boxes_of(100)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stream = torch.cuda.ExternalStream(ctx.stream_handle())
    ctx.set_feature_map(fmap, producer_done=True)

    def run():
        return ctx.detect(boxes, 1.0, 600, 1000, batch_size=10000)

    def whole():
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            ev[0].record(stream)
            run()
            ev[1].record(stream)
            ev[1].synchronize()
            out.append(ev[0].elapsed_time(ev[1]))
        return np.array(out)

    def stages():
        ctx.set_profiling(2)
        acc = {}
        for _ in range(reps):
            run()
            for name, _, ms in ctx.last_kernel_times():
                acc.setdefault(name, []).append(ms)
        ctx.set_profiling(0)
        return {k: float(np.median(v)) for k, v in acc.items()}

    probs, med = {}, {}
    for rnd in (1, 2):
        for tag, head in (("full", full), ("low rank %d / %d" % (r6, r7), low)):
            ctx.load_det_head(head)
            ctx.set_feature_map(fmap, producer_done=True)
            for _ in range(3):
                probs[tag] = run()[0]
            t = whole()
            st = stages()
            med.setdefault(tag, []).append(float(np.median(t)))
            rows = 0
            print("\n== %s, round %d: az_detect of %d proposals, whole call %.3f ms median (%.3f - %.3f, %d reps)"
                  % (tag, rnd, ROWS, np.median(t), t.min(), t.max(), reps))
            model = stage_model(r6, r7, ROWS, tag != "full")
            print("   %-18s %9s %10s %10s" % ("stage", "us", "of MFMA", "of HBM"))
            for name, ms in st.items():
                fl, by = model.get(name, (0.0, 0.0))
                print("   %-18s %9.1f %9.1f%% %9.1f%%" % (name, 1e3 * ms, 100 * fl / (ms * 1e-3) / 1e12 / PEAK_TF if ms else 0,
                                                          100 * by / (ms * 1e-3) / 1e12 / HBM_TBS if ms else 0))
                rows += ms
            print("   %-18s %9.1f" % ("sum of stages", 1e3 * rows), flush=True)
    a, b = probs["full"], probs["low rank %d / %d" % (r6, r7)]
    print("\nwhole-call medians (ms): " + "; ".join("%s: %s" % (k, ", ".join("%.3f" % x for x in v)) for k, v in med.items()))
    print("largest |cls_prob(full) - cls_prob(low rank)| on the synthetic head: %.4f (argmax agrees on %d of %d proposals)"
          % (float(np.abs(a - b).max()), int((a.argmax(1) == b.argmax(1)).sum()), a.shape[0]))
    ctx.close()


if __name__ == "__main__":
    main()
