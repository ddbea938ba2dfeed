#!/usr/bin/env python3
"""Detection over saved proposals, timed (development tool):
  1. az_detect image by image against az_detect_batch over B images (full-size Fast R-CNN head, 300 proposals per
     600x1000 image, seeded 512-channel maps), from device events on the context's stream: ms per image, and fc6's
     share of the fp32 MFMA peak (157.3 TF) with FLOPs from the shapes (unique rows x 2 x 25088 x 4096);
  2. test_net over synthetic_600x1000_<N> (full-size synthetic VGG16 + head) at cfg.TEST.BATCH_IMAGES 1 and 8: images/s.
Usage: perf_det.py [reps] [N]"""
import io
import os
import pickle
import sys
import tempfile
import time
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "lib"))
sys.path.insert(0, HERE)
from aznet_hip import ffi, synth            # noqa: E402

PEAK_TF = 157.3


def boxes_of(seed, n=300, h=600, w=1000):
    rng = np.random.RandomState(seed)
    x1 = rng.uniform(0, w - 40, n)
    y1 = rng.uniform(0, h - 40, n)
    return np.stack([x1, y1, np.minimum(x1 + rng.uniform(16, 600, n), w - 1), np.minimum(y1 + rng.uniform(16, 400, n), h - 1)], 1)


def head_pass(reps):
    import torch
    ctx = ffi.AzContext(0)
    ctx.load_head(synth.make_head(seed=1234, **synth.FULL_DIMS))       # (set_feature_map, for az_detect, needs one)
    ctx.load_det_head(synth.make_det_head(seed=7, **synth.FULL_DET_DIMS))
    fh, fw = synth.conv_out_size(600), synth.conv_out_size(1000)
    maps = [torch.from_numpy(synth.make_feature_map(20 + k, 512, fh, fw)).cuda().contiguous(memory_format=torch.channels_last)
            for k in range(16)]
    boxes = [boxes_of(100 + k) for k in range(16)]
    flop = 2.0 * 25088 * 4096 * 300
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    stream = torch.cuda.ExternalStream(ctx.stream_handle())

    def timed(fn):
        fn()
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            ev[0].record(stream)
            fn()
            ev[1].record(stream)
            ev[1].synchronize()
            out.append(ev[0].elapsed_time(ev[1]))
        return np.array(out)

    def alone(B):
        def f():
            for k in range(B):
                ctx.set_feature_map(maps[k], producer_done=True)
                ctx.detect(boxes[k], 1.0, 600, 1000, batch_size=10000)
        return f

    def batch(B):
        return lambda: ctx.detect_batch(maps[:B], boxes[:B], [1.0] * B, [(600, 1000)] * B, batch_size=10000)
    print("B  | az_detect ms/img (median, min-max) | az_detect_batch ms/img (median, min-max) | fc6 share of peak alone / batch")
    for B in (1, 4, 8, 16):
        ta = timed(alone(B)) / B
        tb = timed(batch(B)) / B
        # fc6 kernel time per image from the context's own events (each call clears them: the last image alone, the
        # whole pass of the batch)
        ctx.set_profiling(2)
        alone(B)()
        k_a = sum(ms for n, _, ms in ctx.last_kernel_times() if n == "det_fc6_gemm")
        batch(B)()
        k_b = sum(ms for n, _, ms in ctx.last_kernel_times() if n == "det_fc6_gemm") / B
        ctx.set_profiling(0)
        print("%2d | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.2f / %.2f" % (
            B, np.median(ta), ta.min(), ta.max(), np.median(tb), tb.min(), tb.max(),
            flop / (k_a * 1e-3) / 1e12 / PEAK_TF if k_a else float("nan"),
            flop / (k_b * 1e-3) / 1e12 / PEAK_TF if k_b else float("nan")))
    ctx.close()


def dataset(n):
    from datasets.factory import get_imdb
    from detect import config as C
    from detect import test as T
    import test_det_net
    C.cfg_set_path("perf_det")
    net = test_det_net.load_frcnn_net("synthetic:7", 0)
    imdb = get_imdb("synthetic_600x1000_%d" % n)
    tmp = tempfile.mkdtemp()
    pf = os.path.join(tmp, "proposals.pkl")
    with open(pf, "wb") as f:
        pickle.dump({"boxes": [boxes_of(i) for i in range(n)], "time": 0.0, "recall": 0}, f)
    for nb in (1, 8, 1, 8):
        C.cfg.TEST.BATCH_IMAGES = nb
        t0 = time.perf_counter()
        with redirect_stdout(io.StringIO()):
            T.test_net({"full": net}, pf, imdb)
        dt = time.perf_counter() - t0
        print("test_net BATCH_IMAGES=%d: %d images in %.2f s, %.1f images/s" % (nb, n, dt, n / dt))


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    head_pass(reps)
    dataset(n)
