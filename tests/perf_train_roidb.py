#!/usr/bin/env python3
"""Times the trainable roidb of synthetic_600x1000_64 with flips (128 entries): the device path end to end --
az_data_layer.roidb.prepare_roidb + add_adjacent_prediction_targets, with every copy and the np.random bookkeeping --
against the NumPy restatement tests/train_ref.py on the same host, same seed.  Not collected by pytest; it lives under
tests/ because product code may not import test infrastructure.

  python tests/perf_train_roidb.py [--reps 5] [--ref-reps 2] [--once]

--once: one untimed device pass only (what a kernel trace wraps)."""
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


def build(rdl, seed=3):
    from datasets.synthetic import SyntheticImdb
    imdb = SyntheticImdb(600, 1000, 64)
    imdb.append_flipped_images()
    np.random.seed(seed)
    t0 = time.perf_counter()
    rdl.prepare_roidb(imdb)
    t1 = time.perf_counter()
    means, stds = rdl.add_adjacent_prediction_targets(imdb)
    t2 = time.perf_counter()
    return imdb, means, stds, t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import train_ref as tr
    from az_data_layer import roidb as rdl
    from aznet_hip import ffi
    ffi.set_default_context(ffi.AzContext(0))
    imdb, means, stds, _, _ = build(rdl)                      # warm-up: allocations, code objects
    if args.once:
        return
    n = len(imdb.roidb)
    E = sum(e["ex_boxes"].shape[0] for e in imdb.roidb)
    T = sum(e["bbox_targets"].shape[0] for e in imdb.roidb)
    dev = []
    for _ in range(args.reps):
        _, _, _, a, b = build(rdl)
        dev.append((a, b))
    rdl.set_backend(tr.RefBackend())
    ref = []
    for _ in range(args.ref_reps):
        rimdb, rmeans, rstds, a, b = build(rdl)
        ref.append((a, b))
    rdl.set_backend(None)
    for x, y in zip(imdb.roidb, rimdb.roidb):
        assert np.array_equal(x["ex_boxes"], y["ex_boxes"]) and np.array_equal(x["zoom_gt"], y["zoom_gt"])
        assert np.array_equal(x["bbox_targets"][:, 4:], y["bbox_targets"][:, 4:])
    d = np.array(dev).sum(axis=1)
    r = np.array(ref).sum(axis=1)
    print("synthetic_600x1000_64 with flips: %d entries, %.0f example regions and %.0f targets per image" % (n, E / n, T / n))
    print("device path : median %.3f s (min %.3f, max %.3f over %d runs; ex_rois %.3f s + targets %.3f s) -> %.0f images/s"
          % (np.median(d), d.min(), d.max(), len(d), np.median([a for a, _ in dev]), np.median([b for _, b in dev]),
             n / np.median(d)))
    print("restatement : median %.3f s (min %.3f, max %.3f over %d runs; ex_rois %.3f s + targets %.3f s) -> %.1f images/s"
          % (np.median(r), r.min(), r.max(), len(r), np.median([a for a, _ in ref]), np.median([b for _, b in ref]),
             n / np.median(r)))
    print("speed-up %.1fx" % (np.median(r) / np.median(d)))
    assert np.median(d) < np.median(r), "the device path must be faster than the NumPy restatement"


if __name__ == "__main__":
    main()
