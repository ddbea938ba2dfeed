#!/usr/bin/env python3
"""Build the trainable roidb of a dataset on the GPU: example regions, zoom labels and normalised adjacency targets
(the reference does this inside tools/train_az.py before the solver starts: get_training_roidb, then
add_adjacent_prediction_targets).  Prints images/s, example regions and targets per image and the 44 means / stds, and
writes the two cache pickles <cache>/<imdb>_trainable_roidb.pkl and <cache>/<imdb>_targets_roidb.pkl that a later run
with TRAIN.USE_CACHE reads.

  python tools/prepare_roidb.py --imdb synthetic_600x1000_64 [--cfg file.yml] [--seed N] [--no-flip] [--gpu 0]
"""
import _init_paths  # noqa: F401
import argparse
import os
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser(description="Build the trainable roidb of AZ-Net on the GPU")
    ap.add_argument("--imdb", dest="imdb_name", default="voc_2007_trainval")
    ap.add_argument("--cfg", dest="cfg_file", default=None, help="optional YAML config")
    ap.add_argument("--seed", type=int, default=None, help="np.random seed of the label noise (default cfg.RNG_SEED)")
    ap.add_argument("--no-flip", action="store_true", help="do not append the flipped images")
    ap.add_argument("--gpu", dest="gpu_id", type=int, default=0)
    args = ap.parse_args()

    from detect.config import cfg, cfg_from_file
    if args.cfg_file:
        cfg_from_file(args.cfg_file)
    if args.no_flip:
        cfg.TRAIN.USE_FLIPPED = False
    from aznet_hip import ffi
    ffi.set_default_context(ffi.AzContext(args.gpu_id))
    import az_data_layer.roidb as rdl
    from datasets.factory import get_imdb
    from detect.train_az import get_training_roidb

    imdb = get_imdb(args.imdb_name)
    for name in ("_trainable_roidb.pkl", "_targets_roidb.pkl"):       # this run REBUILDS the caches
        p = os.path.join(imdb.cache_path, imdb.name + name)
        if os.path.exists(p):
            os.remove(p)
    cfg.TRAIN.USE_CACHE = True
    np.random.seed(cfg.RNG_SEED if args.seed is None else args.seed)
    t0 = time.time()
    roidb = get_training_roidb(imdb)
    t1 = time.time()
    means, stds = rdl.add_adjacent_prediction_targets(imdb)
    t2 = time.time()
    n = len(roidb)
    E = sum(e["ex_boxes"].shape[0] for e in roidb)
    T = sum(e["bbox_targets"].shape[0] for e in roidb)
    Z = sum(int(e["zoom_gt"].sum()) for e in roidb)
    print("%s: %d roidb entries (%s flips)" % (imdb.name, n, "with" if cfg.TRAIN.USE_FLIPPED else "without"))
    print("example regions: %.3f s, adjacency targets: %.3f s (caches included) -> %.1f images/s"
          % (t1 - t0, t2 - t1, n / max(t2 - t0, 1e-9)))
    print("per image: %.1f example regions (%.1f with a zoom label), %.1f targets" % (E / n, Z / n, T / n))
    np.set_printoptions(precision=6, linewidth=120, suppress=True)
    print("means [11 sub-regions x (dx, dy, dw, dh)]:\n%s" % means.reshape(-1, 4))
    print("stds:\n%s" % stds.reshape(-1, 4))


if __name__ == "__main__":
    main()
