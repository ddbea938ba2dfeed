#!/usr/bin/env python3
"""Train an AZ-Net -- the MI355X counterpart of the reference's tools/train_az_net.py (same flags).  Differences forced by
what exists offline:
  --solver  a Caffe solver prototxt (its train_net is read for lr_mult / decay_mult / dropout_ratio / filler std only: the
            layer graph is fixed); without it a solver and a train_net with the reference's values are written into the
            output directory (--shared: the variant with all thirteen convolutions frozen).
  --weights a .caffemodel (read with aznet_hip.caffemodel) -- or none: Caffe's fillers for the head, a seeded backbone.
  --net     `synthetic[:width_div]`: no weights at all; width_div > 1 shrinks the backbone and the head alike (fast runs).
  --imdb    `voc_<year>_<split>`, `synthetic_<H>x<W>_<N>` or `npy:<dir>`.
The snapshots (<snapshot_prefix>[_<infix>]_iter_<n>.caffemodel, adj_bbox un-normalised) load in tools/prop_az.py --net."""
import _init_paths  # noqa: F401
import os
import pprint

import numpy as np

import _cli

FLAGS = [
    ("--solver", "solver", "solver prototxt", None, str),
    ("--iters", "max_iters", "number of iterations to train", 40000, int),
    ("--weights", "pretrained_model", "initialize with pretrained model weights", None, str),
    ("--imdb", "imdb_name", "dataset to train on", "voc_2007_trainval", str),
    ("--rand", "randomize", "randomize (do not use a fixed seed)", None, None),
    ("--norm", "normalize", "to un-normalize (use when pre-trained model is normalized)", None, None),
    ("--net", "net", "(extension) synthetic[:width_div]: seeded weights, no files", None, str),
    ("--shared", "shared", "(extension, without --solver) freeze all thirteen convolutions", None, None),
    ("--base-lr", "base_lr", "(extension, without --solver) base_lr of the written solver", 0.001, float),
    ("--bf16", "bf16", "(extension) bf16 operands in the trainer's matrix products (cfg.TRAIN.PRECISION = 'bf16')", None, None),
]
COMMON = [row for row in _cli.COMMON if row[0] in ("--gpu", "--cfg", "--exp")]


def main():
    args = _cli.parse("Train a AZ-Net", [COMMON, FLAGS])
    from detect.config import cfg, cfg_from_file, cfg_set_mode, cfg_set_path, get_output_dir
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    cfg_set_path(args.exp_dir)
    cfg_set_mode("Train")
    print("Using config:")
    pprint.pprint(cfg)
    seed = cfg.RNG_SEED
    if args.randomize:
        seed = int.from_bytes(os.urandom(4), "little")
    else:
        np.random.seed(cfg.RNG_SEED)          # fix the random seeds (numpy and the dropout / filler generator)
    cfg.TRAIN.UN_NORMALIZE = bool(args.normalize)
    if args.bf16:
        cfg.TRAIN.PRECISION = 'bf16'

    import torch
    torch.cuda.set_device(args.gpu_id)
    from aznet_hip import ffi, synth
    from aznet_hip.backbone import VGG16Conv5
    from datasets.factory import get_imdb
    from detect import prototxt
    from detect.train_az import get_training_roidb, train_net
    ctx = ffi.AzContext(args.gpu_id)
    ffi.set_default_context(ctx)

    imdb = get_imdb(args.imdb_name)
    print("Loaded dataset `{:s}` for training".format(imdb.name))
    get_training_roidb(imdb)
    output_dir = get_output_dir(imdb, None)
    print("Output will be saved to `{:s}`".format(output_dir))

    solver = args.solver
    if solver is None:
        os.makedirs(output_dir, exist_ok=True)
        frozen = prototxt.CONV_LAYERS if args.shared else prototxt.CONV_LAYERS[:4]
        net_file = os.path.join(output_dir, "train.prototxt")
        prototxt.write_train_prototxt(net_file, prototxt.layer_table(frozen=frozen))
        solver = os.path.join(output_dir, "solver.prototxt")
        prototxt.write_solver_prototxt(solver, net_file, base_lr=args.base_lr, clip_gradients=20.0, average_loss=100)
    kw = {}
    if args.net is not None:
        if not args.net.startswith("synthetic"):
            raise SystemExit("--net: synthetic[:width_div] (weights files go to --weights)")
        div = int(args.net.split(":")[1]) if ":" in args.net else 1
        backbone = VGG16Conv5(device="cuda:%d" % args.gpu_id, seed=seed + 1, width_div=div)
        backbone.normalize_output(np.ones((1, 3, 600, 1000), dtype=np.float32))
        kw = dict(backbone=backbone, dims={k: max(4, v // div) for k, v in synth.FULL_DIMS.items() if k != "C"})
    train_net(solver, imdb, output_dir, pretrained_model=args.pretrained_model, max_iters=args.max_iters, ctx=ctx,
              seed=seed, **kw)


if __name__ == "__main__":
    main()
