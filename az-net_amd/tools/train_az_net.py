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

import _cli

FLAGS = _cli.TRAIN + [
    ("--net", "net", "(extension) synthetic[:width_div]: seeded weights, no files", None, str),
    ("--shared", "shared", "(extension, without --solver) freeze all thirteen convolutions", None, None),
] + _cli.TRAIN_EXT
COMMON = [row for row in _cli.COMMON if row[0] in ("--gpu", "--cfg", "--exp")]


def main():
    args = _cli.parse("Train a AZ-Net", [COMMON, FLAGS])
    cfg = _cli.setup_cfg(args, "Train")
    seed = _cli.train_seed(args)
    if args.bf16:
        cfg.TRAIN.PRECISION = 'bf16'
    if args.snapshot_state:
        cfg.TRAIN.SNAPSHOT_STATE = True

    import torch
    torch.cuda.set_device(args.gpu_id)
    from aznet_hip import ffi, synth
    from datasets.factory import get_imdb
    from detect import prototxt
    from detect.config import get_output_dir
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
        backbone, dims = _cli.reduced_net(args.gpu_id, seed + 1, div, synth.FULL_DIMS, ("n6", "n71", "n72"))
        kw = dict(backbone=backbone, dims=dims)
    train_net(solver, imdb, output_dir, pretrained_model=args.pretrained_model, max_iters=args.max_iters, ctx=ctx,
              seed=seed, restore=args.restore, **kw)


if __name__ == "__main__":
    main()
