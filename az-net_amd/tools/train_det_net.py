#!/usr/bin/env python3
"""Train the detection net (Fast R-CNN on AZ-net proposals) -- the MI355X counterpart of the reference's
tools/train_det_net.py (same flags).  Differences forced by what exists offline:
  --solver  a Caffe solver prototxt (its train_net is read for lr_mult / decay_mult / dropout_ratio / filler std only: the
            layer graph is fixed); without it a solver and a train_net with the reference's values are written into the
            output directory.
  --weights a .caffemodel (read with aznet_hip.caffemodel; an ImageNet VGG16 brings the convolutions, fc6 and fc7) -- or
            none: Caffe's fillers for the head, a seeded backbone.
  --net     the AZ-net that makes the proposals: a .caffemodel (tools/train_az_net.py writes one), an .npz, or
            `synthetic[:width_div]`: an untrained AZ-net (seeded backbone, Caffe's fillers), no files; width_div > 1 shrinks
            both nets' backbones and heads alike.  An untrained net's proposals hit the objects only by chance, so this mode
            adds seeded jittered copies of every object to them (write_synthetic_proposals says why).
  --def / --def_fc  accepted and ignored (the layer graphs are fixed).
  --imdb    `voc_<year>_<split>`, `synthetic_<H>x<W>_<N>` or `npy:<dir>`.
The proposals are cached as proposals.pkl under the output directory of (imdb, AZ-net).  The snapshots
(<snapshot_prefix>[_<infix>]_iter_<n>.caffemodel, bbox_pred un-normalised) load in tools/test_det_net.py --net.
Under a skip configuration (--cfg experiments/cfgs/voc_skip.yml: SEAR.FRCNN_CONV names conv3_3, conv4_3, conv5_3) the
skip-connection detector is trained: without --solver the written train net is the reference's frozen/ net (all
convolutions fixed; edit its lr_mult / decay_mult and pass it through --solver to fine-tune them), the snapshots are
vgg16_fast_rcnn_skip_iter_<n>.caffemodel with conv_pool5, and load in tools/test_det_net.py under the same --cfg.
  --ohem    (extension) online hard-example mining (cfg.TRAIN.OHEM): per iteration the trainer scores every image's whole pool
            of up to TRAIN.OHEM_POOL rows in a TEST-phase pass, suppresses overlapping rows (TRAIN.OHEM_NMS) and trains on the
            BATCH_SIZE // IMS_PER_BATCH rows of highest loss per image.  IMS_PER_BATCH * OHEM_POOL may be 4096 at most."""
import _init_paths  # noqa: F401
import os

import numpy as np

import _cli

FLAGS = _cli.TRAIN + [
    ("--def", "prototxt", "(ignored) prototxt defining the AZ-net", None, str),
    ("--def_fc", "prototxt_fc", "(ignored) prototxt defining the AZ-net's fully connected part", None, str),
    ("--net", "caffemodel", "AZ-Net model that makes the proposals (.caffemodel / .npz) or synthetic[:width_div]", None, str),
] + _cli.TRAIN_EXT + [
    ("--ohem", "ohem", "(extension) online hard-example mining: every minibatch is the rows of highest loss of the images' "
                       "whole proposal pools (cfg.TRAIN.OHEM; OHEM_NMS, OHEM_POOL)", None, None),
]
COMMON = [row for row in _cli.COMMON if row[0] in ("--gpu", "--cfg", "--exp")]


def synthetic_az_net(device, seed, div):
    """An untrained AZ-net, 1 / div as wide: a seeded backbone and the head as Caffe's fillers leave it (what
    train_az_net.py --net synthetic starts from).  Its box deltas are ~0, so its proposals are the search's own sub-regions
    at every scale -- boxes of all sizes, some on the objects -- where a head of large random weights throws every box to
    the image border."""
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipAZNet
    backbone, dims = _cli.reduced_net(device, seed + 1, div, synth.FULL_DIMS, ("n6", "n71", "n72"))
    ctx = ffi.AzContext(device)
    sol = ffi.AzSolver(ctx, backbone.out_channels, dims["n6"], dims["n71"], dims["n72"], max_rois=8, seed=seed)
    head = sol.read()
    sol.close()
    return HipAZNet(head, backbone=backbone, device=device, name="vgg16_az_net_synthetic_div%d" % div, ctx=ctx)


def write_synthetic_proposals(net, imdb, seed, copies=6, amount=0.1):
    """proposals.pkl for a synthetic AZ-net, where there is none yet.  An untrained net finds the objects only by chance, and
    a class whose only positive is the object itself has targets of std 0, which the normalisation divides by (as the
    reference's does).  So that a run without files has targets with a spread, every object is added `copies` times with
    its corners moved by up to `amount` of its sides (seeded; IoU with the object >= 0.6) behind the net's own proposals."""
    import pickle
    from detect.config import cfg, get_output_dir
    from detect.test import im_propose
    out = get_output_dir(imdb, net)
    path = os.path.join(out, "proposals.pkl")
    if os.path.exists(path):
        return path
    rng = np.random.RandomState(seed % (2 ** 32))
    props = []
    for i in range(len(imdb.image_index)):
        h, w = imdb.image_size(i)
        regions = np.asarray(im_propose(net, imdb.image_at(i), num_proposals=cfg.SEAR.NUM_PROPOSALS), dtype=np.float64).reshape(-1, 4)
        gt = imdb.roidb[i]["boxes"].astype(np.float64)
        side = np.stack([gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]] * 2, axis=1)
        near = np.repeat(gt, copies, axis=0) + rng.uniform(-amount, amount, (copies * gt.shape[0], 4)) * np.repeat(side, copies, axis=0)
        near[:, 0::2] = np.clip(near[:, 0::2], 0, w - 1)
        near[:, 1::2] = np.clip(near[:, 1::2], 0, h - 1)
        props.append(np.vstack((regions, near)).astype(np.float32))
    os.makedirs(out, exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump(props, f, pickle.HIGHEST_PROTOCOL)
    print("wrote the synthetic net's proposals (with {} seeded copies of every object) to {}".format(copies, path))
    return path


def main():
    args = _cli.parse("Train a detection network", [COMMON, FLAGS])
    cfg = _cli.setup_cfg(args, "Train")
    seed = _cli.train_seed(args)
    if args.bf16:
        cfg.TRAIN.PRECISION = 'bf16'
    if args.snapshot_state:
        cfg.TRAIN.SNAPSHOT_STATE = True
    if args.ohem:
        cfg.TRAIN.OHEM = True

    import torch
    torch.cuda.set_device(args.gpu_id)
    from aznet_hip import ffi, synth
    from datasets.factory import get_imdb
    from detect import prototxt
    from detect.config import get_output_dir
    from detect.train_det import get_training_roidb, train_net

    # the AZ-net that makes the proposals (its own context, closed before the trainer's is made)
    div, az_net = 1, None
    if args.caffemodel is not None:
        if args.caffemodel.startswith("synthetic"):
            div = int(args.caffemodel.split(":")[1]) if ":" in args.caffemodel else 1
            az_net = synthetic_az_net(args.gpu_id, seed, div)
        else:
            import prop_az
            az_net = prop_az.load_net(args.caffemodel, args.gpu_id)
        ffi.set_default_context(az_net.ctx)
    imdb = get_imdb(args.imdb_name)
    print("Loaded dataset `{:s}` for training".format(imdb.name))
    if az_net is None:
        raise SystemExit("--net is required: the AZ-net whose proposals the detection net is trained on")
    if args.caffemodel.startswith("synthetic"):
        write_synthetic_proposals(az_net, imdb, seed)          # (before the flipped entries are appended)
    get_training_roidb(imdb, {"full": az_net, "fc": az_net})
    ctx = az_net.ctx                            # one context serves the proposals, the targets and the trainer
    del az_net
    output_dir = get_output_dir(imdb, None)
    print("Output will be saved to `{:s}`".format(output_dir))

    solver = args.solver
    if solver is None:
        os.makedirs(output_dir, exist_ok=True)
        if len(cfg.SEAR.FRCNN_CONV) > 1:
            # the skip-connection detector (--cfg voc_skip.yml): the reference's frozen/ net and solver_skip values
            if tuple(cfg.SEAR.FRCNN_CONV) != prototxt.SKIP_SOURCES:
                raise SystemExit("cfg.SEAR.FRCNN_CONV = %s: without --solver the skip train net is written for %s"
                                 % (list(cfg.SEAR.FRCNN_CONV), list(prototxt.SKIP_SOURCES)))
            net_file = os.path.join(output_dir, "train_det_skip.prototxt")
            prototxt.write_skip_train_prototxt(net_file, prototxt.skip_layer_table())
            solver = os.path.join(output_dir, "solver_det_skip.prototxt")
            prototxt.write_solver_prototxt(solver, net_file, base_lr=args.base_lr, gamma=0.2, stepsize=160000, clip_gradients=20.0,
                                           average_loss=100, snapshot_prefix="vgg16_fast_rcnn_skip")
        else:
            net_file = os.path.join(output_dir, "train_det.prototxt")
            prototxt.write_train_prototxt(net_file, prototxt.det_layer_table(), name="frcnn_train")
            solver = os.path.join(output_dir, "solver_det.prototxt")
            prototxt.write_solver_prototxt(solver, net_file, base_lr=args.base_lr, stepsize=60000, clip_gradients=20.0, average_loss=100,
                                           snapshot_prefix="vgg16_frcnn")
    kw = {}
    if div > 1 or (args.caffemodel.startswith("synthetic") and args.pretrained_model is None):
        backbone, dims = _cli.reduced_net(args.gpu_id, seed + 3, div, synth.FULL_DET_DIMS, ("n6", "n7"))
        kw = dict(backbone=backbone, dims=dims)
    train_net(solver, imdb, output_dir, pretrained_model=args.pretrained_model, max_iters=args.max_iters, ctx=ctx,
              seed=seed, restore=args.restore, **kw)


if __name__ == "__main__":
    main()
