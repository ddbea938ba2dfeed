#!/usr/bin/env python3
"""Fast R-CNN detection on saved proposals -- the MI355X counterpart of the reference's tools/test_det_net.py
(same flags), the last step of the unshared recipe: prop_az.py writes proposals.pkl, this runs a Fast R-CNN
VGG16 with its OWN conv layers over them (detect.test.test_net).
--net takes a .caffemodel, an .npz (conv*_w / conv*_b plus W6 b6 W7 b7 Wc bc Wb bb) or `synthetic[:seed]`;
--def is accepted and ignored (the layer graph is fixed); --imdb is `voc_<year>_<split>`,
`synthetic_<H>x<W>_<N>` or `npy:<dir>`."""
import _init_paths  # noqa: F401
import os

import numpy as np

import _cli

FLAGS = [
    ("--def", "prototxt", "(ignored) prototxt defining the classifier network", None, str),
    ("--net", "caffemodel", "classifier weights (.caffemodel / .npz) or synthetic[:seed]", None, str),
    ("--prop", "prop", "file saving object proposals", None, str),
    ("--imdb", "imdb_name", "dataset to test", "voc_2007_test", str),
    ("--comp", "comp_mode", "competition mode", None, None),
    # (extension) cfg.TEST.BATCH_IMAGES: the detection head over the proposals of up to N consecutive images in one pass
    ("--batch-images", "batch_images", "run the detection head over up to N consecutive images at once (default 1)", 1, int),
]


def load_frcnn_net(spec, device, tuned=False):
    """HipFrcnnNet (detection head + VGG16 with the detection net's own conv weights) from a --net value."""
    from aznet_hip import synth
    from aznet_hip.backbone import VGG16Conv5
    from aznet_hip.net import HipFrcnnNet
    if tuned:
        import torch
        torch.backends.cudnn.benchmark = True
    if os.environ.get("AZ_BACKBONE_DETERMINISTIC", "0") not in ("", "0"):
        # (as in prop_az.load_net: runs compared across processes pin MIOpen's convolution algorithms)
        import torch
        torch.backends.cudnn.deterministic = True
        if os.environ["AZ_BACKBONE_DETERMINISTIC"] == "2":
            torch.backends.cudnn.enabled = False
    kw = dict(device="cuda:%d" % device, channels_last_compute=bool(tuned), channels_last_out=True)
    if spec.startswith("synthetic"):
        seed = int(spec.split(":")[1]) if ":" in spec else 4242
        head = synth.make_det_head(seed=seed, **synth.FULL_DET_DIMS)
        backbone = VGG16Conv5(seed=seed + 1, **kw)
        backbone.normalize_output(np.zeros((1, 3, 600, 1000), dtype=np.float32) + 1.0)
        name = "vgg16_frcnn_synthetic_%d" % seed
    elif spec.endswith(".caffemodel"):
        from aznet_hip import caffemodel as cm
        layers = cm.load_caffemodel(spec)
        head = cm.det_head_from_layers(layers)
        backbone = VGG16Conv5(weights=cm.backbone_from_layers(layers), **kw)
        name = os.path.splitext(os.path.basename(spec))[0]
    else:
        z = np.load(spec)
        head = {k: z[k] for k in ("W6", "b6", "W7", "b7", "Wc", "bc", "Wb", "bb")}
        conv = {k[:-2]: (z[k], z[k[:-2] + "_b"]) for k in z.files if k.startswith("conv") and k.endswith("_w")}
        backbone = VGG16Conv5(weights=conv or None, **kw)
        name = os.path.splitext(os.path.basename(spec))[0]
    return HipFrcnnNet(head, backbone, device=device, name=name)


def main():
    args = _cli.parse("Use Fast-RCNN for object detection", [_cli.COMMON, FLAGS])
    # (the reference's order, without a search mode: this step makes no proposals)
    import pprint
    from detect.config import cfg, cfg_from_file, cfg_set_path
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    cfg_set_path(args.exp_dir)
    print("Using config:")
    pprint.pprint(cfg)
    cfg.TEST.BATCH_IMAGES = max(1, int(getattr(args, "batch_images", 1) or 1))
    if args.caffemodel is None or args.prop is None:
        print("error: --net and --prop are required")
        raise SystemExit(2)
    if not args.caffemodel.startswith("synthetic"):
        _cli.wait_for(args.caffemodel, args.wait)
    import torch
    torch.cuda.set_device(args.gpu_id)
    from datasets.factory import get_imdb
    from detect import test as T
    net = load_frcnn_net(args.caffemodel, args.gpu_id, tuned=bool(getattr(args, "tune_backbone", False)))
    imdb = get_imdb(args.imdb_name)
    if hasattr(imdb, "competition_mode"):
        imdb.competition_mode(args.comp_mode)
    T.test_net({"full": net}, args.prop, imdb)


if __name__ == "__main__":
    main()
