#!/usr/bin/env python3
"""Compress a Fast R-CNN detection net's fc6 / fc7 by truncated SVD -- the counterpart of Fast R-CNN's
tools/compress_net.py (section 4.4 of the paper; not in the reference tree): no retraining, fewer FLOPs.

    compress_net.py --net <det .caffemodel | synthetic[:seed]> [--fc6 1024] [--fc7 256] [--out path]

writes <name>_svd_fc6_<r6>_fc7_<r7>.caffemodel beside the input (or at --out): fc6 becomes fc6_L (one blob [r6, in], no
bias) + fc6_U ([out, r6] and fc6's bias), fc7 likewise; every other layer (the backbone's convolutions, conv_pool5,
cls_score, bbox_pred) is copied through.  A rank of 0 leaves that layer as it is.  `synthetic[:seed]` is the seeded
reduced detection head (synth.SMALL_DET_DIMS) alone -- under a --cfg that names the skip-connection detector's maps, with
a seeded front --, for trying the tool without weights.  Prints, per layer, ||W - U L||_F / ||W||_F.
test_det_net.py --net <that file>, test_shared.py --net_frcnn <that file> and perf_det.py then run the compressed head
with no further flag.

An AZ net -- a file that holds an int6 layer -- has its int6 compressed instead:

    compress_net.py --net <az .caffemodel | synthetic[:seed]> --int6 1024 [--out path]

writes <name>_svd_int6_<r>.caffemodel: int6_L (one blob) + int6_U (weight and int6's bias) in int6's place, every other
layer (the convolutions, int7_1, int7_2, adj_score, adj_bbox, zoom_score) copied through.  `synthetic[:seed]` with --int6
and neither --fc6 nor --fc7 is the seeded reduced AZ head (synth.SMALL_DIMS).  prop_az.py, set_thresh.py, diagnose_prop.py,
test_shared.py --net_az and train_det_net.py --net run that file with no further flag.  The compressed net is another
model: its zoom scores move, so tune thresh.pkl on the compressed file (train_az_net.py snapshot -> compress_net.py --int6
-> set_thresh.py -> prop_az.py).  A file with neither int6 nor fc6 is refused."""
import _init_paths  # noqa: F401
import argparse
import os


def synthetic_layers(seed, skip=False):
    """{layer: blobs} of the seeded reduced detection head (and, skip: a seeded conv_pool5 that folds VGG16's 256 + 512 +
    512 source channels to the reduced head's C -- the channel counts a file without conv layers is read with)."""
    from aznet_hip import synth
    head = synth.make_det_head(seed=seed, **synth.SMALL_DET_DIMS)
    layers = {"fc6": [head["W6"], head["b6"]], "fc7": [head["W7"], head["b7"]],
              "cls_score": [head["Wc"], head["bc"]], "bbox_pred": [head["Wb"], head["bb"]]}
    if skip:
        C = synth.SMALL_DET_DIMS["C"]
        front = synth.make_skip_front(seed=seed + 2, Cs=synth.SKIP_CS, Cout=C)
        layers["conv_pool5"] = [front["Wp"].reshape(C, -1, 1, 1), front["bp"]]
    return layers


def synthetic_az_layers(seed):
    """{layer: blobs} of the seeded reduced AZ head (synth.SMALL_DIMS)."""
    from aznet_hip import synth
    head = synth.make_head(seed=seed, **synth.SMALL_DIMS)
    return {"int6": [head["W6"], head["b6"]], "int7_1": [head["W71"], head["b71"]], "int7_2": [head["W72"], head["b72"]],
            "adj_score": [head["Was"], head["bas"]], "adj_bbox": [head["Wab"], head["bab"]],
            "zoom_score": [head["Wz"], head["bz"]]}


def compress_az_layers(layers, r6, log=print):
    """The layer dict of an AZ net with int6 replaced by int6_L / int6_U at rank r6, everything else as it is and in the
    file's order.  -> (layers, {"int6": relative Frobenius error})."""
    from aznet_hip import caffemodel as cm
    from aznet_hip import compress
    r6 = int(r6)
    W, b = cm._fc(layers, "int6")
    Lf, U = compress.compress_layer(W, r6)
    err = compress.rel_error(W, Lf, U)
    log("int6 [%d, %d] -> int6_L [%d, %d] + int6_U [%d, %d]: ||W - U L|| / ||W|| = %.6e"
        % (W.shape[0], W.shape[1], r6, W.shape[1], W.shape[0], r6, err))
    out = {}
    for name, blobs in layers.items():
        if name == "int6":
            out["int6_L"], out["int6_U"] = [Lf], [U, b]
        else:
            out[name] = blobs
    return out, {"int6": err}


def compress_layers(layers, r6, r7, log=print):
    """The layer dict with fc6 / fc7 replaced by their _L / _U pairs at ranks r6 / r7 (0: kept), everything else as it is
    and in the file's order.  -> (layers, {layer: relative Frobenius error})."""
    from aznet_hip import caffemodel as cm
    from aznet_hip import compress
    out, errs = {}, {}
    ranks = {"fc6": int(r6 or 0), "fc7": int(r7 or 0)}
    for name, blobs in layers.items():
        r = ranks.get(name, 0)
        if not r:
            out[name] = blobs
            continue
        W, b = cm._fc(layers, name)
        Lf, U = compress.compress_layer(W, r)
        errs[name] = compress.rel_error(W, Lf, U)
        log("%s [%d, %d] -> %s_L [%d, %d] + %s_U [%d, %d]: ||W - U L|| / ||W|| = %.6e"
            % (name, W.shape[0], W.shape[1], name, r, W.shape[1], name, W.shape[0], r, errs[name]))
        out[name + "_L"] = [Lf]
        out[name + "_U"] = [U, b]
    for name, r in ranks.items():
        if r and name not in layers:
            raise ValueError("the net has no %s layer to compress (already compressed?)" % name)
    return out, errs


def main(argv=None):
    ap = argparse.ArgumentParser(description="Compress a Fast R-CNN network's fc6 / fc7 by truncated SVD")
    ap.add_argument("--net", dest="caffemodel", required=True, help="detection net (.caffemodel) or synthetic[:seed]")
    ap.add_argument("--def", dest="prototxt", default=None, help="(ignored) prototxt of the uncompressed network")
    ap.add_argument("--def-svd", dest="prototxt_svd", default=None, help="(ignored) prototxt of the compressed network")
    ap.add_argument("--fc6", dest="r6", type=int, default=None, help="rank of fc6 (0: leave it; default 1024)")
    ap.add_argument("--fc7", dest="r7", type=int, default=None, help="rank of fc7 (0: leave it; default 256)")
    ap.add_argument("--int6", dest="r_int6", type=int, default=None, help="an AZ net: rank of int6 (default 1024)")
    ap.add_argument("--out", dest="out", default=None, help="output file (default: <name>_svd_fc6_<r6>_fc7_<r7>.caffemodel; an AZ net: <name>_svd_int6_<r>.caffemodel)")
    ap.add_argument("--cfg", dest="cfg_file", default=None, help="optional config file (synthetic: a skip configuration adds the front)")
    args = ap.parse_args(argv)
    from aznet_hip import caffemodel as cm
    det_flags = args.r6 is not None or args.r7 is not None
    args.r6 = 1024 if args.r6 is None else args.r6
    args.r7 = 256 if args.r7 is None else args.r7
    if args.caffemodel.startswith("synthetic") and args.r_int6 is not None and not det_flags:
        seed = int(args.caffemodel.split(":")[1]) if ":" in args.caffemodel else 4242
        layers = synthetic_az_layers(seed)
        stem = "vgg16_az_net_synthetic_%d" % seed
    elif args.caffemodel.startswith("synthetic"):
        seed = int(args.caffemodel.split(":")[1]) if ":" in args.caffemodel else 4242
        skip = False
        if args.cfg_file is not None:
            from detect.config import cfg, cfg_from_file
            cfg_from_file(args.cfg_file)
            skip = len(cfg.SEAR.FRCNN_CONV) > 1
        layers = synthetic_layers(seed, skip)
        stem = "vgg16_frcnn_synthetic_%d" % seed
    else:
        layers = cm.load_caffemodel(args.caffemodel)
        stem = os.path.splitext(args.caffemodel)[0]
    if "int6" in layers:                      # an AZ net is recognised by its int6 layer
        r = 1024 if args.r_int6 is None else args.r_int6
        out_layers, _ = compress_az_layers(layers, r)
        path = args.out or "%s_svd_int6_%d.caffemodel" % (stem, r)
    elif "fc6" in layers or "fc6_L" in layers:
        out_layers, _ = compress_layers(layers, args.r6, args.r7)
        path = args.out or "%s_svd_fc6_%d_fc7_%d.caffemodel" % (stem, args.r6, args.r7)
    else:
        raise ValueError("the net holds neither an int6 layer (an AZ net) nor an fc6 layer (a detection net): nothing to compress")
    cm.write_caffemodel(path, out_layers)
    print("Wrote compressed network to %s (%.1f MB)" % (path, os.path.getsize(path) / 1e6))
    return path


if __name__ == "__main__":
    main()
