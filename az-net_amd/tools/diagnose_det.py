#!/usr/bin/env python3
"""Diagnose a saved detections.pkl (test_net's all_boxes, before NMS): which kinds of error its AP is made of.
NMS at cfg.TEST.NMS first, exactly as tools/eval_det.py applies it (detect.test.postprocess_detections, so --soft-nms /
--bbox-vote diagnose a saved run under Soft-NMS and box voting), unless --no-nms.  Then detect.diagnose_det: every
detection typed after Hoiem et al. (ECCV 2012) -- true positive, duplicate, localisation, similar class, other class,
background -- the missed objects, and the AP with each kind of error fixed (TIDE, ECCV 2020), in one device call over
the whole set.  Prints the tables and writes <out>/det_diagnosis.pkl.  The reference has no counterpart: it left
evaluation to MATLAB.
--protocol voc (the default): VOCevaldet's rules on any imdb with ground truth (a COCO imdb through its gt_roidb) -- one
threshold 0.5, the +1 overlap, difficult boxes, the 11-point or area AP, and the cut table of the top-ranked detections.
--protocol coco: COCOeval's rules -- ten thresholds .50:.95, crowd boxes, the first 100 detections per image and
category, the 101-point AP; the AP / AP50 / AP75 that eval_det.py prints for a COCO imdb, each with its seven dAP columns,
and the type tables at IoU .50 and .75.  A COCO imdb is packed from its annotation file as evaluation packs it (no file
is written), any other imdb from gt_roidb.  Writes <out>/det_diagnosis_coco.pkl.  Area range all only; no cut table."""
import _init_paths  # noqa: F401
import argparse
import os
import pickle

import _cli


def build_parser():
    ap = argparse.ArgumentParser(description="Diagnose a saved detections.pkl (false-positive types, oracle-fix AP)")
    ap.add_argument("dets", help="detections.pkl written by test_net")
    ap.add_argument("--imdb", dest="imdb_name", default="voc_2007_test")
    ap.add_argument("--out", dest="output_dir", default=None, help="where det_diagnosis.pkl goes (default: next to dets)")
    ap.add_argument("--no-nms", dest="no_nms", action="store_true", help="diagnose the detections as saved")
    ap.add_argument("--bg-overlap", dest="bg_overlap", type=float, default=0.1,
                    help="overlap from which a false positive is a localisation error or a confusion (default 0.1)")
    ap.add_argument("--protocol", dest="protocol", choices=("voc", "coco"), default="voc",
                    help="voc: VOCevaldet's rules, one threshold, det_diagnosis.pkl (default); coco: COCOeval's rules, "
                         "AP@[.5:.95] / AP50 / AP75 with area all and maxDets 100, det_diagnosis_coco.pkl")
    ap.add_argument("--cfg", dest="cfg_file", default=None)
    ap.add_argument("--gpu", dest="gpu_id", type=int, default=0)
    return _cli.add_flags(ap, [_cli.POSTPROC])


def main():
    args = build_parser().parse_args()
    from detect.config import cfg_from_file
    if args.cfg_file:
        cfg_from_file(args.cfg_file)
    _cli.set_postproc(args)
    import torch
    torch.cuda.set_device(args.gpu_id)
    from datasets.factory import get_imdb
    from detect.diagnose_det import diagnose, summary_lines
    from detect.test import postprocess_detections
    with open(args.dets, "rb") as f:
        all_boxes = pickle.load(f)
    imdb = get_imdb(args.imdb_name)
    if len(all_boxes) != imdb.num_classes or len(all_boxes[0]) != imdb.num_images:
        raise SystemExit("error: %s holds %d x %d entries, %s has %d classes x %d images"
                         % (args.dets, len(all_boxes), len(all_boxes[0]), imdb.name, imdb.num_classes, imdb.num_images))
    if not args.no_nms:
        print("Applying NMS to all detections")
        all_boxes = postprocess_detections(all_boxes)
    from aznet_hip import ffi
    ctx = ffi.default_context(args.gpu_id)               # --gpu's device: the context the NMS above ran on, or a new one there
    d = diagnose(imdb, all_boxes, bg_overlap=args.bg_overlap, ctx=ctx, protocol=args.protocol)
    for line in summary_lines(d):
        print(line)
    out = args.output_dir or os.path.dirname(os.path.abspath(args.dets))
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "det_diagnosis_coco.pkl" if args.protocol == "coco" else "det_diagnosis.pkl")
    with open(path, "wb") as f:
        pickle.dump(d, f, pickle.HIGHEST_PROTOCOL)
    print("wrote", path)


if __name__ == "__main__":
    main()
