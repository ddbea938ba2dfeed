#!/usr/bin/env python3
"""Re-evaluate a saved detections.pkl (test_net's all_boxes, before NMS) without rerunning detection.
NMS at cfg.TEST.NMS first (as test_net does: detect.test.postprocess_detections, so --soft-nms / --bbox-vote or the
cfg.TEST keys behind them re-score a saved run under Soft-NMS and box voting), unless --no-nms.
A VOC or COCO imdb goes through its own evaluate_detections: VOC results files and XML ground truth with difficult flags (voc_eval.m's AP block,
<cls>_pr.mat in --out), or the COCO results json in --out and COCOeval's 12 summary lines (box IoU).
Any other imdb with a gt_roidb is evaluated the VOC way on its ground truth, difficult taken as 0 and the
detections rounded as a results file would hold them."""
import _init_paths  # noqa: F401
import argparse
import os
import pickle

import _cli


def eval_on_roidb(imdb, all_boxes, output_dir):
    from datasets import voc_eval
    classes = [c for c in imdb.classes if c != "__background__"]
    n = imdb.num_images
    gb, gd, goff = voc_eval.gt_segments(classes, voc_eval.roidb_records(imdb))
    dets = voc_eval.all_boxes_dets(imdb, all_boxes)
    r = voc_eval.evaluate(n, classes, dets, gb, gd, goff, metric_07=True)
    os.makedirs(output_dir, exist_ok=True)
    lines, tail = voc_eval.report(classes, r["ap"], r["ap_auc"])
    co = r["class_off"]
    for k, c in enumerate(classes):
        print(lines[k])
        voc_eval.save_pr(output_dir, c, r["rec"][co[k]:co[k + 1]], r["prec"][co[k]:co[k + 1]], r["ap"][k], r["ap_auc"][k])
    print("\n".join(tail))
    return r["ap"], r["ap_auc"]


def build_parser():
    ap = argparse.ArgumentParser(description="Evaluate a saved detections.pkl (PASCAL VOC AP / COCO AP)")
    ap.add_argument("dets", help="detections.pkl written by test_net")
    ap.add_argument("--imdb", dest="imdb_name", default="voc_2007_test")
    ap.add_argument("--out", dest="output_dir", default=None, help="where <cls>_pr.mat / the COCO results json go (default: next to dets)")
    ap.add_argument("--no-nms", dest="no_nms", action="store_true", help="evaluate the detections as saved")
    ap.add_argument("--comp", dest="comp_mode", action="store_true", help="competition mode (keep results files)")
    ap.add_argument("--cfg", dest="cfg_file", default=None)
    ap.add_argument("--gpu", dest="gpu_id", type=int, default=0)
    return _cli.add_flags(ap, [_cli.POSTPROC])


def main():
    args = build_parser().parse_args()
    from detect.config import cfg, cfg_from_file
    if args.cfg_file:
        cfg_from_file(args.cfg_file)
    _cli.set_postproc(args)
    import torch
    torch.cuda.set_device(args.gpu_id)
    from datasets.factory import get_imdb
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
    out = args.output_dir or os.path.dirname(os.path.abspath(args.dets))
    print("Evaluating detections")
    if hasattr(imdb, "evaluate_detections"):
        imdb.competition_mode(args.comp_mode)
        imdb.evaluate_detections(all_boxes, out)
    else:
        eval_on_roidb(imdb, all_boxes, out)


if __name__ == "__main__":
    main()
