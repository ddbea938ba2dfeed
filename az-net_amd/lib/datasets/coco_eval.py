"""COCO box evaluation: what coco._do_coco_eval hands to pycocotools (COCOeval evaluate / accumulate / summarize),
run natively with iouType 'bbox' (DESIGN §1c).  The results file is read back as COCO.loadRes reads it, ground truth
and detections are packed into az_coco_eval's class-major (category, image) segments, and one call evaluates every
category on the GPU.  Prints COCOeval.summarize's 12 lines."""
import json

import numpy as np

from aznet_hip import ffi

_SUMMARY = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100),
            (1, None, "medium", 100), (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10),
            (0, None, "all", 100), (0, None, "small", 100), (0, None, "medium", 100), (0, None, "large", 100)]


def summary_lines(stats):
    """COCOeval.summarize's printed lines for the 12 stats."""
    i_str = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    out = []
    for (ap, iou, area, md), v in zip(_SUMMARY, stats):
        iou_str = "{:0.2f}:{:0.2f}".format(0.5, 0.95) if iou is None else "{:0.2f}".format(iou)
        out.append(i_str.format("Average Precision" if ap == 1 else "Average Recall", "(AP)" if ap == 1 else "(AR)",
                                iou_str, area, md, float(v)))
    return out


def pack(gt_index, results):
    """Ground truth (a COCOIndex) and a loaded results list -> az_coco_eval's arguments as a dict.  Images and
    categories are the ground truth's sorted unique ids; a detection of another category is dropped (getAnnIds'
    catIds filter), one on another image is an error (loadRes's assertion).  Within a segment, file order."""
    img_ids = np.unique(np.array(gt_index.getImgIds(), np.int64))
    cat_ids = np.unique(np.array(gt_index.getCatIds(), np.int64))
    K, N = len(cat_ids), len(img_ids)

    def segments(image_ids, cat):
        ii = np.searchsorted(img_ids, image_ids)
        kk = np.searchsorted(cat_ids, cat)
        ok_i = (ii < N) & (img_ids[np.minimum(ii, max(N - 1, 0))] == image_ids) if N else np.zeros(len(ii), bool)
        ok_k = (kk < K) & (cat_ids[np.minimum(kk, max(K - 1, 0))] == cat) if K else np.zeros(len(kk), bool)
        return kk * N + ii, ok_i, ok_k

    anns = [a for i in img_ids.tolist() for a in gt_index.img_to_anns.get(i, [])]
    g_img = np.array([a["image_id"] for a in anns], np.int64)
    g_cat = np.array([a["category_id"] for a in anns], np.int64)
    g_seg, _, g_ok = segments(g_img, g_cat)
    g_box = np.array([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
    g_area = np.array([a["area"] for a in anns], np.float64)
    g_crowd = np.array([1 if a.get("iscrowd", 0) else 0 for a in anns], np.uint8)

    d_img = np.array([r["image_id"] for r in results], np.int64)
    d_cat = np.array([r["category_id"] for r in results], np.int64)
    d_seg, d_oki, d_ok = segments(d_img, d_cat)
    if not d_oki.all():
        raise ValueError("Results do not correspond to current coco set")
    d_box = np.array([r["bbox"] for r in results], np.float64).reshape(-1, 4)
    d_score = np.array([r["score"] for r in results], np.float64)

    def order(seg, ok):
        keep = np.nonzero(ok)[0]
        o = keep[np.argsort(seg[keep], kind="stable")]
        off = np.zeros(K * N + 1, np.int64)
        off[1:] = np.cumsum(np.bincount(seg[keep], minlength=K * N))
        return o, off

    go, goff = order(g_seg, g_ok)
    do, doff = order(d_seg, d_ok)
    if doff[-1] >= 2 ** 31 or goff[-1] >= 2 ** 31:
        raise ffi.AzError(ffi.AZ_ERR_CAPACITY, "coco_eval: more than int32 boxes")
    return {"n_classes": K, "n_images": N, "det_box": d_box[do], "det_score": d_score[do], "det_off": doff,
            "gt_box": g_box[go], "gt_area": g_area[go], "gt_crowd": g_crowd[go], "gt_off": goff,
            "cat_ids": cat_ids, "img_ids": img_ids, "det_order": do}


def evaluate(gt_index, results, ctx=None, verbose=True):
    """COCOeval(gt, gt.loadRes(results), 'bbox') evaluate + accumulate + summarize.  Returns az_coco_eval's dict
    (stats [12], precision [10,101,K,4,3], recall [10,K,4,3]) plus the packing's cat_ids / img_ids."""
    p = pack(gt_index, results)
    ctx = ctx or ffi.default_context()
    r = ctx.coco_eval(p["n_classes"], p["n_images"], p["det_box"], p["det_score"], p["det_off"], p["gt_box"],
                      p["gt_area"], p["gt_crowd"], p["gt_off"])
    r["cat_ids"], r["img_ids"] = p["cat_ids"], p["img_ids"]
    if verbose:
        print("\n".join(summary_lines(r["stats"])))
    return r


def evaluate_results_file(gt_index, path, ctx=None):
    with open(path) as f:
        results = json.load(f)
    if not isinstance(results, list):
        raise ValueError("results in not an array of objects")
    return evaluate(gt_index, results, ctx=ctx)
