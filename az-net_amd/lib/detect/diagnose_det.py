"""Why is a detector's AP what it is?  Every detection of a VOC evaluation typed after Hoiem et al., "Diagnosing Error in
Object Detectors" (ECCV 2012) -- true positive, duplicate, localisation error, confusion with a similar class, with
another class, with background -- and the AP recomputed with each kind of error fixed, after TIDE (Bolya et al.,
ECCV 2020): which errors cost how much.

    diagnose(imdb, all_boxes)   the tables for a whole image set, in one az_det_diag_eval call ("Detection
                                diagnosis"); with protocol="coco" under COCOeval's rules -- ten IoU thresholds, crowd
                                boxes, 100 detections per image and category, the 101-point AP -- in one
                                az_coco_diag_eval call ("Detection diagnosis, COCO protocol")
    summary_lines(d)            the tables as text, for either protocol

`all_boxes` is what test_net saves as detections.pkl, after NMS.  The reference has no such analysis (it handed evaluation
to MATLAB); the wording of the summary is this backend's own.
"""
import numpy as np

from datasets import voc_eval

TYPE_NAMES = ("IGN", "TP", "DUP", "LOC", "SIM", "OTH", "BG")
IGN, TP, DUP, LOC, SIM, OTH, BG = range(7)
VARIANT_NAMES = ("plain", "-DUP", "LOC fixed", "-SIM", "-OTH", "-BG", "-missed", "all")
DEFAULT_CUTS = (0.25, 0.5, 1, 2, 4, 8)
DEFAULT_AREA_EDGES = (32 ** 2, 96 ** 2)
SIZE_NAMES = ("small", "medium", "large")
# Hoiem's sets of similar classes; tvmonitor and bottle are similar to nothing
VOC_GROUPS = {"vehicles": ("aeroplane", "bicycle", "boat", "bus", "car", "motorbike", "train"),
              "animals": ("bird", "cat", "cow", "dog", "horse", "sheep"),
              "furniture": ("chair", "diningtable", "pottedplant", "sofa"),
              "person": ("person",), "bottle": ("bottle",), "tvmonitor": ("tvmonitor",)}


def default_groups(classes):
    """class_group for `classes` (background left out): Hoiem's sets when they are the 20 VOC names, else None (every
    class on its own: SIM stays empty)."""
    where = {c: g for g, names in enumerate(VOC_GROUPS.values()) for c in names}
    if len(classes) != len(where) or set(classes) != set(where):
        return None
    return np.array([where[c] for c in classes], np.int32)


def _class_group(classes, groups):
    if groups is None:
        return default_groups(classes)
    if isinstance(groups, dict):                         # class name -> any hashable label; a class left out is on its own
        labels = {}
        return np.array([labels.setdefault(groups.get(c, ("own", c)), len(labels)) for c in classes], np.int32)
    g = np.asarray(groups, np.int32).ravel()
    if g.size != len(classes):
        raise ValueError("diagnose: groups needs one entry per class (%d), got %d" % (len(classes), g.size))
    return g


def segments(imdb, all_boxes):
    """The evaluation's segments of (imdb, all_boxes): a pascal_voc imdb's ground truth from its XML records (with the
    difficult flags, the 11-point metric up to VOC2007), any other imdb's from gt_roidb as tools/eval_det.py takes it;
    the detections rounded as a results file holds them.  -> (classes, metric_07, det_box, det_conf, det_off, gt_box,
    gt_difficult, gt_off)."""
    from datasets.pascal_voc import pascal_voc
    classes = [c for c in imdb.classes if c != "__background__"]
    if isinstance(imdb, pascal_voc):                     # by class: a coco imdb has a _devkit_path and a _year too
        recs, metric_07 = voc_eval.load_records(imdb), int(imdb._year) <= 2007
    else:
        recs, metric_07 = voc_eval.roidb_records(imdb), True
    gb, gd, goff = voc_eval.gt_segments(classes, recs)
    db, dc, doff = voc_eval.det_segments(imdb.num_images, voc_eval.all_boxes_dets(imdb, all_boxes))
    return classes, metric_07, db, dc, doff, gb, gd, goff


def diagnose(imdb, all_boxes, bg_overlap=0.1, groups=None, cuts=DEFAULT_CUTS, area_edges=DEFAULT_AREA_EDGES, ctx=None,
             protocol="voc"):
    """Tables of saved detections.  protocol "coco": see diagnose_coco (cuts do not apply).  "voc" returns a dict: az_det_diag_eval's outputs (type, ov_same, arg_same, ov_other,
    other_class, loc_fixed, gt_claim, type_table, miss, fp_at, npos, ap_fix; ap_fix[:, 0] is the AP evaluation reports),
    the segments they index (det_off, gt_off, gt_box, gt_difficult), the parameters, and from the host: `dap`
    [C,7] = ap_fix[:, 1:] - ap_fix[:, :1] with its mean over the classes `mean_dap` (NaN entries left out), `miss_by_size`
    / `gt_by_size` [C,3] (missed and all non-difficult objects, small / medium / large by area_edges), `confusion` [C,C]
    (SIM + OTH rows: detection class x other_class).  groups: None (Hoiem's sets for the 20 VOC classes, else every
    class on its own), a dict class name -> label, or one int per class.  ctx: the AzContext to run on."""
    if protocol == "coco":
        return diagnose_coco(imdb, all_boxes, bg_overlap=bg_overlap, groups=groups, area_edges=area_edges, ctx=ctx)
    if protocol != "voc":
        raise ValueError("diagnose: protocol must be 'voc' or 'coco', got %r" % (protocol,))
    classes, metric_07, db, dc, doff, gb, gd, goff = segments(imdb, all_boxes)
    C, N = len(classes), imdb.num_images
    if doff[-1] >= 2 ** 31 or goff[-1] >= 2 ** 31:
        raise ValueError("diagnose: more than int32 detections")
    group = _class_group(classes, groups)
    if ctx is None:
        from aznet_hip import ffi
        ctx = ffi.default_context()
    d = ctx.det_diag_eval(C, N, db, dc, doff, gb, gd, goff, min_overlap=voc_eval.MIN_OVERLAP, bg_overlap=bg_overlap,
                          metric_07=metric_07, class_group=group, cuts=cuts)
    d.update(classes=classes, class_group=group, imdb=getattr(imdb, "name", None), num_images=N, metric_07=bool(metric_07),
             min_overlap=voc_eval.MIN_OVERLAP, bg_overlap=float(bg_overlap), cuts=np.asarray(cuts, np.float64),
             area_edges=tuple(float(e) for e in area_edges), det_off=np.asarray(doff, np.int64),
             gt_off=np.asarray(goff, np.int64), gt_box=gb, gt_difficult=gd)
    d.update(host_tables(d))
    return d


def host_tables(d):
    """What diagnose adds on the host from gt_claim, type, other_class and the boxes (they are small)."""
    C, N = len(d["classes"]), int(d["num_images"])
    gb = np.asarray(d["gt_box"], np.float64).reshape(-1, 4)
    goff, doff = np.asarray(d["gt_off"], np.int64), np.asarray(d["det_off"], np.int64)
    gt_class = np.repeat(np.arange(C), goff[N::N] - goff[:-1:N]) if N else np.zeros(0, np.int64)
    det_class = np.repeat(np.arange(C), doff[N::N] - doff[:-1:N]) if N else np.zeros(0, np.int64)
    area = (gb[:, 2] - gb[:, 0] + 1.0) * (gb[:, 3] - gb[:, 1] + 1.0)
    size = np.where(area < d["area_edges"][0], 0, np.where(area < d["area_edges"][1], 1, 2))
    counts = ~np.asarray(d["gt_difficult"]).astype(bool)
    missed = counts & (np.asarray(d["gt_claim"]) < 0)
    by_size, miss_by_size = np.zeros((C, 3), np.int64), np.zeros((C, 3), np.int64)
    np.add.at(by_size, (gt_class[counts], size[counts]), 1)
    np.add.at(miss_by_size, (gt_class[missed], size[missed]), 1)
    ty = np.asarray(d["type"])
    conf = (ty == SIM) | (ty == OTH)
    confusion = np.zeros((C, C), np.int64)
    np.add.at(confusion, (det_class[conf], np.asarray(d["other_class"])[conf]), 1)
    ap = np.asarray(d["ap_fix"], np.float64)
    dap = ap[:, 1:] - ap[:, :1]
    ok = ~np.isnan(dap)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_dap = np.where(ok, dap, 0.0).sum(0) / ok.sum(0)
    return {"gt_by_size": by_size, "miss_by_size": miss_by_size, "confusion": confusion, "dap": dap, "mean_dap": mean_dap}


def coco_segments(imdb, all_boxes):
    """az_coco_eval's segments of (imdb, all_boxes), without a file.  A coco imdb is packed exactly as
    evaluate_detections packs it: _write_coco_results_file's entries ([x, y, w, h] truncated to 1/100), then
    coco_eval.pack against the annotation file (its area fields and crowd flags; images and categories in sorted id
    order).  Any other imdb with ground truth is packed from gt_roidb in its own image order: w = x2 - x1 + 1,
    area = w * h, no crowd boxes.  -> (classes, pack's dict, the categories' supercategories or None)."""
    from datasets import coco as coco_mod
    from datasets import coco_eval
    classes = [c for c in imdb.classes if c != "__background__"]
    if isinstance(imdb, coco_mod.coco):
        if imdb._image_set not in ("train", "val"):
            raise ValueError("diagnose: %s has no ground truth to diagnose against" % imdb.name)
        cat_ids = imdb._coco[0].getCatIds()
        results = []
        for cls_ind in range(1, len(imdb.classes)):
            for im_ind, index in enumerate(imdb.image_index):
                cls_dets = all_boxes[cls_ind][im_ind]
                if not coco_mod._is_empty(cls_dets):
                    for k in range(cls_dets.shape[0]):
                        results.append(coco_mod._result_entry(cls_dets, k, index, cat_ids[cls_ind - 1]))
        p = coco_eval.pack(imdb._coco[0], results)
        cats = sorted(imdb._coco[0].dataset.get("categories", []), key=lambda c: c["id"])
        sup = [c.get("supercategory") for c in cats]
        return classes, p, (sup if len(sup) == len(classes) and all(x is not None for x in sup) else None)
    K, N = len(classes), imdb.num_images
    roidb = imdb.gt_roidb()
    dbox, dscore, doff, gbox, goff = [], [], [0], [], [0]
    for k in range(1, K + 1):
        for i in range(N):
            dets = all_boxes[k][i]
            n = 0 if (isinstance(dets, list) and len(dets) == 0) else dets.shape[0]
            for r in range(n):
                e = coco_mod._result_entry(dets, r, i, k)
                dbox.append(e["bbox"])
                dscore.append(e["score"])
            doff.append(doff[-1] + n)
            b = np.asarray(roidb[i]["boxes"], np.float64).reshape(-1, 4)[np.asarray(roidb[i]["gt_classes"]) == k]
            for x1, y1, x2, y2 in b:
                gbox.append([x1, y1, x2 - x1 + 1.0, y2 - y1 + 1.0])
            goff.append(goff[-1] + b.shape[0])
    gbox = np.array(gbox, np.float64).reshape(-1, 4)
    p = {"n_classes": K, "n_images": N, "det_box": np.array(dbox, np.float64).reshape(-1, 4),
         "det_score": np.array(dscore, np.float64), "det_off": np.array(doff, np.int64), "gt_box": gbox,
         "gt_area": gbox[:, 2] * gbox[:, 3], "gt_crowd": np.zeros(gbox.shape[0], np.uint8), "gt_off": np.array(goff, np.int64)}
    return classes, p, None


def diagnose_coco(imdb, all_boxes, bg_overlap=0.1, groups=None, area_edges=DEFAULT_AREA_EDGES, ctx=None):
    """diagnose(..., protocol="coco"): the tables under COCOeval's rules (area range all, maxDets 100, the ten thresholds).
    Returns a dict with protocol = "coco": az_coco_diag_eval's outputs (ov_same, arg_same, ov_other, other_class, type
    [10,D], loc_fixed [10,D], gt_claim [10,G], npos, type_table [K,10,7], miss [K,10], prec_fix, recall_fix, ap_fix
    [K,10,8], stats_fix [8,3]: stats_fix[0] is the AP / AP50 / AP75 evaluation prints), the segments they index (det_off,
    gt_off, gt_box, gt_area, gt_crowd), the parameters, and from the host: `dap_stats` [7,3] = stats_fix[1:] -
    stats_fix[0], per class `dap` [K,10,7], `miss_by_size` [K,10,3] / `gt_by_size` [K,3] (missed and all counting
    objects by gt_area against area_edges), `confusion` [K,K] (SIM + OTH rows at IoU 0.5).  groups: None (a coco imdb: the
    annotation file's supercategories when every category has one; the 20 VOC names: Hoiem's sets; else every class on
    its own), a dict class name -> label, or one int per class.  The cut table of the VOC protocol (fp_at) is not
    part of this one."""
    classes, p, sup = coco_segments(imdb, all_boxes)
    if groups is None and sup is not None:
        groups = dict(zip(classes, sup))
    group = _class_group(classes, groups)
    if ctx is None:
        from aznet_hip import ffi
        ctx = ffi.default_context()
    d = ctx.coco_diag_eval(p["n_classes"], p["n_images"], p["det_box"], p["det_score"], p["det_off"], p["gt_box"],
                           p["gt_area"], p["gt_crowd"], p["gt_off"], bg_overlap=bg_overlap, class_group=group)
    d.update(protocol="coco", classes=classes, class_group=group, imdb=getattr(imdb, "name", None),
             num_images=int(p["n_images"]), bg_overlap=float(bg_overlap), area_edges=tuple(float(e) for e in area_edges),
             det_off=np.asarray(p["det_off"], np.int64), gt_off=np.asarray(p["gt_off"], np.int64), gt_box=p["gt_box"],
             gt_area=p["gt_area"], gt_crowd=p["gt_crowd"])
    d.update(coco_host_tables(d))
    return d


def coco_host_tables(d):
    """What diagnose_coco adds on the host from gt_claim, type, other_class, the areas and the curves' means."""
    K, N = len(d["classes"]), int(d["num_images"])
    goff, doff = np.asarray(d["gt_off"], np.int64), np.asarray(d["det_off"], np.int64)
    gt_class = np.repeat(np.arange(K), goff[N::N] - goff[:-1:N]) if N else np.zeros(0, np.int64)
    det_class = np.repeat(np.arange(K), doff[N::N] - doff[:-1:N]) if N else np.zeros(0, np.int64)
    area = np.asarray(d["gt_area"], np.float64)
    size = np.where(area < d["area_edges"][0], 0, np.where(area < d["area_edges"][1], 1, 2))
    counts = ~np.asarray(d["gt_crowd"]).astype(bool) & (area >= 0.0) & (area <= 1e10)
    claim = np.asarray(d["gt_claim"]).reshape(10, -1)
    by_size, miss_by_size = np.zeros((K, 3), np.int64), np.zeros((K, 10, 3), np.int64)
    np.add.at(by_size, (gt_class[counts], size[counts]), 1)
    for t in range(10):
        missed = counts & (claim[t] < 0)
        np.add.at(miss_by_size[:, t], (gt_class[missed], size[missed]), 1)
    ty = np.asarray(d["type"]).reshape(10, -1)[0]
    conf = (ty == SIM) | (ty == OTH)
    confusion = np.zeros((K, K), np.int64)
    np.add.at(confusion, (det_class[conf], np.asarray(d["other_class"])[conf]), 1)
    ap, st = np.asarray(d["ap_fix"], np.float64), np.asarray(d["stats_fix"], np.float64)
    return {"gt_by_size": by_size, "miss_by_size": miss_by_size, "confusion": confusion, "dap": ap[:, :, 1:] - ap[:, :, :1],
            "dap_stats": st[1:] - st[0]}


def _coco_summary_lines(d):
    classes = list(d["classes"])
    w = max([len(c) for c in classes] + [5])
    st, dst = np.asarray(d["stats_fix"], np.float64), np.asarray(d["dap_stats"], np.float64)
    lines = ["COCO protocol (area all, maxDets 100): AP and what fixing one kind of error would add (dAP, points):"]
    lines.append("  %-10s %6s" % ("", "AP") + "".join("%10s" % n for n in VARIANT_NAMES[1:]))
    for j, name in enumerate(("IoU .50:.95", "IoU .50", "IoU .75")):
        lines.append("  %-11s%s" % (name, _pct(st[0, j] if st[0, j] > -1 else float("nan")))
                     + "".join("    %s" % _pct(v) for v in dst[:, j]))
    tt = np.asarray(d["type_table"], np.int64).reshape(len(classes), 10, 7)
    miss = np.asarray(d["miss"], np.int64).reshape(len(classes), 10)
    order = list(range(1, 7)) + [0]
    for t, iou in ((0, 0.5), (5, 0.75)):
        lines.append("Detections by type at IoU %.2f (IoU >= %.3g with an object of the class a localisation error, with "
                     "another class's a confusion):" % (iou, d.get("bg_overlap", 0.1)))
        lines.append("  %-*s %7s %7s" % (w, "class", "objects", "missed") + "".join("%8s" % n for n in TYPE_NAMES[1:] + TYPE_NAMES[:1]))
        for k, c in enumerate(classes):
            if int(d["npos"][k]) == 0 and tt[k, t].sum() == 0:
                continue                                         # 80 categories: the ones without anything stay out
            lines.append("  %-*s %7d %7d" % (w, c, int(d["npos"][k]), int(miss[k, t])) + "".join("%8d" % int(tt[k, t, ty]) for ty in order))
        lines.append("  %-*s %7d %7d" % (w, "all", int(np.sum(d["npos"])), int(miss[:, t].sum()))
                     + "".join("%8d" % int(tt[:, t, ty].sum()) for ty in order))
    ms, gs = np.asarray(d["miss_by_size"], np.int64)[:, 0].sum(0), np.asarray(d["gt_by_size"], np.int64).sum(0)
    lines.append("Missed objects by size at IoU 0.50 (areas below %g / %g / above): " % tuple(d.get("area_edges", DEFAULT_AREA_EDGES))
                 + ", ".join("%s %d of %d" % (SIZE_NAMES[k], int(ms[k]), int(gs[k])) for k in range(3)))
    cf = np.asarray(d["confusion"], np.int64)
    top = [(int(cf[a, b]), a, b) for a, b in zip(*np.nonzero(cf))]
    top.sort(key=lambda r: (-r[0], r[1], r[2]))
    lines.append("Confusions at IoU 0.50 (a detection of one class on an object of another): %d" % int(cf.sum()))
    for n, a, b in top[:10]:
        lines.append("  %7d  %s on %s" % (n, classes[a], classes[b]))
    return lines


def _pct(x):
    return "   n/a" if x != x else "%6.1f" % (100.0 * x)


def _share(a, b):
    return "   n/a" if not b else "%6.3f" % (float(a) / float(b))


def summary_lines(d):
    """The tables of diagnose() as lines of text (either protocol)."""
    if d.get("protocol") == "coco":
        return _coco_summary_lines(d)
    classes = list(d["classes"])
    w = max([len(c) for c in classes] + [5])
    tt = np.asarray(d["type_table"], np.int64)
    lines = ["Detections by type (overlap >= %.3g a match, >= %.3g a localisation error or a confusion):"
             % (d.get("min_overlap", 0.5), d.get("bg_overlap", 0.1))]
    lines.append("  %-*s %7s %7s" % (w, "class", "objects", "missed") + "".join("%8s" % n for n in TYPE_NAMES[1:] + TYPE_NAMES[:1]))
    order = list(range(1, 7)) + [0]
    for k, c in enumerate(classes):
        lines.append("  %-*s %7d %7d" % (w, c, int(d["npos"][k]), int(d["miss"][k])) + "".join("%8d" % int(tt[k, t]) for t in order))
    lines.append("  %-*s %7d %7d" % (w, "all", int(np.sum(d["npos"])), int(np.sum(d["miss"])))
                 + "".join("%8d" % int(tt[:, t].sum()) for t in order))
    ap = np.asarray(d["ap_fix"], np.float64)
    dap = np.asarray(d["dap"], np.float64)
    lines.append("AP (%s) and what fixing one kind of error would add (dAP, points):"
                 % ("11-point" if d.get("metric_07", True) else "area"))
    lines.append("  %-*s %6s" % (w, "class", "AP") + "".join("%10s" % n for n in VARIANT_NAMES[1:]))
    for k, c in enumerate(classes):
        lines.append("  %-*s %s" % (w, c, _pct(ap[k, 0])) + "".join("    %s" % _pct(v) for v in dap[k]))
    plain = ap[:, 0]
    mean_ap = float(plain[~np.isnan(plain)].mean()) if (~np.isnan(plain)).any() else float("nan")
    lines.append("  %-*s %s" % (w, "mean", _pct(mean_ap)) + "".join("    %s" % _pct(v) for v in np.asarray(d["mean_dap"])))
    fa = np.asarray(d["fp_at"], np.int64).sum(0) if len(classes) else np.zeros((0, 7), np.int64)
    lines.append("What the top-ranked detections are made of (the first cut x objects of every class, shares of the false positives):")
    lines.append("     cut    rows      TP      FP" + "".join("%8s" % n for n in TYPE_NAMES[2:]))
    for k, cut in enumerate(np.asarray(d["cuts"]).ravel()):
        fp = int(fa[k, 2:].sum())
        lines.append("  %6.4g %7d %7d %7d" % (float(cut), int(fa[k].sum()), int(fa[k, TP]), fp)
                     + "".join("  %s" % _share(fa[k, t], fp) for t in range(2, 7)))
    ms, gs = np.asarray(d["miss_by_size"], np.int64).sum(0), np.asarray(d["gt_by_size"], np.int64).sum(0)
    lines.append("Missed objects by size (areas below %g / %g / above): " % tuple(d.get("area_edges", DEFAULT_AREA_EDGES))
                 + ", ".join("%s %d of %d" % (SIZE_NAMES[k], int(ms[k]), int(gs[k])) for k in range(3)))
    cf = np.asarray(d["confusion"], np.int64)
    top = [(int(cf[a, b]), a, b) for a, b in zip(*np.nonzero(cf))]
    top.sort(key=lambda r: (-r[0], r[1], r[2]))
    lines.append("Confusions (a detection of one class on an object of another): %d" % int(cf.sum()))
    for n, a, b in top[:10]:
        lines.append("  %7d  %s on %s" % (n, classes[a], classes[b]))
    return lines
