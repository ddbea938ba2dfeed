"""Why is a detector's AP what it is?  Every detection of a VOC evaluation typed after Hoiem et al., "Diagnosing Error in
Object Detectors" (ECCV 2012) -- true positive, duplicate, localisation error, confusion with a similar class, with
another class, with background -- and the AP recomputed with each kind of error fixed, after TIDE (Bolya et al.,
ECCV 2020): which errors cost how much.

    diagnose(imdb, all_boxes)   the tables for a whole image set, in one az_det_diag_eval call ("Detection
                                diagnosis")
    summary_lines(d)            the tables as text

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


def diagnose(imdb, all_boxes, bg_overlap=0.1, groups=None, cuts=DEFAULT_CUTS, area_edges=DEFAULT_AREA_EDGES, ctx=None):
    """Tables of saved detections.  Returns a dict: az_det_diag_eval's outputs (type, ov_same, arg_same, ov_other,
    other_class, loc_fixed, gt_claim, type_table, miss, fp_at, npos, ap_fix; ap_fix[:, 0] is the AP evaluation reports),
    the segments they index (det_off, gt_off, gt_box, gt_difficult), the parameters, and from the host: `dap`
    [C,7] = ap_fix[:, 1:] - ap_fix[:, :1] with its mean over the classes `mean_dap` (NaN entries left out), `miss_by_size`
    / `gt_by_size` [C,3] (missed and all non-difficult objects, small / medium / large by area_edges), `confusion` [C,C]
    (SIM + OTH rows: detection class x other_class).  groups: None (Hoiem's sets for the 20 VOC classes, else every
    class on its own), a dict class name -> label, or one int per class.  ctx: the AzContext to run on."""
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


def _pct(x):
    return "   n/a" if x != x else "%6.1f" % (100.0 * x)


def _share(a, b):
    return "   n/a" if not b else "%6.3f" % (float(a) / float(b))


def summary_lines(d):
    """The tables of diagnose() as lines of text."""
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
