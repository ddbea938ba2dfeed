"""The analysis AZ_results.mat was recorded for (lib/detect/tune.py:368-419 writes the file; the reference read it
offline): why did proposals miss objects -- did the zoom indicator stop above them, or did the search reach them and
the adjacency prediction fail?

    diagnose(results)      the tables for a whole image set, in one az_diag_eval call ("Proposal diagnosis")
    summary_lines(d)       the tables as text

`results` is what detect.tune.test_proposals returns (or AZ_results.mat loaded back, plus `level_regions`).  The wording
of the summary is this backend's own: the reference prints nothing here.
"""
import numpy as np

from detect.config import cfg

DEFAULT_CUTS = (10, 50, 100, 300, 1000, 2000)
DEFAULT_AREA_EDGES = (32 ** 2, 96 ** 2)
SIZE_NAMES = ("all", "small", "medium", "large")


def anchor_levels(results):
    """Per image the search level of every anchor: anchor_boxes is level-major (tune.py:299), level_regions counts the
    anchors of each level."""
    if "level_regions" not in results:
        raise ValueError("diagnose: the results carry no level_regions (detect.tune.test_proposals records them)")
    out = []
    for i, regions in enumerate(results["level_regions"]):
        regions = np.asarray(regions, dtype=np.int64).ravel()
        m = np.asarray(results["anchor_boxes"][i]).reshape(-1, 5).shape[0]
        if int(regions.sum()) != m:
            raise ValueError("diagnose: image %d has %d anchors but level_regions counts %d" % (i, m, int(regions.sum())))
        out.append(np.repeat(np.arange(regions.size, dtype=np.int32), regions))
    return out


def _need_level(root_area, gt_area, max_ratio):
    """The level at which an anchor of the object's size sits: the first at which a region of the root's area / 4^level
    (divide_region halves both sides) is no longer asked to zoom for the object, area(gt) / area(region) > max_ratio."""
    level = np.zeros(gt_area.shape, dtype=np.int32)
    area = np.array(root_area, dtype=np.float64)
    for _ in range(32):
        more = (gt_area / (area + 1e-14) <= max_ratio) & (area >= 1.0)
        if not more.any():
            break
        level += more
        area = np.where(more, area / 4.0, area)
    return level


def diagnose(results, imdb=None, cuts=DEFAULT_CUTS, iou_thresh=0.5, area_edges=DEFAULT_AREA_EDGES, ctx=None):
    """Tables of a recorded proposal run.  Returns a dict: az_diag_eval's outputs (anchor_label, level_table, best_iou,
    best_rank, first_hit, deepest_level, recall_table, the offsets), the parameters, per object its image (`gt_image`),
    area and the level an anchor of its size sits at (`need_level`), and `fn`.  imdb: only its name is kept.  ctx: the
    AzContext to run on (default: a new one on the current device)."""
    if ctx is None:
        from aznet_hip import ffi
        import torch
        ctx = ffi.AzContext(torch.cuda.current_device() if torch.cuda.is_available() else 0)
    n = len(results["anchor_boxes"])
    levels = anchor_levels(results)
    anchors = [np.asarray(results["anchor_boxes"][i], dtype=np.float64).reshape(-1, 5) for i in range(n)]
    props = [np.asarray(results["prop_boxes"][i], dtype=np.float64).reshape(-1, 5)[:, :4] for i in range(n)]
    gts = [np.asarray(results["gt_boxes"][i], dtype=np.float64).reshape(-1, 4) for i in range(n)]
    tz = float(np.asarray(results["Tz"]).ravel()[0])
    # the zoom score was a float32 widened by the search's hstack: narrowing it back is exact
    d = ctx.diag_eval([a[:, :4] for a in anchors], [a[:, 4].astype(np.float32) for a in anchors], levels, gts, props, tz,
                      cfg.SEAR.EMB_REG_THRESH, cfg.SEAR.EMB_OBJ_THRESH, iou_thresh=iou_thresh, cuts=cuts, area_edges=area_edges)
    d["Tz"], d["iou_thresh"], d["area_edges"] = tz, float(iou_thresh), tuple(float(e) for e in area_edges)
    d["num_images"] = n
    d["imdb"] = getattr(imdb, "name", None)
    d["fn"] = list(results.get("fn", []))
    counts = np.diff(d["gt_off"])
    d["gt_image"] = np.repeat(np.arange(n, dtype=np.int32), counts)
    g = np.vstack([np.zeros((0, 4))] + gts)
    d["gt_area"] = (g[:, 2] - g[:, 0] + 1.0) * (g[:, 3] - g[:, 1] + 1.0)
    root_area = np.array([(a[0, 2] - a[0, 0] + 1.0) * (a[0, 3] - a[0, 1] + 1.0) if a.shape[0] else 0.0 for a in anchors])
    d["need_level"] = _need_level(root_area[d["gt_image"]], d["gt_area"], float(cfg.SEAR.EMB_REG_THRESH))
    return d


def _ratio(a, b):
    return "%6.3f" % (float(a) / float(b)) if b else "   n/a"


def summary_lines(d):
    """The tables of diagnose() as lines of text."""
    lines = []
    lt = np.asarray(d["level_table"], dtype=np.int64)
    lines.append("Zoom indicator by search level (Tz = %.6g; level 0 zooms at 0):" % d.get("Tz", float("nan")))
    lines.append("  level   anchors    zoomed  labelled      both  precision  recall")
    used = [l for l in range(lt.shape[0]) if lt[l, 0]]
    for l in used:
        a, z, lab, both = (int(v) for v in lt[l])
        lines.append("  %5d %9d %9d %9d %9d     %s  %s" % (l, a, z, lab, both, _ratio(both, z), _ratio(both, lab)))
    if not used:
        lines.append("  (no anchors)")
    rt = np.asarray(d["recall_table"], dtype=np.int64)
    cuts = [int(c) for c in d["cuts"]]
    total = rt[-1]
    lines.append("Recall at IoU >= %.3g by proposal budget and object size (areas below %g / %g / above):"
                 % (d.get("iou_thresh", 0.5), d.get("area_edges", DEFAULT_AREA_EDGES)[0], d.get("area_edges", DEFAULT_AREA_EDGES)[1]))
    lines.append("  budget " + "".join("%16s" % s for s in SIZE_NAMES))
    for c, cut in enumerate(cuts):
        lines.append("  %6d " % cut + "".join("  %s (%5d)" % (_ratio(rt[c, k], total[k]), int(rt[c, k])) for k in range(4)))
    lines.append("  objects" + "".join("%16d" % int(total[k]) for k in range(4)))
    fh = np.asarray(d["first_hit"])
    deep = np.asarray(d["deepest_level"])
    need = np.asarray(d.get("need_level", np.zeros(fh.shape, np.int32)))
    missed = fh < 0
    never = missed & (deep < need)
    reached = missed & ~never
    lines.append("Missed objects (no proposal at IoU >= %.3g): %d of %d" % (d.get("iou_thresh", 0.5), int(missed.sum()), fh.size))
    lines.append("  never reached (the zoom stopped above an anchor of their size): %d" % int(never.sum()))
    lines.append("  reached but not hit (the adjacency prediction failed):          %d" % int(reached.sum()))
    if missed.any():
        lines.append("     image  object      area  need  deepest  best_iou  best_rank")
        gi = np.asarray(d.get("gt_image", np.zeros(fh.shape, np.int32)))
        off = np.asarray(d["gt_off"])
        area = np.asarray(d.get("gt_area", np.zeros(fh.shape)))
        for j in np.nonzero(missed)[0][:50]:
            lines.append("  %8d %7d %9.0f %5d %8d  %8.4f %10d" % (int(gi[j]), int(j - off[gi[j]]), float(area[j]), int(need[j]),
                                                                 int(deep[j]), float(d["best_iou"][j]), int(d["best_rank"][j])))
        if int(missed.sum()) > 50:
            lines.append("  ... and %d more (diagnosis.pkl holds them all)" % (int(missed.sum()) - 50))
    return lines
