"""NumPy restatement of the VOCdevkit's VOCevaldet.m and the wrapper's xVOCap.m, walking
detections one at a time as VOCevaldet does.  Test infrastructure only: no product file imports it."""
import numpy as np


def colon_thresholds():
    """MATLAB's 0:0.1:1: a + k*d for the first half, b - (n-k)*d for the second, (a+b)/2 in the middle."""
    t = [k * 0.1 for k in range(6)] + [1.0 - (10 - k) * 0.1 for k in range(6, 11)]
    t[5] = 0.5
    return t


def _mmax(v):
    """MATLAB's max: NaN ignored unless every value is NaN; [] for an empty set."""
    if v.size == 0:
        return None
    w = v[~np.isnan(v)]
    return float(w.max()) if w.size else float("nan")


def xvocap(rec, prec):
    mrec = np.concatenate([[0.0], rec, [1.0]])
    mpre = np.concatenate([[0.0], prec, [0.0]])
    for i in range(mpre.size - 2, -1, -1):
        a, b = mpre[i], mpre[i + 1]
        mpre[i] = b if np.isnan(a) else (a if np.isnan(b) else max(a, b))
    i = np.where(mrec[1:] != mrec[:-1])[0] + 1
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]))


def ap11(rec, prec):
    ap = 0.0
    for t in colon_thresholds():
        p = _mmax(prec[rec >= t])
        ap = ap + (0.0 if p is None else p) / 11
    return ap


def evaldet(det_img, det_conf, det_box, gt_boxes, gt_diff, min_overlap=0.5, metric_07=True):
    """One class.  det_img [D] image number, det_conf [D], det_box [D,4] (1-based results-file values),
    in file order; gt_boxes / gt_diff: per image, [k,4] 1-based and [k] flags.
    -> dict(match [D] input order, rec, prec [D] rank order, npos, ap, ap_auc)."""
    det_conf = np.asarray(det_conf, np.float64)
    D = det_conf.size
    npos = int(sum(int((~np.asarray(d, bool)).sum()) for d in gt_diff))
    order = np.argsort(-det_conf, kind="stable")
    claimed = [np.zeros(len(d), bool) for d in gt_diff]
    tp = np.zeros(D)
    fp = np.zeros(D)
    match = np.zeros(D, np.int8)
    for r, d in enumerate(order):
        i = int(det_img[d])
        bb = [float(v) for v in det_box[d]]
        ovmax, jmax = -np.inf, -1
        for j, g in enumerate(np.asarray(gt_boxes[i], np.float64).reshape(-1, 4)):
            g = [float(v) for v in g]
            iw = min(bb[2], g[2]) - max(bb[0], g[0]) + 1
            ih = min(bb[3], g[3]) - max(bb[1], g[1]) + 1
            if iw > 0 and ih > 0:
                ua = (bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + (g[2] - g[0] + 1) * (g[3] - g[1] + 1) - iw * ih
                ov = iw * ih / ua
                if ov > ovmax:
                    ovmax, jmax = ov, j
        if ovmax >= min_overlap:
            if not gt_diff[i][jmax]:
                if not claimed[i][jmax]:
                    tp[r] = 1
                    claimed[i][jmax] = True
                    match[d] = 1
                else:
                    fp[r] = 1
                    match[d] = -1
        else:
            fp[r] = 1
            match[d] = -1
    fp = np.cumsum(fp)
    tp = np.cumsum(tp)
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = tp / float(npos)
        prec = tp / (fp + tp)
    auc = xvocap(rec, prec)
    ap = ap11(rec, prec) if metric_07 else auc
    return {"match": match, "rec": rec, "prec": prec, "npos": npos, "ap": ap, "ap_auc": auc}


def evaluate_flat(n_classes, n_images, det_box, det_conf, det_off, gt_box, gt_diff, gt_off, min_overlap=0.5,
                  metric_07=True):
    """The segment layout of az_voc_eval (class-major segments) through evaldet, class by class."""
    out = {"match": np.zeros(int(det_off[-1]), np.int8), "rec": np.zeros(int(det_off[-1])),
           "prec": np.zeros(int(det_off[-1])), "npos": np.zeros(n_classes, np.int64),
           "ap": np.zeros(n_classes), "ap_auc": np.zeros(n_classes)}
    for c in range(n_classes):
        s0, s1 = c * n_images, (c + 1) * n_images
        lo, hi = int(det_off[s0]), int(det_off[s1])
        img = np.repeat(np.arange(n_images), np.diff(det_off[s0:s1 + 1]))
        gb = [gt_box[gt_off[s]:gt_off[s + 1]] for s in range(s0, s1)]
        gd = [np.asarray(gt_diff[gt_off[s]:gt_off[s + 1]], bool) for s in range(s0, s1)]
        r = evaldet(img, det_conf[lo:hi], det_box[lo:hi], gb, gd, min_overlap, metric_07)
        out["match"][lo:hi] = r["match"]
        out["rec"][lo:hi] = r["rec"]
        out["prec"][lo:hi] = r["prec"]
        out["npos"][c] = r["npos"]
        out["ap"][c] = r["ap"]
        out["ap_auc"][c] = r["ap_auc"]
    return out
