"""NumPy restatement of pycocotools' COCOeval (iouType 'bbox') evaluateImg / accumulate / summarize, on az_coco_eval's
class-major segments.  Written loop for loop after the Python original so that the kernel can be held to
it bit for bit; slow, for tests only."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ["all", "small", "medium", "large"]


def bb_iou(d, g, iscrowd):
    """maskApi.c bbIou: [len(d), len(g)] for xywh boxes, a crowd box's union the detection's area."""
    o = np.zeros((len(d), len(g)))
    for gi in range(len(g)):
        G = g[gi]
        ga = G[2] * G[3]
        for di in range(len(d)):
            D = d[di]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if iscrowd[gi] else da + ga - i
            o[di, gi] = i / u
    return o


def evaluate_img(dt, gt, a_rng, max_det):
    """dt: list of dicts (bbox, score, area, id, pos) in file order; gt: (bbox, area, iscrowd, id, pos).  Returns
    evaluateImg's dict plus 'dtPos' / 'dtGtPos' (file positions) for the match outputs, or None."""
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        g["_ignore"] = 1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0
    gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[0:max_det]]
    iscrowd = [int(o["iscrowd"]) for o in gt]
    ious = bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], iscrowd) if len(dt) and len(gt) else []
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    dtpos = -np.ones((T, D), np.int64)
    gtIg = np.array([g["_ignore"] for g in gt])
    dtIg = np.zeros((T, D))
    if not len(ious) == 0:
        for tind, t in enumerate(IOU_THRS):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = gt[m]["id"]
                dtpos[tind, dind] = gt[m]["pos"]
                gtm[tind, m] = d["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtMatches": dtm, "gtMatches": gtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gtIg,
            "dtIgnore": dtIg, "dtPos": [d["pos"] for d in dt], "dtGtPos": dtpos}


def coco_eval(n_classes, n_images, det_box, det_score, det_off, gt_box, gt_area, gt_crowd, gt_off):
    """Same inputs as AzContext.coco_eval; returns precision, recall, stats, dt_match, dt_ignore as it does."""
    K, I0, A0 = n_classes, n_images, len(AREA_RNG)
    det_box = np.asarray(det_box, np.float64).reshape(-1, 4)
    gt_box = np.asarray(gt_box, np.float64).reshape(-1, 4)
    D = len(det_score)
    segs = []
    for s in range(K * I0):
        dts = [{"bbox": [float(v) for v in det_box[p]], "score": float(det_score[p]),
                "area": float(det_box[p, 2]) * float(det_box[p, 3]), "id": p + 1, "pos": p}
               for p in range(det_off[s], det_off[s + 1])]
        gts = [{"bbox": [float(v) for v in gt_box[q]], "area": float(gt_area[q]), "iscrowd": int(gt_crowd[q]),
                "id": q + 1, "pos": q - gt_off[s]} for q in range(gt_off[s], gt_off[s + 1])]
        segs.append((dts, gts))
    # evaluate(): for catId, for areaRng, for imgId
    evalImgs = [evaluate_img(segs[k * I0 + i][0], segs[k * I0 + i][1], a_rng, MAX_DETS[-1])
                for k in range(K) for a_rng in AREA_RNG for i in range(I0)]
    dt_match = -np.ones((A0, len(IOU_THRS), D), np.int32)
    dt_ignore = -np.ones((A0, len(IOU_THRS), D), np.int8)
    for k in range(K):
        for a in range(A0):
            for i in range(I0):
                e = evalImgs[(k * A0 + a) * I0 + i]
                if e is None:
                    continue
                for dind, p in enumerate(e["dtPos"]):
                    dt_match[a, :, p] = e["dtGtPos"][:, dind]
                    dt_ignore[a, :, p] = e["dtIgnore"][:, dind]
    # accumulate()
    T, R, M = len(IOU_THRS), len(REC_THRS), len(MAX_DETS)
    precision = -np.ones((T, R, K, A0, M))
    recall = -np.ones((T, K, A0, M))
    for k in range(K):
        Nk = k * A0 * I0
        for a in range(A0):
            Na = a * I0
            for m, maxDet in enumerate(MAX_DETS):
                E = [evalImgs[Nk + Na + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, REC_THRS, side="left")
                    try:
                        for ri, pi in enumerate(inds):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return {"precision": precision, "recall": recall, "stats": summarize(precision, recall),
            "dt_match": dt_match, "dt_ignore": dt_ignore}


def summarize_one(precision, recall, ap=1, iouThr=None, areaRng="all", maxDets=100):
    aind = [i for i, aRng in enumerate(AREA_LBL) if aRng == areaRng]
    mind = [i for i, mDet in enumerate(MAX_DETS) if mDet == maxDets]
    if ap == 1:
        s = precision
        if iouThr is not None:
            s = s[np.where(iouThr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind]
    else:
        s = recall
        if iouThr is not None:
            s = s[np.where(iouThr == IOU_THRS)[0]]
        s = s[:, :, aind, mind]
    return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])


def summarize(precision, recall):
    args = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100),
            (1, None, "medium", 100), (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10),
            (0, None, "all", 100), (0, None, "small", 100), (0, None, "medium", 100), (0, None, "large", 100)]
    return np.array([summarize_one(precision, recall, *a) for a in args], np.float64)
