"""A NumPy restatement of online hard-example mining for the detection trainer (test infrastructure; the yardstick of
tests/test_ohem_host.py and tests/test_gpu_ohem.py).  Written from include/aznet_hip.h (az_det_solver_mine) and the issue's
definition, not from the HIP code.  Three parts:
  row losses    one loss per pool row from cls_score / bbox_pred: in float64, and in float32 in the kernel's operation order
                (the box term and the final add bit for bit; the softmax through NumPy's exp / log, so within rounding)
  pool builder  the rows a roidb entry hands over under TRAIN.OHEM
  selection     per image greedy NMS with the loss as score in az_nms's arithmetic (float32, one rounding per operation, a row
                dropped at IoU >= thresh) and tie rule (equal scores: the higher index first), then the first per_image
The reference project has no such mode: this file is the definition the device is held to."""
import numpy as np

import det_step_ref as D
from det_step_ref import bound, rel_err  # noqa: F401

F32 = np.float32
TINY = np.finfo(np.float32).tiny


# ---- row losses -------------------------------------------------------------------------------------------------------------
def bbox_loss32(bbox_pred, labels, targets):
    """bbox_r = ((f0 + f1) + f2) + f3 in float32, f = (0.5 d) d if |d| < 1 else |d| - 0.5, d = bbox_pred[r, 4 label + q] - t[r, q];
    0 for label 0 or without targets.  Every operation is one float32 operation: the device's bits."""
    bp = np.ascontiguousarray(bbox_pred, F32)
    lab = np.asarray(labels).astype(np.int64)
    out = np.zeros(lab.size, F32)
    if targets is None:
        return out
    t = np.ascontiguousarray(targets, F32).reshape(-1, 4)
    rows = np.flatnonzero(lab > 0)
    f = []
    for q in range(4):
        d = bp[rows, 4 * lab[rows] + q] - t[rows, q]
        ad = np.abs(d)
        f.append(np.where(ad < F32(1), (F32(0.5) * d) * d, ad - F32(0.5)).astype(F32))
    out[rows] = ((f[0] + f[1]) + f[2]) + f[3]
    return out


def cls_loss(cls_score, labels, dtype):
    """cls_r = -log(max(p[label], FLT_MIN)), p = exp(x - max) / sum, in `dtype`."""
    x = np.asarray(cls_score, dtype)
    lab = np.asarray(labels).astype(np.int64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True, dtype=dtype)).astype(dtype)
    return (-np.log(np.maximum(p[np.arange(x.shape[0]), lab], dtype(TINY)))).astype(dtype)


def bbox_loss64(bbox_pred, labels, targets):
    lab = np.asarray(labels).astype(np.int64)
    out = np.zeros(lab.size, np.float64)
    if targets is None:
        return out
    bp, t = np.asarray(bbox_pred, np.float64), np.asarray(targets, np.float64).reshape(-1, 4)
    rows = np.flatnonzero(lab > 0)
    d = bp[rows[:, None], 4 * lab[rows, None] + np.arange(4)[None, :]] - t[rows]
    ad = np.abs(d)
    out[rows] = np.where(ad < 1, 0.5 * d * d, ad - 0.5).sum(axis=1)
    return out


def row_losses(cls_score, bbox_pred, labels, targets, dtype=np.float64):
    """(loss, cls, bbox) per row in float64, or in float32 in the kernel's order (loss = float32(cls + bbox))."""
    if dtype == np.float64:
        c, b = cls_loss(cls_score, labels, np.float64), bbox_loss64(bbox_pred, labels, targets)
        return c + b, c, b
    c, b = cls_loss(np.asarray(cls_score, F32), labels, F32), bbox_loss32(bbox_pred, labels, targets)
    return (c + b).astype(F32), c, b


# ---- the pool builder -------------------------------------------------------------------------------------------------------
def pool_inds(max_overlaps, fg_thresh, bg_hi, bg_lo, pool):
    """(rows, number of foreground rows among them): the foreground in order, then the background band in order (everything
    below fg_thresh where the band is empty), cut at `pool`."""
    ov = np.asarray(max_overlaps)
    fg = [i for i in range(ov.size) if ov[i] >= fg_thresh]
    bg = [i for i in range(ov.size) if bg_lo <= ov[i] < bg_hi]
    if not bg:
        bg = [i for i in range(ov.size) if ov[i] < fg_thresh]
    return np.asarray((fg + bg)[:pool], dtype=np.int64), min(len(fg), pool)


# ---- selection --------------------------------------------------------------------------------------------------------------
def nms(dets, thresh):
    """Greedy NMS of records [x1, y1, x2, y2, score] (lib/utils/nms.pyx in float32, one rounding per operation): visited by
    descending score, of equal scores the higher index first; a later box is dropped when its IoU with a kept box is
    >= thresh (compared in float64).  Returns the kept indices in visiting order."""
    d = np.ascontiguousarray(dets, F32).reshape(-1, 5)
    n = d.shape[0]
    if n == 0:
        return np.zeros(0, np.int64)
    order = np.lexsort((-np.arange(n), -d[:, 4].astype(np.float64)))       # score descending, then index descending
    x1, y1, x2, y2 = (d[order, q] for q in range(4))
    area = ((x2 - x1) + F32(1)) * ((y2 - y1) + F32(1))
    dead = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(int(order[i]))
        j = np.arange(i + 1, n)
        w = np.maximum(F32(0), (np.minimum(x2[i], x2[j]) - np.maximum(x1[i], x1[j])) + F32(1))
        h = np.maximum(F32(0), (np.minimum(y2[i], y2[j]) - np.maximum(y1[i], y1[j])) + F32(1))
        inter = (w * h).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = (inter / ((area[i] + area[j]) - inter)).astype(F32)
        dead[j] |= ovr.astype(np.float64) >= thresh
    return np.asarray(keep, np.int64)


def image_ranges(rois, N):
    idx = np.asarray(rois)[:, 0].astype(np.int64)
    off = np.searchsorted(idx, np.arange(N + 1), side="left")
    return off


def select(rois, loss, N, thresh, per_image):
    """(sel: the chosen global rows image by image, n_sel [N], keep: every image's full keep list as global rows)."""
    rois = np.ascontiguousarray(rois, F32).reshape(-1, 5)
    loss = np.ascontiguousarray(loss, F32)
    off = image_ranges(rois, N)
    sel, n_sel, keeps = [], [], []
    for i in range(N):
        a, b = int(off[i]), int(off[i + 1])
        k = nms(np.hstack((rois[a:b, 1:5], loss[a:b, None])), thresh) + a
        keeps.append(k.astype(np.int32))
        sel.append(k[:per_image].astype(np.int32))
        n_sel.append(min(per_image, k.size))
    return (np.concatenate(sel) if sel else np.zeros(0, np.int32)), np.asarray(n_sel, np.int32), keeps


def keep_array(keeps, off, R):
    """The keep lists laid out as az_det_solver_fetch("mine_keep") lays them out: image i's from its first row, -1 behind."""
    out = np.full(R, -1, np.int32)
    for i, k in enumerate(keeps):
        out[off[i]:off[i] + k.size] = k
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------
def pool_blobs(seed, counts, ncls, H=D.MAP_H, W=D.MAP_W, dup=0):
    """A pool of sum(counts) rows over len(counts) images (counts[i] rows name image i, possibly none): rois inside H x W
    cells, labels (0, 1 and ncls - 1 among them where there is room), compact targets [R, 4].  dup: that many rows repeat
    the row before them exactly."""
    rng = np.random.Generator(np.random.PCG64(seed))
    R = int(sum(counts))
    x1 = rng.uniform(0, 16 * W - 40, R)
    y1 = rng.uniform(0, 16 * H - 40, R)
    x2 = np.minimum(x1 + rng.uniform(20, 16 * W * 0.7, R), 16 * W - 1)
    y2 = np.minimum(y1 + rng.uniform(20, 16 * H * 0.7, R), 16 * H - 1)
    idx = np.repeat(np.arange(len(counts)), counts).astype(np.float64)
    rois = np.stack([idx, x1, y1, x2, y2], 1).astype(F32)
    labels = np.where(rng.random(R) < 0.3, rng.integers(1, ncls, R), 0).astype(F32)
    for r, v in zip(range(R), (ncls - 1, 0, 1)):
        labels[r] = v
    targets = (rng.standard_normal((R, 4)) * 1.5).astype(F32)
    for r in rng.choice(np.arange(1, R), size=min(dup, max(R - 1, 0)), replace=False) if R > 1 and dup else []:
        if rois[r, 0] == rois[r - 1, 0]:
            rois[r], labels[r], targets[r] = rois[r - 1], labels[r - 1], targets[r - 1]
    return {"rois": rois, "labels": labels, "targets": targets}


def synth_head(seed, ncls, C=8, n6=36, n7=28):
    return D.filler_head(seed, C, n6, n7, ncls)


def synth_map(seed, C, N=2):
    from aznet_hip import synth
    return np.concatenate([synth.make_feature_map(seed + i, C, D.MAP_H, D.MAP_W) for i in range(N)], axis=0)


def forward64(head, fmap, rois, dtype=np.float64):
    """(cls_score, bbox_pred) of the TEST-phase forward from the map on, in `dtype`."""
    pool, _ = D.roi_pool(fmap, rois)
    r = D.step(head, pool, {"labels": np.zeros(pool.shape[0]), "bbox_targets": np.zeros((pool.shape[0], head["bb"].size)),
                            "bbox_loss_weights": np.zeros((pool.shape[0], head["bb"].size))}, None, dtype=dtype, want_dpool=False)
    return r["cls_score"], r["bbox_pred"]


# ---- the planted case: two images, 340 and 200 candidate rows, gaps between an image's row losses far above rounding --------
PLANT = dict(seed=61, ncls=21, counts=(340, 200), thresh=0.7, per_image=64, factor=100.0)


def planted_case():
    """(head, fmap, blobs, info): rows are drawn, their losses computed in float64 and float32 from the map on, and a row
    whose float64 or float32 loss lies within factor * bound * max loss of an earlier kept row of its image is discarded (in
    the restatement alone), so no rounding within the 8x rule can reorder two rows.  info: gap, the smallest gap left, the bound."""
    P = PLANT
    head = synth_head(P["seed"], P["ncls"])
    fmap = synth_map(P["seed"], head["W6"].shape[1] // 49)
    blobs = pool_blobs(P["seed"] + 1, P["counts"], P["ncls"])
    s64, b64 = forward64(head, fmap, blobs["rois"])
    s32, b32 = forward64(head, fmap, blobs["rois"], np.float32)
    l64 = row_losses(s64, b64, blobs["labels"], blobs["targets"])[0]
    l32 = row_losses(s32, b32, blobs["labels"], blobs["targets"], np.float32)[0]
    b = bound(rel_err(l32, l64))
    gap = P["factor"] * b * float(np.abs(l64).max())
    keep = []
    for i in range(len(P["counts"])):
        rows = np.flatnonzero(blobs["rois"][:, 0] == i)
        taken = []
        for r in rows[np.argsort(l64[rows], kind="stable")]:
            if not taken or (l64[r] - l64[taken[-1]] >= gap and float(l32[r]) - float(l32[taken[-1]]) >= gap):
                taken.append(r)
        keep.extend(sorted(taken))
    keep = np.asarray(keep, np.int64)
    blobs = {k: np.ascontiguousarray(v[keep]) for k, v in blobs.items()}
    l64, l32 = l64[keep], l32[keep]
    small = min(float(np.diff(np.sort(l64[blobs["rois"][:, 0] == i])).min()) for i in range(len(P["counts"])))
    return head, fmap, blobs, dict(gap=gap, smallest=small, bound=b, loss64=l64, loss32=l32)
