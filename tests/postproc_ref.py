"""NumPy restatement of Soft-NMS and box voting as include/aznet_hip.h defines them (az_soft_nms_batched,
az_box_vote_batched), operation for operation, and the seeded cases the host and the GPU tests share.

IoU is az_nms's float32 arithmetic: every NumPy operation on float32 arrays rounds once, as the library (built without
contraction) does.  soft_nms_ref runs in float32 (the device's bits for methods hard and linear; for gaussian np.exp is not
expf, so that method is held to float64 by the 8x rule) or in float64 (the same steps on the float32 inputs widened).
box_vote_ref keeps the float32 IoU and sums in float64 in ascending row order."""
from fractions import Fraction

import numpy as np

METHODS = ("hard", "linear", "gaussian")


def _areas(b, one):
    return ((b[:, 2] - b[:, 0]) + one) * ((b[:, 3] - b[:, 1]) + one)


def iou_row(b, area, k):
    """IoU of box k with every box of b [n, 4] (dtype = b's), one rounding per operation."""
    one, zero = b.dtype.type(1), b.dtype.type(0)
    xx1 = np.maximum(b[k, 0], b[:, 0])
    yy1 = np.maximum(b[k, 1], b[:, 1])
    xx2 = np.minimum(b[k, 2], b[:, 2])
    yy2 = np.minimum(b[k, 3], b[:, 3])
    w = np.maximum(zero, (xx2 - xx1) + one)
    h = np.maximum(zero, (yy2 - yy1) + one)
    inter = w * h
    den = (area[k] + area) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / den


def soft_nms_ref(dets, method, thresh, sigma=0.5, min_score=0.001, dtype=np.float32, info=None):
    """(keep int64 [nk], scores dtype [nk]).  info (a dict): receives 'gap', the smallest relative gap between a picked score
    and the runner-up of its round, and 'margin', the smallest relative distance of a decayed score from min_score."""
    assert method in METHODS
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    n = dets.shape[0]
    b = dets[:, :4].astype(dtype)
    s = dets[:, 4].astype(dtype)
    area = _areas(b, dtype(1))
    sig = dtype(np.float32(sigma))
    alive = np.ones(n, bool)
    keep, out = [], []
    gap, margin = np.inf, np.inf
    for _ in range(n):
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        cur = s[idx]
        m = cur.max()
        k = int(idx[cur == m].max())                     # equal scores: the higher original index
        if info is not None and idx.size > 1 and m > 0:
            second = np.max(np.where(idx == k, -np.inf, cur))
            gap = min(gap, float((m - second) / m))
        keep.append(k)
        out.append(s[k])
        alive[k] = False
        ovr = iou_row(b, area, k)
        if method == "gaussian":
            with np.errstate(invalid="ignore"):
                w = np.exp(-(ovr * ovr) / sig)
        else:
            over = ovr.astype(np.float64) >= thresh
            w = np.where(over, (dtype(1) - ovr) if method == "linear" else dtype(0), dtype(1)).astype(dtype)
        with np.errstate(invalid="ignore"):
            s = np.where(alive, s * w, s).astype(dtype)
        if info is not None and min_score > 0 and alive.any():
            margin = min(margin, float(np.min(np.abs(s[alive].astype(np.float64) - min_score)) / min_score))
        alive &= ~(s.astype(np.float64) < min_score)
    if info is not None:
        info["gap"], info["margin"] = gap, margin
    return np.asarray(keep, np.int64), np.asarray(out, dtype)


def box_vote_ref(dets, keep, vote_thresh, loop=None):
    """[nk, 4] float32.  loop=True: the definition as written, a Python loop over the rows in ascending order; False: the same
    sums through np.cumsum, which adds in that order too (large groups); None: the loop up to 20000 pairs."""
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    keep = np.asarray(keep, np.int64).ravel()
    n = dets.shape[0]
    b = dets[:, :4]
    area = _areas(b, np.float32(1))
    if loop is None:
        loop = n * keep.size <= 20000
    out = np.zeros((keep.size, 4), np.float32)
    b64, s64 = b.astype(np.float64), dets[:, 4].astype(np.float64)
    for r, k in enumerate(keep):
        votes = iou_row(b, area, int(k)).astype(np.float64) >= vote_thresh
        if loop:
            sw, sc = 0.0, [0.0, 0.0, 0.0, 0.0]
            for j in range(n):
                if votes[j]:
                    sj = float(dets[j, 4])
                    sw += sj
                    for q in range(4):
                        sc[q] += sj * float(dets[j, q])
            sc = np.asarray(sc)
        else:
            j = np.flatnonzero(votes)
            sw = float(np.cumsum(s64[j])[-1]) if j.size else 0.0
            sc = np.cumsum(s64[j, None] * b64[j], axis=0)[-1] if j.size else np.zeros(4)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[r] = b[k] if sw == 0 else (sc / sw).astype(np.float32)
    return out


def box_vote_exact(dets, keep, vote_thresh):
    """The voted boxes as exact rationals rounded once to float64 and then to float32 -- for cases whose sums the device
    holds exactly (whole-number coordinates, power-of-two scores)."""
    dets = np.asarray(dets, np.float32).reshape(-1, 5)
    b = dets[:, :4]
    area = _areas(b, np.float32(1))
    out = np.zeros((len(keep), 4), np.float32)
    for r, k in enumerate(keep):
        votes = np.flatnonzero(iou_row(b, area, int(k)).astype(np.float64) >= vote_thresh)
        sw = sum(Fraction(float(dets[j, 4])) for j in votes)
        for q in range(4):
            out[r, q] = b[k, q] if sw == 0 else np.float32(float(sum(Fraction(float(dets[j, 4])) * Fraction(float(b[j, q])) for j in votes) / sw))
    return out


def postprocess_ref(all_boxes, method, thresh, sigma, min_score, vote, vote_thresh):
    """detect.test.postprocess_detections group by group, through the restatement."""
    out = [[[] for _ in cls] for cls in all_boxes]
    for c, cls in enumerate(all_boxes):
        for i, d in enumerate(cls):
            if isinstance(d, list) and d == []:
                continue
            d = np.asarray(d, np.float32).reshape(-1, 5)
            keep, sc = soft_nms_ref(d, method, thresh, sigma, min_score if method != "hard" else hard_min_score(d))
            if keep.size == 0:
                continue
            boxes = box_vote_ref(d, keep, vote_thresh) if vote else d[keep, :4]
            out[c][i] = np.hstack((boxes, sc[:, None])).astype(np.float32)
    return out


def hard_min_score(dets):
    """A min_score at which method hard is az_nms: the smallest positive score (tiny when there is none)."""
    s = np.asarray(dets, np.float32).reshape(-1, 5)[:, 4]
    return float(s[s > 0].min()) if np.any(s > 0) else float(np.finfo(np.float32).tiny)


# ---- case generators -------------------------------------------------------------------------------------------------------
def random_group(seed, n, span=300.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    x1, y1 = rng.uniform(0, span, n), rng.uniform(0, span, n)
    b = np.stack([x1, y1, x1 + rng.uniform(5, span / 2, n), y1 + rng.uniform(5, span / 2, n)], 1)
    return np.hstack((b, rng.uniform(0.01, 1.0, (n, 1)))).astype(np.float32)


def clustered_group(seed, n, clusters=None, span=400.0, jitter=8.0):
    """n boxes around a few objects: what a detector hands to NMS (many overlaps inside a cluster)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nc = clusters or max(1, n // 12)
    cx, cy = rng.uniform(0, span, nc), rng.uniform(0, span, nc)
    cw, ch = rng.uniform(30, 150, nc), rng.uniform(30, 150, nc)
    a = rng.integers(0, nc, n)
    x1 = cx[a] + rng.normal(0, jitter, n)
    y1 = cy[a] + rng.normal(0, jitter, n)
    x2 = x1 + cw[a] * rng.uniform(0.8, 1.25, n)
    y2 = y1 + ch[a] * rng.uniform(0.8, 1.25, n)
    return np.stack([x1, y1, x2, y2, rng.uniform(0.01, 1.0, n)], 1).astype(np.float32)


def with_duplicates(d, seed):
    """Every third row repeats an earlier one, box and score."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = d.copy()
    for i in range(2, d.shape[0], 3):
        d[i] = d[rng.integers(0, i)]
    return d


def equal_scores(d, value=0.5):
    d = d.copy()
    d[:, 4] = value
    return d


def whole_number_group(seed, n):
    """Whole-number coordinates below 2^10 and power-of-two scores: every float64 sum of box voting is exact."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x1, y1 = rng.integers(0, 200, n), rng.integers(0, 200, n)
    b = np.stack([x1, y1, x1 + rng.integers(20, 120, n), y1 + rng.integers(20, 120, n)], 1).astype(np.float64)
    s = 2.0 ** -rng.integers(0, 8, n).astype(np.float64)
    return np.hstack((b, s[:, None])).astype(np.float32)


# Gaussian Soft-NMS is compared with the float64 restatement in order and count, which holds only where no decision is close:
# the seeds below were searched on the CPU (gaussian_seed) for a relative gap of at least GAP between every picked score and
# its runner-up and a relative distance of at least GAP between every decayed score and min_score, in float64;
# tests/test_postproc_host.py asserts both and that the float32 restatement then picks the same boxes in the same order.
GAP = 1e-4
GAUSS = dict(thresh=0.3, sigma=0.5, min_score=0.001)
GAUSS_SIZES = (2, 30, 45, 65, 80, 100, 257)
GAUSS_SEEDS = {2: 0, 30: 0, 45: 0, 65: 0, 80: 1, 100: 1, 257: 0}      # gaussian_seed(n) for n in GAUSS_SIZES


def gaussian_ok(d):
    info = {}
    k64, _ = soft_nms_ref(d, "gaussian", dtype=np.float64, info=info, **GAUSS)
    k32, _ = soft_nms_ref(d, "gaussian", dtype=np.float32, **GAUSS)
    return info["gap"] >= GAP and info["margin"] >= GAP and np.array_equal(k64, k32), info


def gaussian_seed(n, limit=4000):
    for seed in range(limit):
        if gaussian_ok(clustered_group(1000 * n + seed, n))[0]:
            return seed
    raise AssertionError("no seed below %d gives a gap of %g at %d boxes" % (limit, GAP, n))


def gaussian_case(n):
    return clustered_group(1000 * n + GAUSS_SEEDS[n], n)


def front_door_boxes():
    """all_boxes[class][image] of 3 classes x 4 images (class 0: the background, empty lists): clustered detections with
    planted near-duplicates (a row shifted by a pixel at a lower score), one empty group and one single box."""
    all_boxes = [[[] for _ in range(4)] for _ in range(3)]
    for c in (1, 2):
        for i in range(4):
            n = (0, 1, 37, 90)[(c + i) % 4]
            d = clustered_group(50 + 10 * c + i, n, clusters=3)
            for r in range(1, n, 4):
                d[r, :4] = d[r - 1, :4] + np.float32(1.0)
                d[r, 4] = d[r - 1, 4] * np.float32(0.9)
            all_boxes[c][i] = d
    return all_boxes
