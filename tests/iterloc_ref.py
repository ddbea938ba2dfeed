"""Iterative box localisation restated in NumPy, and the case tables of tests/test_iterloc_host.py and
tests/test_gpu_iterloc.py (test infrastructure).

iter_ref(detect_fn, boxes, rounds, min_score, max_rows) is the definition of az_detect_iter: detect_fn(boxes) is one
one-shot detection, (scores [P, K] f32, boxes [P, 4K] f64, ...).  With detect_fn = det_infer_ref.detect_ref on a bias-only
head every answer is known in closed form; with detect_fn = AzContext.detect it is the host loop a caller had to write
before the entry existed (download, select in NumPy, az_detect on the selected boxes, take the class column), which is the
yardstick of the device loop: a roi's bits do not depend on its batch, so the two are compared with array_equal."""
import numpy as np

import det_infer_ref as D

MAX_ROUNDS, MAX_ROWS = 8, 4096


def select(scores, min_score, max_rows):
    """The sources among `scores` (one per candidate, in ascending flat index f): score >= float32(min_score), and past
    max_rows of them the max_rows highest, ties to the lower f (az_topk's rule).  Returns their f, ascending."""
    s = np.asarray(scores, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        f = np.flatnonzero(s >= np.float32(min_score))
    if f.size > max_rows:
        order = np.argsort(-s[f], kind="stable")[:max_rows]       # stable: among equal scores the lower f first
        f = np.sort(f[order])
    return f


def iter_ref(detect_fn, boxes, rounds, min_score, max_rows):
    """Returns (scores, boxes, extra): round 1 as detect_fn gives it, extra = dict(cls, src, round, score, box, count) of the
    later rounds, round after round."""
    assert 1 <= rounds <= MAX_ROUNDS and 1 <= max_rows <= MAX_ROWS
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    out = detect_fn(boxes)
    scores, pred = np.asarray(out[0], np.float32), np.asarray(out[1], np.float64)
    P, K = scores.shape
    ex = dict(cls=[], src=[], round=[], score=[], box=[])
    count = np.zeros(rounds - 1, np.int32)
    # the candidates of round 2: (row i, class j >= 1) at f = (j - 1) * P + i
    c_score = scores[:, 1:].T.reshape(-1)
    c_box = pred.reshape(P, K, 4)[:, 1:].transpose(1, 0, 2).reshape(-1, 4)
    c_cls = np.repeat(np.arange(1, K, dtype=np.int32), P)
    c_src = np.tile(np.arange(P, dtype=np.int32), K - 1)
    for r in range(rounds - 1):
        f = select(c_score, min_score, max_rows) if P else np.zeros(0, np.int64)
        count[r] = f.size
        if f.size == 0:
            break
        cls, src = c_cls[f], c_src[f]
        o = detect_fn(c_box[f])
        s2, p2 = np.asarray(o[0], np.float32), np.asarray(o[1], np.float64)
        e = np.arange(f.size)
        c_score, c_box = s2[e, cls], p2.reshape(f.size, K, 4)[e, cls]      # from new row e only its own class's column
        c_cls, c_src = cls, e.astype(np.int32)                             # round t + 2 selects among these alone
        ex["cls"].append(cls); ex["src"].append(src); ex["score"].append(c_score); ex["box"].append(c_box)
        ex["round"].append(np.full(f.size, r + 2, np.int32))
    cat = lambda k, dt, shape: (np.concatenate(ex[k]).astype(dt) if ex[k] else np.zeros(shape, dt))      # noqa: E731
    extra = dict(cls=cat("cls", np.int32, 0), src=cat("src", np.int32, 0), round=cat("round", np.int32, 0),
                 score=cat("score", np.float32, 0), box=cat("box", np.float64, (0, 4)), count=count)
    return scores, pred, extra


def same(a, b):
    """Two (scores, boxes, extra) results, bit for bit; returns the first field that differs, or None."""
    if not (np.array_equal(a[0], b[0]) and a[0].dtype == b[0].dtype):
        return "scores"
    if not (np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype):
        return "boxes"
    for k in ("count", "cls", "src", "round", "score", "box"):
        x, y = np.asarray(a[2][k]), np.asarray(b[2][k])
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            return k
    return None


# ---- heads and boxes --------------------------------------------------------------------------------------------------------
IMAGE = (375, 500, 1.6)                    # height, width, test scale: det_infer_ref.IMAGES[0]


def shift_head(ncls, bc=None):
    """Bias-only head, class j moves a box by (j / 64 of its width, -j / 128 of its height), dw = dh = 0: with eps = 0 and
    a 64 x 32 box that is (j, -j / 4) pixels a round, exactly."""
    bb = np.zeros((ncls, 4), np.float32)
    bb[:, 0] = np.arange(ncls) / 64.0
    bb[:, 1] = -np.arange(ncls) / 128.0
    return D.bias_head(ncls, bb, bc)


def spread_boxes(P, H, W, seed=5):
    """P boxes inside an H x W image, distinct, a few cells wide (their refined boxes stay inside for a few rounds)."""
    rng = np.random.RandomState(seed)
    x1 = rng.randint(40, W - 140, P) + rng.randint(0, 4, P) * 0.25
    y1 = rng.randint(60, H - 120, P) + rng.randint(0, 4, P) * 0.25
    return np.stack([x1, y1, x1 + rng.randint(24, 90, P), y1 + rng.randint(24, 60, P)], 1).astype(np.float64)


def row_score_head(ncls, dims=D.BIAS_DIMS):
    """A head whose class scores differ from roi to roi (fc6 reads the pooled map, the rest passes it on): small random
    weights with distinct logits per class, deltas as class_head's.  Not exact in closed form: for the host loop only."""
    rng = np.random.RandomState(ncls)
    h = D.class_head(ncls)
    C, n6, n7 = dims["C"], dims["n6"], dims["n7"]
    h["W6"] = (rng.rand(n6, C * 49).astype(np.float32) - 0.25) / 32
    h["W7"] = (rng.rand(n7, n6).astype(np.float32) - 0.25) / 2
    h["Wc"] = (rng.rand(ncls, n7).astype(np.float32) - 0.5) * 2
    return h
