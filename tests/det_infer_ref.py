"""References and case tables for detection inference at its edges (test infrastructure, plain NumPy / float64; the
yardstick of tests/test_det_infer_host.py and tests/test_gpu_det_infer_edges.py).

  A. az_detect       decode() restates _bbox_pred + _clip_boxes (lib/detect/test.py:106-151) in the reference's operation
                     order, detect_ref() the whole _frcnn_forward (:259-318) around a head given as a function of the unique
                     rows.  Two heads make the result exact: bias_head (all weights zero: every roi's deltas are `bb`, its
                     logits `bc`) and the integer head of head_sizes_ref.int_det_case with bbox_pred scaled by 2^-k.
  B. the pyramid     pyramid_ref.rois_blob / chunked are the reference's own formula; here only the scale sets and the boxes
                     around every switch point 2 * 224^2 / (s_a^2 + s_b^2).
  C. NMS             nms_walk(): the greedy walk of lib/utils/nms.pyx:17-68 in float32 NumPy in the documented tie order
                     (equal scores: the higher original index first); reference_keep(): the oracle's C walk in that order.
  D. image blob      the shapes and scales of the front-end cases (the reference is oracle.image_blob).
"""
import numpy as np

import pyramid_ref as pr

# (height, width, test scale): at scale 16 a roi's 1/16 cell is its rounded box, so the anchors of the small image stay apart
IMAGES = ((375, 500, 1.6), (16, 16, 16.0))
MAP_HW = (38, 63)                       # conv5_3 of a 600 x 1000 blob: the largest map any case uses
BIAS_DIMS = dict(C=4, n6=8, n7=8)
EPS = (0.0, 1e-14, 1.0)
CLASS_COUNTS = (2, 21, 63, 64, 65, 81, 128, 129, 255, 256)
BATCHES = (1, 7, 64, 10000)
CAP = 64                                # max_regions of the capacity context


# ---- A. az_detect ---------------------------------------------------------------------------------------------------------
def bias_head(ncls, bb, bc=None, dims=BIAS_DIMS):
    """A detection head whose weights are all zero: every slab sum is zeros plus the bias."""
    C, n6, n7 = dims["C"], dims["n6"], dims["n7"]
    bb = np.asarray(bb, np.float32).reshape(4 * ncls)
    bc = np.full(ncls, 0.5, np.float32) if bc is None else np.asarray(bc, np.float32).reshape(ncls)
    return {"W6": np.zeros((n6, C * 49), np.float32), "b6": np.zeros(n6, np.float32),
            "W7": np.zeros((n7, n6), np.float32), "b7": np.zeros(n7, np.float32),
            "Wc": np.zeros((ncls, n7), np.float32), "bc": bc, "Wb": np.zeros((4 * ncls, n7), np.float32), "bb": bb}


def decode(anchors, deltas, im_hw, eps):
    """_bbox_pred then _clip_boxes: anchors [R,4] f64, deltas [R,4K] f32 -> (clipped [R,4K] f64, unclipped [R,4K] f64).
    One rounding per operation, np.exp in the deltas' float32."""
    a = np.asarray(anchors, np.float64).reshape(-1, 4)
    d = np.asarray(deltas, np.float32).reshape(a.shape[0], -1)
    widths = a[:, 2] - a[:, 0] + eps
    heights = a[:, 3] - a[:, 1] + eps
    ctr_x = a[:, 0] + 0.5 * widths
    ctr_y = a[:, 1] + 0.5 * heights
    pcx = d[:, 0::4] * widths[:, None] + ctr_x[:, None]
    pcy = d[:, 1::4] * heights[:, None] + ctr_y[:, None]
    pw = np.exp(d[:, 2::4]) * widths[:, None]
    ph = np.exp(d[:, 3::4]) * heights[:, None]
    raw = np.zeros(d.shape)
    raw[:, 0::4] = pcx - 0.5 * pw
    raw[:, 1::4] = pcy - 0.5 * ph
    raw[:, 2::4] = pcx + 0.5 * pw
    raw[:, 3::4] = pcy + 0.5 * ph
    out = raw.copy()
    out[:, 0::4] = np.maximum(out[:, 0::4], 0)
    out[:, 1::4] = np.maximum(out[:, 1::4], 0)
    out[:, 2::4] = np.minimum(out[:, 2::4], im_hw[1] - 1)
    out[:, 3::4] = np.minimum(out[:, 3::4], im_hw[0] - 1)
    return out, raw


def unique_rows(boxes, scales, dedup, batch):
    """(rois [P,5] f32, index [U], inverse [P]) in the device entries' numbering; cfg.DEDUP_BOXES <= 0 skips the dedup
    (test.py:281 `if cfg.DEDUP_BOXES > 0:`): identity."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    scales = np.atleast_1d(np.asarray(scales, np.float64))
    if dedup > 0:
        return pr.chunked(boxes, scales, dedup, batch)
    ident = np.arange(boxes.shape[0], dtype=np.int64)
    rois = pr.rois_blob(boxes, scales) if len(boxes) else np.zeros((0, 5), np.float32)
    return rois, ident, ident.copy()


def detect_ref(boxes, scales, dedup, batch, im_hw, eps, head):
    """_frcnn_forward: head(index, rois_u) -> (probabilities [U,K], deltas [U,4K]) of the unique rows.  Returns scores
    [P,K], boxes [P,4K] f64 and a dict with index / inverse and the unclipped boxes of every input row."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    rois, index, inv = unique_rows(boxes, scales, dedup, batch)
    prob_u, delta_u = head(index, rois[index])
    clipped, raw = decode(boxes[index], delta_u, im_hw, eps)
    return np.asarray(prob_u)[inv], clipped[inv], {"index": index, "inv": inv, "raw": raw[inv], "rois": rois}


def bias_rows(head):
    """The head function of a bias-only head: every unique row gets softmax(bc) in Caffe's float32 and bb."""
    bc = head["bc"].astype(np.float32)
    e = np.exp(bc - bc.max())
    s = np.float32(0)
    for v in e:                                             # channel order, float32
        s = np.float32(s + v)
    p = (e / s).astype(np.float32)
    return lambda index, rois_u: (np.tile(p, (len(index), 1)), np.tile(head["bb"].astype(np.float32), (len(index), 1)))


# the classes of the clip head: (dx, dy) in anchor widths / heights, dw = dh = 0 -> expf is exactly 1
CLIP_SHIFTS = ((0, 0), (-0.75, 0), (0.75, 0), (0, -0.75), (0, 0.75), (-8, 0), (8, 0), (0, -8), (0, 8), (-0.75, -0.75),
               (0.75, 0.75), (-0.5, 0), (0.5, 0), (0, -0.5), (0, 0.5), (0.25, -0.125))


def clip_head():
    bb = np.zeros((len(CLIP_SHIFTS), 4), np.float32)
    bb[:, :2] = CLIP_SHIFTS
    return bias_head(len(CLIP_SHIFTS), bb)


def clip_anchors(H, W):
    """Anchors whose decoded classes hit every clip edge of an H x W image (the host twin asserts which)."""
    xm, ym = W - 1.0, H - 1.0
    return np.array([
        [xm / 4, ym / 4, 3 * xm / 4, 3 * ym / 4],          # centred, half the image: each shift of 0.75 clips one side alone
        [0, 0, xm, ym],                                     # the image itself: sides exactly on 0 and W-1 / H-1 at eps 0
        [0, 0, xm / 2, ym / 2],                             # a shift of -0.5 / +0.5 lands a side exactly on 0 / the middle
        [xm / 2, ym / 2, xm, ym],                           # ... and exactly on W-1 / H-1
        [-10, -7, W + 12, H + 9],                           # larger than the image: all four clips
        [-30, -20, -5, -3],                                 # negative coordinates, wholly outside
        [W + 5, H + 3, W + 40, H + 30],                     # wholly past the image
        [W / 2.0, H / 3.0, W / 2.0, H / 3.0 + 5],           # x2 == x1: width = eps
        [1, 1, 2, 2],
        [W / 3.0 + 0.3, H / 5.0 + 0.7, W / 1.5 + 0.1, H / 1.25 + 0.9],
    ], dtype=np.float64)


def class_head(ncls, log_sizes=False):
    """Distinct deltas per class: dx = (c - ncls/2) / 64, dy = ((3c + 1) % 257 - 128) / 128 (exact in float32; dw = dh = 0
    unless log_sizes), and distinct logits in steps of 1/4."""
    c = np.arange(ncls)
    bb = np.zeros((ncls, 4), np.float32)
    bb[:, 0] = (c - ncls // 2) / 64.0
    bb[:, 1] = ((3 * c + 1) % 257 - 128) / 128.0
    if log_sizes:
        bb[:, 2] = (c % 7 - 3) / 16.0
        bb[:, 3] = (c % 5 - 2) / 16.0
    bc = ((c * 37) % 11 - 5) * 0.25
    return bias_head(ncls, bb, bc)


def class_anchors(H, W):
    return np.array([[W / 4.0, H / 4.0, 3 * W / 4.0, 3 * H / 4.0], [2, 3, W / 2.0, H / 2.0], [W / 2.0, 1, W - 2.0, H - 3.0]])


def chunk_sizes(batch, cap=CAP):
    return sorted({p for p in (1, batch - 1, batch, batch + 1, 2 * batch, cap) if 1 <= p <= cap})


def chunk_boxes(P, H, W, scale):
    """P boxes over five distinct 1/16 cells: row i repeats row i - 5 exactly, row i - 10 moved by a fraction of its cell
    (merged, but with its own anchor) -- the same box lies in one chunk and in two, whatever the chunk size."""
    cell = 16.0 / scale
    base = np.array([[1, 1, 6, 5], [2, 1, 7, 6], [1, 2, 5, 7], [3, 3, 8, 8], [0, 2, 6, 6]], np.float64) * cell
    i = np.arange(P)
    b = base[i % 5].copy()
    b[(i // 5) % 2 == 1] += 0.2 * cell * np.array([0.5, -0.25, 0.25, 0.125])
    return np.minimum(b, [W - 1.0, H - 1.0, W - 1.0, H - 1.0])


def overflow_boxes():
    """dedup = 1: coordinates >= 1000 and < 0, so a hash field runs into the next one.  Rows 0 / 1 collide although the
    boxes differ (x1 = 1000, y1 = 0 against x1 = 0, y1 = 1), as do rows 6 / 7 (x1 = -1000, y1 = 1 against x1 = 0, y1 = 0);
    rows 2 / 3 and 4 / 5 are ordinary duplicates, the rest are distinct with negative keys among them."""
    return np.array([[1000, 0, 1500, 1200], [0, 1, 1500, 1200], [-3, -2, 1001, 2000], [-3, -2, 1001, 2000],
                     [1999.4, 5, 2500.4, 1000.5], [1999, 5, 2500, 1000], [-1000, 1, 10, 10], [0, 0, 10, 10],
                     [-1, -1, -1, -1], [-2000, -1500, -1001, -1000.5], [999, 999, 999, 999], [-0.5, 0.5, 1.5, 2.5]],
                    dtype=np.float64)


def int_case(orc=None):
    """The integer-exact detection head (12, 132, 100, 21) on its 300 rois with bbox_pred times 2^-k, k the smallest with
    max |delta| <= 1: the deltas vary per roi and are exact multiples of 2^-k.  `zero_sizes`: the same head with the dw / dh
    rows of bbox_pred zeroed (expf exactly 1: the decode is exact)."""
    import head_sizes_ref as hs
    pool = (lambda f, r: orc.roi_pool(f[0], r)) if orc is not None else None
    case = hs.int_det_case((12, 132, 100, 21), pool=pool)
    k = int(np.ceil(np.log2(max(float(np.abs(case["bbox"]).max()), 1.0))))
    unit = np.float32(2.0 ** -k)
    head = dict(case["head"])
    head["Wb"], head["bb"] = head["Wb"] * unit, head["bb"] * unit
    deltas = (case["bbox"].astype(np.float64) * float(unit)).astype(np.float32)
    zhead = dict(head)
    zhead["Wb"], zhead["bb"] = head["Wb"].copy(), head["bb"].copy()
    rows = np.arange(head["bb"].size) % 4 >= 2
    zhead["Wb"][rows] = 0
    zhead["bb"][rows] = 0
    zdeltas = deltas.copy()
    zdeltas[:, rows] = 0
    return {"k": k, "head": head, "zero_sizes": zhead, "deltas": deltas, "zero_deltas": zdeltas, "fmap": case["fmap"],
            "boxes": case["rois"][:, 1:5].astype(np.float64), "p64": case["p64"]["cls"],
            "p32": hs.softmax32(case["pre"]["cls"].astype(np.float32)), "im": (hs.IM_H, hs.IM_W)}


# ---- B. the pyramid -------------------------------------------------------------------------------------------------------
SCALE_SETS = {
    "three": [1.28, 1.536, 1.835],
    "two": [1.0, 2.0],
    "eight": [float(v) for v in np.geomspace(0.5, 4.0, 8)],
    "descending": [1.835, 1.536, 1.28],
    "unsorted": [1.536, 2.2, 0.9, 1.28],
    "tie": [1.28, 1.6, 1.6, 2.0],
    "all_equal": [1.6, 1.6, 1.6],
}


def switch_points(scales):
    """The f64 area at which levels a and b (distinct scales) are equally far from 224^2, for every pair a < b."""
    s = np.asarray(scales, np.float64)
    return [(a, b, 2.0 * 224.0 * 224.0 / (s[a] * s[a] + s[b] * s[b])) for a in range(len(s)) for b in range(a + 1, len(s))
            if s[a] != s[b]]


def switch_boxes(scales, ulps=4):
    """For every switch point A: boxes of height 1 and width within `ulps` units in the last place of A, A itself included
    (x1 = 0, x2 = w - 1: w - 1 and w share a binade, so x2 - x1 + 1 gives w back exactly)."""
    rows = []
    for a, b, A in switch_points(scales):
        w = A
        for _ in range(ulps):
            w = np.nextafter(w, -np.inf)
        for _ in range(2 * ulps + 1):
            rows.append([0.0, 0.0, w - 1.0, 0.0])
            w = np.nextafter(w, np.inf)
    return np.array(rows, np.float64).reshape(-1, 4)


def spread_boxes(n=200, seed=3):
    """Boxes of every size from 8 to 1400 pixels a side (every level of every scale set is some box's)."""
    rng = np.random.RandomState(seed)
    side = np.exp(rng.uniform(np.log(8), np.log(1400), n))
    x1, y1 = rng.uniform(-20, 400, n), rng.uniform(-20, 300, n)
    return np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.5, 2, n)], 1)


def degenerate_boxes():
    """Negative areas (x2 < x1 - 1), an infinite area and NaN areas (0 * inf, a NaN coordinate)."""
    big = 1e200
    return np.array([[50, 10, 10, 200], [300, 300, 100, 100], [10, 200, 400, 20], [-big, -big, big, big],
                     [5, -1.5e308, 4, 1.5e308], [np.nan, 0, 10, 10], [0, 0, 10, np.nan]], dtype=np.float64)


def merge_pair(scales=(1.0, 2.0)):
    """Two boxes on different levels with identical projected coordinates: [0,0,199,199] at scale 1 and half of it at 2."""
    return np.array([[0, 0, 199, 199], [0, 0, 99.5, 99.5], [40, 20, 239, 219], [20, 10, 119.5, 109.5]], np.float64)


# ---- C. NMS ---------------------------------------------------------------------------------------------------------------
NMS_SMALL = 256
NMS_MAPPED_MAX = 16384                  # az_nms_batched polls host-mapped memory up to this many boxes in a call


def nms_case(rng, n, kind):
    """The five adversarial kinds of tests/test_gpu_nms_fuzz.py at a given size, finite scores."""
    if n == 0:
        return np.zeros((0, 5), np.float32)
    if kind == 0:
        x1 = rng.uniform(0, 900, n); y1 = rng.uniform(0, 500, n); w = rng.uniform(10, 210, n); h = rng.uniform(10, 210, n)
    elif kind == 1:
        k = max(1, n // 50); cx = rng.uniform(0, 900, k); cy = rng.uniform(0, 500, k); a = rng.randint(k, size=n)
        x1 = cx[a] + rng.normal(0, 6, n); y1 = cy[a] + rng.normal(0, 6, n); w = 80 + rng.normal(0, 5, n); h = 60 + rng.normal(0, 5, n)
    elif kind == 2:
        m = max(1, n // 4); bx = rng.uniform(0, 900, m); by = rng.uniform(0, 500, m); a = rng.randint(m, size=n)
        x1 = bx[a]; y1 = by[a]; w = np.full(n, 50.0); h = np.full(n, 40.0)
    elif kind == 3:
        x1 = rng.randint(0, 40, n) * 8.0; y1 = rng.randint(0, 30, n) * 8.0
        w = rng.randint(1, 6, n) * 8.0 - 1; h = rng.randint(1, 6, n) * 8.0 - 1
    else:
        x1 = rng.uniform(0, 900, n); y1 = rng.uniform(0, 500, n); w = rng.uniform(-20, 100, n); h = rng.uniform(-20, 100, n)
    sc = rng.permutation(n) / float(n) if rng.rand() < 0.5 else np.round(rng.uniform(0, 1, n) * 16) / 16.0
    return np.stack([x1, y1, x1 + w, y1 + h, sc], 1).astype(np.float32)


def nms_none_suppressed(n=NMS_SMALL, ties=True):
    """n disjoint boxes: all kept (count n: 256 fills the count's nine bits)."""
    i = np.arange(n)
    x1, y1 = (i % 16) * 40.0, (i // 16) * 30.0
    sc = np.round((i * 7 % 16)) / 16.0 if ties else (i * 37 % n) / float(n)
    return np.stack([x1, y1, x1 + 19, y1 + 14, sc], 1).astype(np.float32)


def nms_all_but_first(n=NMS_SMALL):
    """n copies of one box with distinct scores: only the best survives."""
    i = np.arange(n)
    return np.stack([np.full(n, 10.0), np.full(n, 20.0), np.full(n, 90.0), np.full(n, 70.0), (i * 101 % n) / float(n)],
                    1).astype(np.float32)


def nms_groups(sizes, seed):
    """One group per size: the kinds in turn; a size written as ('none', n) / ('first', n) is the matching special group."""
    rng = np.random.RandomState(seed)
    out = []
    for g, n in enumerate(sizes):
        if isinstance(n, tuple):
            out.append(nms_none_suppressed(n[1]) if n[0] == "none" else nms_all_but_first(n[1]))
        else:
            out.append(nms_case(rng, int(n), g % 5))
    return out


EDGE_SIZES = [0, 0, 1, 2, 257, 63, 64, 0, 65, 128, 300, 255, 256, ("none", 256), ("first", 256), 0]
NMS_TABLE = {
    # name: (sizes, seed)
    "edges": (EDGE_SIZES, 11),
    "all_empty": ([0, 0, 0], 12),
    "one_empty": ([0], 13),
    "many_small": (list(np.random.RandomState(14).randint(1, 9, 2000)), 14),
    "largest_mapped": ([256] * 63 + [("none", 256)], 15),                   # 16384 boxes: the last host-mapped total
    "one_more": ([256] * 63 + [("first", 256), 1], 16),                      # 16385: the first copied-back one
    "copy_back": ([256, ("none", 256), ("first", 256), 255, 0, 257, 256] * 12 + [0, 1, 300, 2], 17),
}


def nms_total(sizes):
    return int(sum(n[1] if isinstance(n, tuple) else n for n in sizes))


def nms_walk(dets, thresh):
    """nms.pyx:17-68 in float32 NumPy; equal scores in the documented order (the higher original index first)."""
    d = np.ascontiguousarray(dets, np.float32).reshape(-1, 5)
    n = d.shape[0]
    one = np.float32(1)
    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    areas = ((x2 - x1) + one) * ((y2 - y1) + one)
    order = np.lexsort((np.arange(n), d[:, 4]))[::-1]
    alive = np.ones(n, bool)
    keep = []
    for pos, i in enumerate(order):
        if not alive[i]:
            continue
        keep.append(int(i))
        rest = order[pos + 1:]
        rest = rest[alive[rest]]
        w = np.maximum(np.float32(0), (np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest])) + one)
        h = np.maximum(np.float32(0), (np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest])) + one)
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / ((areas[i] + areas[rest]) - inter)
        alive[rest[ovr.astype(np.float64) >= thresh]] = False
    return keep


def reference_keep(orc, dets, thresh):
    """The oracle's C walk (orc_nms) given the documented order of ties, as tests/test_gpu_nms_fuzz.py builds it."""
    dets = np.ascontiguousarray(dets, np.float32).reshape(-1, 5)
    n = dets.shape[0]
    if n == 0:
        return []
    order = np.ascontiguousarray(np.lexsort((np.arange(n), dets[:, 4]))[::-1], dtype=np.int64)
    keep = np.zeros(n, dtype=np.int64)
    nk = orc.lib().orc_nms(orc._fp(dets), n, orc._lp(order), float(thresh), orc._lp(keep))
    return [int(k) for k in keep[:nk]]


# ---- D. the image front-end ---------------------------------------------------------------------------------------------
MEANS = np.array([102.9801, 115.9465, 122.7717], np.float32)
# (h, w, scale, what it is for)
BLOB_CASES = (
    (5, 255, 1.0, "ow 255"), (5, 256, 1.0, "ow 256: the grid edge"), (5, 257, 1.0, "ow 257"),
    (3, 128, 2.0, "ow 256 by scale 2"), (4, 1024, 0.5, "ow 512 by scale 0.5"), (3, 171, 3.0, "ow 513 by scale 3"),
    (6, 1026, 0.5, "ow 513 by scale 0.5"), (1, 40, 1.7, "h 1"), (40, 1, 1.7, "w 1"), (1, 1, 3.0, "one pixel"),
    (3, 50, 0.4, "oh 1"), (50, 3, 0.4, "ow 1"), (5, 9, 0.5, "2.5 -> 2 and 4.5 -> 4: ties to even, down"),
    (7, 11, 0.5, "3.5 -> 4 and 5.5 -> 6: ties to even, up"), (37, 53, 1.0, "scale 1"), (24, 36, 0.5, "scale 0.5"),
    (19, 23, 2.0, "scale 2"), (13, 17, 3.0, "scale 3"), (61, 83, 0.3, "non-dyadic down"), (47, 59, 1.0 / 1.7, "non-dyadic down"),
)


def blob_image(h, w, kind, seed=0):
    if kind == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "full":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) % 2) * 255).astype(np.uint8)[:, :, None], 3, 2)
    return np.random.RandomState(seed + 131 * h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
