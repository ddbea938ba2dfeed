"""Plain references and seeded cases for the three small integer / compare stages every proposal passes through: decode +
filter (az_decode_filter), top-k (az_topk / az_topk_radix) and the threshold selection of a search.  NumPy only, float64
and exact integers; nothing here imports the library under test.  tests/test_select_edges_host.py checks on the CPU that
the references reproduce the g4 / g8 goldens and the oracle's decode and that every generator meets the conditions it
states; tests/test_gpu_select_edges.py runs the kernels on the same cases.

Restrictions of the generators: no NaN and no -0.0 (the search's scores are softmax outputs, neither occurs).  Under that
restriction the order of the score's bit key (score_key: sign-flipped bits, ascending with the value) is the order of the
value, so topk_ref equals np.argsort(-s.astype(np.float64), kind="stable")[:min(k, n)] -- the host test asserts it on every
generated pattern."""
import numpy as np

NSUB = 11                 # candidates per region
TOPK_MAX = 4096           # az_topk refuses a larger k
RANK_MAX_N = 65536        # the counting kernels take n <= this, the radix select everything above
DEFAULT_MAX_REGIONS = 16384
DEFAULT_MAX_CANDIDATES = DEFAULT_MAX_REGIONS * NSUB
BLOCK = 256               # candidates per workgroup of the flag / compaction kernels
RADIX_THREADS = 1024      # threads of the single-workgroup select: its ordered gather gives thread t [t*per, (t+1)*per)


# ------------------------------------------------------------------------------------------------------ references
def score_key(scores):
    """The order-preserving uint32 key of a float32 (ascending with the value; -0.0 sorts below +0.0)."""
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def topk_ref(scores, k):
    """Indices of the min(k, n) largest keys, descending; equal keys: lower index first."""
    key = score_key(scores).astype(np.int64)
    return np.argsort(-key, kind="stable")[:min(int(k), key.shape[0])]


def thresh_ref(scores, Tc):
    return np.where(np.asarray(scores).astype(np.float64) >= Tc)[0]


def decode_raw(anchors, deltas, eps):
    """_bbox_pred (lib/detect/test.py:106-139) in float64, np.exp taken on the float32 deltas and then widened: the
    unclipped boxes [R*11, 4] in r*11+s order."""
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 4)
    R = a.shape[0]
    d = np.asarray(deltas, dtype=np.float32).reshape(R, NSUB, 4)
    w = (a[:, 2] - a[:, 0] + eps)[:, None]
    h = (a[:, 3] - a[:, 1] + eps)[:, None]
    cx = a[:, 0][:, None] + 0.5 * w
    cy = a[:, 1][:, None] + 0.5 * h
    pcx = d[:, :, 0].astype(np.float64) * w + cx
    pcy = d[:, :, 1].astype(np.float64) * h + cy
    pw = np.exp(d[:, :, 2]).astype(np.float64) * w
    ph = np.exp(d[:, :, 3]).astype(np.float64) * h
    return np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], axis=2).reshape(R * NSUB, 4)


def decode_clipped(anchors, deltas, im_h, im_w, eps):
    b = decode_raw(anchors, deltas, eps)
    b[:, 0] = np.maximum(b[:, 0], 0.0)
    b[:, 1] = np.maximum(b[:, 1], 0.0)
    b[:, 2] = np.minimum(b[:, 2], im_w - 1.0)
    b[:, 3] = np.minimum(b[:, 3], im_h - 1.0)
    return b


def sides(boxes):
    return np.minimum(boxes[:, 3] - boxes[:, 1] + 1, boxes[:, 2] - boxes[:, 0] + 1)


def decode_filter_ref(anchors, deltas, scores, im_h, im_w, eps, min_side):
    """_bbox_pred + _clip_boxes + _unwrap_adj_pred (lib/detect/test.py:171-187): the kept boxes and scores in r*11+s order,
    and per candidate (kept or not) the margin min(w, h) + 1 - min_side; a candidate is kept iff its side >= min_side."""
    b = decode_clipped(anchors, deltas, im_h, im_w, eps)
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    side = sides(b)
    keep = np.where(side >= min_side)[0]
    return b[keep], s[keep], side - min_side


# -------------------------------------------------------------------------------------------------- top-k cases
def topk_sizes(max_candidates=DEFAULT_MAX_CANDIDATES):
    return [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, RANK_MAX_N - 1, RANK_MAX_N,
            RANK_MAX_N + 1, RANK_MAX_N + 1025, max_candidates]


TOPK_KS = [1, 2, 300, 4095, 4096]
# the patterns every size gets, and the sizes every pattern gets (the tie-run pattern needs n > k: see tie_straddle)
SIZE_PATTERNS = ["uniform_ties", "all_equal", "ascending", "descending", "max_first", "max_last"]
PATTERN_SIZES = [257, 1025, 4097, 8193, RANK_MAX_N, RANK_MAX_N + 1025]
PATTERN_KS = [1, 300, 4096]


def _bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def _place(n, k, count_hi, rng, hi=0.75, lo=0.25):
    s = np.full(n, lo, dtype=np.float32)
    s[rng.permutation(n)[:count_hi]] = hi
    return s


def per_thread_chunk(n):
    return (n + RADIX_THREADS - 1) // RADIX_THREADS


def tie_straddle(n, k, rng=None):
    """A run of k + 1 equal scores that starts before and ends after a multiple b of the per-thread chunk, g scores
    above it (k >= 4: one in front of the run and one behind it, else none) and lower scores elsewhere: the k-th selected
    candidate is an element of the run, and for k >= 4 one behind b.  Needs n >= max(k + 3, 10).
    Returns (scores, run_start, run_end, b, g)."""
    k = min(k, TOPK_MAX)
    assert n >= max(k + 3, 10)
    per = per_thread_chunk(n)
    b = per * max(1, (n // 2) // per)
    g = 2 if k >= 4 else 0
    need = k - g                                    # elements of the run that are selected
    lo_start = 1 if g else 0
    front = max(1, min(need - 1, b - lo_start))     # elements of the run in front of b
    start = b - front
    end = start + k + 1
    assert lo_start <= start < b < end <= n - lo_start
    s = np.full(n, 0.25, dtype=np.float32)
    s[start:end] = 0.5
    if g:
        s[0] = 0.75
        s[n - 1] = 0.875
    return s, start, end, b, g


def topk_scores(pattern, n, k, seed):
    """One float32 score vector of a named pattern (no NaN, no -0.0)."""
    rng = np.random.RandomState(seed)
    kk = min(k, TOPK_MAX)
    if pattern == "uniform_ties":
        s = rng.uniform(0, 1, n).astype(np.float32)
        if n > 4:
            s[rng.randint(0, n, n // 4)] = s[rng.randint(0, n, n // 4)]
        return s
    if pattern == "all_equal":
        return np.full(n, 0.5, dtype=np.float32)
    if pattern == "two_values_cut_in_lower":        # fewer than k of the upper value: the k-th selected is a lower one
        return _place(n, kk, min(n, kk // 2), rng)
    if pattern == "two_values_cut_in_upper":        # more than k of the upper value: the k-th selected is an upper one
        return _place(n, kk, min(n, kk + max(1, (n - kk) // 2)), rng)
    if pattern == "low10":                          # only the third radix pass (key bits 0..9) tells the scores apart
        return _bits(np.uint32(0x3F000000) | rng.randint(0, 1 << 10, n).astype(np.uint32))
    if pattern == "mid11":                          # only the second pass (key bits 10..20)
        return _bits(np.uint32(0x3F000155) | (rng.randint(0, 1 << 11, n).astype(np.uint32) << np.uint32(10)))
    if pattern == "top11":                          # only the first pass (key bits 21..31); exponent < 255: finite
        return _bits(np.uint32(0x00000155) | (rng.randint(0, 0x3FC, n).astype(np.uint32) << np.uint32(21)))
    if pattern == "tie_straddle":
        return tie_straddle(n, kk, rng)[0]
    if pattern == "ascending":                      # consecutive bit patterns from 0.5 up: strictly ascending
        return _bits(np.uint32(0x3F000000) + np.arange(n, dtype=np.uint32))
    if pattern == "descending":
        return _bits(np.uint32(0x3F000000) + np.arange(n, dtype=np.uint32)[::-1])
    if pattern == "zero_one":                       # exact 0.0 and 1.0 among values between them
        s = rng.uniform(0, 1, n).astype(np.float32)
        c = rng.randint(0, 3, n)
        s[c == 0] = 0.0
        s[c == 1] = 1.0
        return s
    if pattern == "denormals":                      # positive denormals, some 0.0, a few normal values
        s = _bits(rng.randint(1, 1 << 23, n).astype(np.uint32))
        c = rng.randint(0, 8, n)
        s[c == 0] = 0.0
        s[c == 1] = np.float32(1.5e-38)
        s[c == 2] = s[0]
        return s
    if pattern == "negative_inf":                   # the key is defined for every float: negatives, +inf, -inf
        s = rng.standard_normal(n).astype(np.float32)
        s[s == 0] = 1.0
        c = rng.randint(0, 16, n)
        s[c == 0] = np.inf
        s[c == 1] = -np.inf
        s[c == 2] = np.float32(-1e-40)              # a negative denormal
        return s
    if pattern in ("max_first", "max_last"):        # one distinct maximum at either end
        s = (rng.uniform(0, 0.875, n)).astype(np.float32)
        s[0 if pattern == "max_first" else n - 1] = 1.0
        return s
    raise KeyError(pattern)


TOPK_PATTERNS = ["uniform_ties", "all_equal", "two_values_cut_in_lower", "two_values_cut_in_upper", "low10", "mid11", "top11",
                 "tie_straddle", "ascending", "descending", "zero_one", "denormals", "negative_inf", "max_first", "max_last"]
KEY_BIT_RANGES = {"low10": (0, 10), "mid11": (10, 21), "top11": (21, 32)}


def pattern_cases(pattern):
    """(n, k, seed) of one pattern: PATTERN_SIZES x PATTERN_KS (the tie run where n >= k + 3)."""
    out = []
    for i, n in enumerate(PATTERN_SIZES):
        for j, k in enumerate(PATTERN_KS):
            if pattern == "tie_straddle" and n < max(k + 3, 10):
                continue
            out.append((n, k, 1000 + 10 * i + j))
    return out


# ---------------------------------------------------------------------------------------------- decode + filter cases
IMAGES = [(600, 1000), (375, 500), (16, 16)]
MIN_SIDES = [1.0, 10.0, 16.5]
EPSS = [0.0, 1e-14, 1.0]
DECODE_ROWS = [0, 1, 23, 24, 93, 94, 1000, DEFAULT_MAX_REGIONS]
KEEP_PATTERNS = ["none", "all", "alternating", "block_last", "block_first", "first_only"]
MARGIN_BAND = 1e-3        # px: ten times the box tolerance's atol; keep / drop is asserted outside this band only
MARGIN_SHARE = 0.01       # at most this share of a random case may lie inside the band
BOX_RTOL, BOX_ATOL = 1e-6, 1e-4


def id_scores(n):
    """Candidate c carries the score c + 1 (exact in float32 below 2^24): the output names its survivors."""
    assert n < (1 << 24)
    return np.arange(1, n + 1, dtype=np.float32)


def survivors(scores_out):
    return np.asarray(scores_out).astype(np.int64) - 1


def _zero_deltas(R):
    return np.zeros((R, NSUB, 4), dtype=np.float32)


# the eleven centre shifts of an edge row, in units of the anchor's size (all exact in binary)
EDGE_SHIFTS = [(0, 0), (-0.25, 0), (0, -0.25), (0.25, 0), (0, 0.25), (-0.25, -0.25), (0.25, 0.25), (-4, 0), (4, 0), (0, -4),
               (0, 4)]


def clip_case(im_h, im_w, eps, min_side):
    """Log-size deltas 0: anchors at the four edges, the four corners, the centre and one larger than the image, each
    with the eleven EDGE_SHIFTS -- every clip alone, all four at once, and boxes pushed wholly outside the image."""
    W, H = float(im_w), float(im_h)
    sw, sh = np.floor(W / 4), np.floor(H / 4)                  # anchor extent (w = sw - 1 + eps)
    xs = [0.5, np.floor((W - sw) / 2), W - sw - 0.5]           # (half a pixel inside: a quarter-size shift crosses the edge)
    ys = [0.5, np.floor((H - sh) / 2), H - sh - 0.5]
    anchors = [[x, y, x + sw - 1, y + sh - 1] for y in ys for x in xs]
    anchors.append([-8.0, -8.0, W + 7, H + 7])                 # all four clips at once
    anchors.append([-8.0, 2.0, W + 7, H - 3])                  # x1 and x2 only
    anchors.append([2.0, -8.0, W - 3, H + 7])                  # y1 and y2 only
    anchors = np.array(anchors, dtype=np.float64)
    R = anchors.shape[0]
    d = _zero_deltas(R)
    for s, (dx, dy) in enumerate(EDGE_SHIFTS):
        d[:, s, 0] = dx
        d[:, s, 1] = dy
    return dict(anchors=anchors, deltas=d.reshape(R, 4 * NSUB), scores=id_scores(R * NSUB).reshape(R, NSUB), im_h=im_h, im_w=im_w,
                eps=eps, min_side=min_side)


def _sym_anchor(v, big, axis):
    """An anchor whose decoded box (deltas 0, eps 0) is exactly [-v, v] along `axis` and [-big, big] along the other:
    w = 2v, the centre 0, both halves exact."""
    return [-v, -big, v, big] if axis == 0 else [-big, -v, big, v]


def min_side_case(min_side, im_h=600, im_w=1000):
    """eps 0, deltas 0: per axis one candidate whose side equals min_side exactly (kept) and one whose side is the
    double below min_side (dropped), found by the reference among a handful of anchors (a row's eleven candidates are
    alike).  Returns the case, the indices of the equal candidates and those of the one-step-below candidates."""
    t = np.nextafter(np.float64(min_side), -np.inf)
    rows, eq, below = [], [], []
    for axis in (0, 1):
        found = {}
        cands = [min_side - 1.0, t - 1.0, np.nextafter(t - 1.0, -np.inf), np.nextafter(t - 1.0, np.inf), (t - 1.0) / 2.0,
                 (min_side - 1.0) / 2.0]
        for v in cands:
            a = np.array([_sym_anchor(v, 100.0, axis)], dtype=np.float64)
            side = sides(decode_clipped(a, _zero_deltas(1), im_h, im_w, 0.0))[0]
            if side == min_side and "eq" not in found:
                found["eq"] = a[0]
            if side == t and "below" not in found:
                found["below"] = a[0]
        assert "eq" in found and "below" in found, (min_side, axis, sorted(found))
        eq.append(len(rows) * NSUB + np.arange(NSUB))
        rows.append(found["eq"])
        below.append(len(rows) * NSUB + np.arange(NSUB))
        rows.append(found["below"])
    anchors = np.array(rows, dtype=np.float64)
    R = anchors.shape[0]
    case = dict(anchors=anchors, deltas=_zero_deltas(R).reshape(R, 4 * NSUB), scores=id_scores(R * NSUB).reshape(R, NSUB),
                im_h=im_h, im_w=im_w, eps=0.0, min_side=float(min_side))
    return case, np.concatenate(eq), np.concatenate(below)


def keep_flags(pattern, n):
    c = np.arange(n)
    if pattern == "none":
        return np.zeros(n, dtype=bool)
    if pattern == "all":
        return np.ones(n, dtype=bool)
    if pattern == "alternating":
        return (c & 1) == 0
    if pattern == "block_last":                     # the last candidate of every 256-candidate block (and of the tail)
        return ((c % BLOCK) == BLOCK - 1) | (c == n - 1)
    if pattern == "block_first":
        return (c % BLOCK) == 0
    if pattern == "first_only":
        return c == 0
    raise KeyError(pattern)


def rows_case(R, pattern, im_h, im_w, eps, min_side):
    """R regions whose candidates are kept or dropped after `pattern`: a kept candidate is its anchor (deltas 0, a box of
    side >= 17 inside the image), a dropped one the same box moved 128 widths to the right, out of every image."""
    n = R * NSUB
    r = np.arange(R, dtype=np.float64)
    size = 17.0 if min(im_h, im_w) > 40 else float(min(im_h, im_w))     # 16 x 16: the whole image (side 16 + eps)
    if size == 17.0:
        x = np.mod(r * 7.0, im_w - 20.0)
        y = np.mod(np.floor(r / 3.0), im_h - 20.0)
    else:
        x = np.zeros(R)
        y = np.zeros(R)
    anchors = np.stack([x, y, x + size - 1, y + size - 1], axis=1).reshape(R, 4)
    d = np.zeros((n, 4), dtype=np.float32)
    d[~keep_flags(pattern, n), 0] = 128.0
    return dict(anchors=anchors, deltas=d.reshape(R, 4 * NSUB), scores=id_scores(n).reshape(R, NSUB), im_h=im_h, im_w=im_w, eps=eps,
                min_side=min_side)


def rows_settings(i):
    """Image, eps and min_side of the i-th row-count case: the three lists walked at different strides (min_side 16.5
    never on the 16 x 16 image, where the kept boxes have side 16 + eps)."""
    im = IMAGES[i % 3]
    ms = MIN_SIDES[(i // 3 + i) % 3]
    if im == (16, 16) and ms > 16:
        ms = 10.0
    return im[0], im[1], EPSS[(i + 1) % 3], ms


RANDOM_CASES = [(300, 600, 1000, 1e-14, 10.0, 11), (257, 375, 500, 0.0, 16.5, 12), (120, 16, 16, 1.0, 1.0, 13),
                (1000, 600, 1000, 1.0, 10.0, 14)]


def random_case(R, im_h, im_w, eps, min_side, seed):
    """Anchors inside (and slightly around) the image, centre deltas in [-1, 1], log-size deltas in [-2, 2]."""
    rng = np.random.RandomState(seed)
    x1 = rng.uniform(-0.1 * im_w, 0.9 * im_w, R)
    y1 = rng.uniform(-0.1 * im_h, 0.9 * im_h, R)
    w = rng.uniform(2, 0.6 * im_w, R)
    h = rng.uniform(2, 0.6 * im_h, R)
    anchors = np.stack([x1, y1, x1 + w, y1 + h], axis=1)
    d = np.empty((R, NSUB, 4), dtype=np.float32)
    d[:, :, :2] = rng.uniform(-1, 1, (R, NSUB, 2))
    d[:, :, 2:] = rng.uniform(-2, 2, (R, NSUB, 2))
    return dict(anchors=anchors, deltas=d.reshape(R, 4 * NSUB), scores=id_scores(R * NSUB).reshape(R, NSUB), im_h=im_h, im_w=im_w,
                eps=eps, min_side=min_side)


def case_ref(case):
    return decode_filter_ref(case["anchors"], case["deltas"], case["scores"], case["im_h"], case["im_w"], case["eps"],
                             case["min_side"])
