"""Case builders of tests/test_gpu_det_edges.py and its host twin tests/test_det_edges_host.py (test infrastructure): the
detection trainer (csrc/az_det_solver.hip) and the box-target kernels (csrc/az_det_train.hip) at their edges.  Softmax rows
whose columns reach every lane group of k_solver_softmax_loss, the size contract's upper edge (256 classes, 4096 rows),
hyper-parameters other than az_det_solver_create's, and example / object sets that the target kernels have not met (images
without example boxes, ties, degenerate boxes, classes with one row or identical rows, more than 256 classes).  NumPy only,
seeded, no GPU; the references are tests/det_step_ref.py and tests/det_train_ref.py."""
import functools

import numpy as np

import det_step_ref as D
import det_train_ref as DR

f32 = np.float32


def _f32(v):
    """What the trainer holds of a multiplier or ratio: its float32."""
    return float(np.float32(v))


# ---- 1. softmax-with-loss at lane-group and wave edges ---------------------------------------------------------------------
# a lane serves the columns lane, lane + 64, lane + 128, lane + 192: lane group q holds the columns [64 q, 64 q + 64)
SM_DIMS = dict(C=4, n6=8, n7=8)
SM_NCLS = (2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
SM_K = (1, 2, 4)
SM_ROWS = (1, 2, 4, 8)
HOT, COLD = np.float32(3.5), np.float32(-200.0)


def lane_groups(ncls):
    return (ncls + 63) // 64


def hot_columns(ncls, k):
    """The k columns at 3.5.  k = 1: the last column (the highest lane group alone holds the row's mass); k = 2: the two
    columns either side of the highest lane-group boundary; k = 4: one column in every lane group the ncls has, on the
    boundaries (0, 63 | 64, ncls - 1 up to three groups; 0, 127 | 128, ncls - 1 for four), filled up with the lowest free
    columns where those coincide."""
    G = lane_groups(ncls)
    if k == 1:
        cols = [ncls - 1]
    elif k == 2:
        cols = [64 * (G - 1) - 1, 64 * (G - 1)] if G > 1 else [0, ncls - 1]
    else:
        cols = sorted(set({1: [0, ncls - 1], 2: [0, 63, 64, ncls - 1], 3: [0, 63, 64, ncls - 1], 4: [0, 127, 128, ncls - 1]}[G]))
        c = 1
        while len(cols) < k:
            if c not in cols:
                cols.append(c)
            c += 1
    assert len(set(cols)) == k and min(cols) >= 0 and max(cols) < ncls
    return sorted(cols)


def exact_cases():
    return [(ncls, k) for ncls in SM_NCLS for k in SM_K if k <= ncls]


def softmax_map(rows):
    """(fmap [1, 4, 6, 8], rois [rows, 5]): what the rows pool does not matter, cls_score's weights are zero."""
    fmap = np.abs(np.random.RandomState(3).standard_normal((1, 4, 6, 8))).astype(np.float32) + 0.5
    return fmap, np.array([[0, 0, 0, 127, 95]] * rows, np.float32)


def exact_case(ncls, k):
    """(bias [ncls], labels [R], p [R, ncls], d [R, ncls]) of one exact row repeated R times: the bias is -200 but for k
    columns at 3.5, so e = exp(x - max) is 1 or exp(-203.5) = 0, p = 1 / k or 0, and with R a power of two
    d = (p - onehot) / R without a rounding.  The labels walk over a 3.5 column (the highest), a -200 column (the highest:
    p = 0, the FLT_MIN clamp), column 0 and column ncls - 1, starting where the case's index says."""
    i = exact_cases().index((ncls, k))
    R = SM_ROWS[i % 4]
    hot = hot_columns(ncls, k)
    bias = np.full(ncls, COLD, np.float32)
    bias[hot] = HOT
    cold = [c for c in range(ncls) if c not in hot]
    cand = [hot[-1]] + ([cold[-1]] if cold else []) + [0, ncls - 1]
    labels = np.array([cand[(r + i // 4) % len(cand)] for r in range(R)], np.float32)
    p = np.zeros((R, ncls), np.float32)
    p[:, hot] = np.float32(1) / np.float32(k)
    d = p.copy()
    d[np.arange(R), labels.astype(np.int64)] -= np.float32(1)
    d = d * (np.float32(1) / np.float32(R))
    return bias, labels, p, d.astype(np.float32)


SMR_NCLS = (65, 129, 193, 256)
SMR_ROWS = (1, 2, 3, 4, 5, 7, 9, 255, 256, 257)          # at 1, 2 and 3 rows some of the four waves have no row
SMR_SPAN = 30.0
SMR_MAP = (2, 4, D.MAP_H, D.MAP_W)


def random_rows_map():
    return np.abs(np.random.Generator(np.random.PCG64(77)).standard_normal(SMR_MAP)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _random_rows_pool(rows):
    """The rois of random_blobs(1000 + rows, ...) do not depend on ncls (they are drawn first): one pooling per row count."""
    rois = D.random_blobs(1000 + rows, rows, 2, D.MAP_H, D.MAP_W, 2)["rois"]
    return D.roi_pool(random_rows_map(), rois)[0]


@functools.lru_cache(maxsize=None)
def random_case(ncls, rows):
    """(head, fmap, blobs, pool5, seed): filler_head with Wc scaled so that the float64 logits span +-30 (bias aside);
    re-seeded until the float32 restatement's ReLU gates equal float64's (and fc7 is alive)."""
    pool = _random_rows_pool(rows)
    blobs = D.random_blobs(1000 + rows, rows, 2, D.MAP_H, D.MAP_W, ncls)
    for seed in range(200, 240):
        head = D.filler_head(seed, SM_DIMS["C"], SM_DIMS["n6"], SM_DIMS["n7"], ncls)
        r64 = D.step(head, pool, blobs, None, want_dpool=False)
        span = float(np.abs(r64["a7"] @ head["Wc"].T.astype(np.float64)).max())
        if span == 0.0:
            continue
        head["Wc"] = (head["Wc"] * (SMR_SPAN / span)).astype(np.float32)
        r32 = D.step(head, pool, blobs, None, dtype=np.float32, want_dpool=False)
        if all(D.gate_mismatch(r32["pre%d" % t], r64["pre%d" % t]) == 0.0 for t, _, _ in D.LAYERS):
            return head, random_rows_map(), blobs, pool, seed
    raise AssertionError("no seed gives equal gates")


# ---- 2. the size contract's upper edge -------------------------------------------------------------------------------------
SIZE = dict(C=4, n6=8, n7=8, ncls=256, R=4096)           # bbox_pred's unsplit forward product: 4096 x 1024 = part_elems


@functools.lru_cache(maxsize=None)
def size_case():
    """(head, fmap, blobs, pool5): integer weights (-1 .. 1), biases (-3 .. 3) and a 2 x 4 x 12 x 16 map of 0 .. 2, the rois
    of random_blobs: every partial sum is an integer (tests/test_gpu_det_train.py::test_integer_heads_bit_for_bit)."""
    rng = np.random.Generator(np.random.PCG64(41))
    C, n6, n7, ncls, n = (SIZE[k] for k in ("C", "n6", "n7", "ncls", "R"))
    ints = lambda shape, lo, hi: rng.integers(lo, hi + 1, shape).astype(np.float32)
    head = {"W6": ints((n6, C * 49), -1, 1), "b6": ints(n6, -3, 3), "W7": ints((n7, n6), -1, 1), "b7": ints(n7, -3, 3),
            "Wc": ints((ncls, n7), -1, 1), "bc": ints(ncls, -3, 3), "Wb": ints((4 * ncls, n7), -1, 1), "bb": ints(4 * ncls, -3, 3)}
    fmap = ints((2, C, D.MAP_H, D.MAP_W), 0, 2)
    blobs = D.random_blobs(9, n, 2, D.MAP_H, D.MAP_W, ncls)
    return head, fmap, blobs, D.roi_pool(fmap, blobs["rois"])[0]


def partial_sum_bounds(head, pool, r):
    """[(layer, the largest possible |partial sum| = max over rows and units of sum |a| |w| + |b|)] of the four products."""
    out, x = [], pool.astype(np.float64)
    for nm, wk, bk, nxt in (("fc6", "W6", "b6", "a6"), ("fc7", "W7", "b7", "a7"), ("cls_score", "Wc", "bc", None), ("bbox_pred", "Wb", "bb", None)):
        out.append((nm, float((np.abs(x) @ np.abs(head[wk]).T.astype(np.float64) + np.abs(head[bk])).max())))
        if nxt is not None:
            x = r[nxt]
    return out


# ---- 3. hyper-parameters off the defaults ------------------------------------------------------------------------------------
RATIO_SETS = ((0.3, 0.0), (0.0, 0.6), (0.25, 0.9), (0.8, 0.5))
HYPER_HEADS = ("voc", "coco")                             # R = 37 and R = 130
FRONT_DOOR = dict(ratios=(0.3, 0.0), steps=3)


def f32_scale(ratio):
    """The kernel's dropout scale: 1.0f / (1.0f - ratio) in float32."""
    return np.float32(1) / (np.float32(1) - np.float32(ratio))


def hyper_multipliers():
    """(lr_mult, decay_mult) by parameter name: fc7 frozen (lr_mult 0 / 0; its decay_mult stays 1 / 0), cls_score's weights
    at 0.1, bbox_pred's bias at 3; decay on fc6's bias, none on bbox_pred's weights.  As the float32 values the trainer
    multiplies with."""
    lr = dict(D.LR_MULT, W7=0.0, b7=0.0, Wc=_f32(0.1), bb=3.0)
    dc = dict(D.DECAY_MULT, b6=1.0, Wb=0.0)
    return lr, dc


def front_door_multipliers():
    return dict(D.LR_MULT, W7=0.0, b7=0.0), dict(D.DECAY_MULT)


def front_door_rows(rows):
    """prototxt.det_layer_table's rows with dropout 0.3 on fc6, no Dropout block on fc7 and fc7 frozen."""
    out = []
    for name, typ, lw, lb, dw, db, std, drop in rows:
        if name == "fc6":
            drop = 0.3
        elif name == "fc7":
            lw, lb, drop = 0.0, 0.0, None
        out.append((name, typ, lw, lb, dw, db, std, drop))
    return out


# ---- 5. target kernels on hostile sets -----------------------------------------------------------------------------------------
EX_COUNTS = (0, 3, 0, 0, 255, 1, 257, 0)                  # offsets 0 0 3 3 3 258 259 516 516: rows 256 and 512 start a block
GT_COUNTS = (2, 0, 1, 3, 70, 1, 5, 0)
TARGET_SETTINGS = {"a": dict(bbox_thresh=0.25, bg_lo=0.0, eps=0.0),
                   "b": dict(bbox_thresh=0.25, bg_lo=0.0, eps=1e-14),
                   "c": dict(bbox_thresh=0.7, bg_lo=0.3, eps=1e-14)}
TIE_BOX, TIE_OBJECT = (0., 0., 9., 9.), (0., 0., 19., 19.)               # IoU 100 / 400
NINE_DOWN = float(np.nextafter(np.float32(9), np.float32(0)))
TWIN_OBJECT, TWIN_AT, TWIN_CLASSES = (300., 320., 420., 470.), 10, (5, 9, 4)


def _jitter(rng, box, n, amount):
    box = np.asarray(box, np.float64)
    bw, bh = box[2] - box[0], box[3] - box[1]
    out = box[None, :] + rng.uniform(-amount, amount, (n, 4)) * np.array([bw, bh, bw, bh])
    out = np.maximum(out, 0)
    return np.stack([np.minimum(out[:, 0], out[:, 2]), np.minimum(out[:, 1], out[:, 3]),
                     np.maximum(out[:, 0], out[:, 2]), np.maximum(out[:, 1], out[:, 3])], 1)


def _objects(rng, n, lo, hi):
    x, y = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    return np.floor(np.stack([x, y, x + rng.uniform(30, 200, n), y + rng.uniform(30, 200, n)], 1))


@functools.lru_cache(maxsize=None)
def offsets_case():
    """(ex, gt, labels): per image the example boxes f32 [E, 4], the objects f32 [G, 4] and their classes (int64).  Image 4
    holds the geometry: [0,0,9,9] in [0,0,19,19] (IoU exactly 0.25), the float32 boxes next to that tie on either side,
    three identical objects of classes 5, 9, 4 at rows 10 .. 12, objects and boxes under one pixel wide or high, and
    coordinates near 1e4."""
    rng = np.random.Generator(np.random.PCG64(22))
    ex, gt, lab = [None] * 8, [None] * 8, [None] * 8
    none = np.zeros((0, 4))
    # image 4
    g4 = np.vstack([[TIE_OBJECT], _objects(rng, 9, 40, 900), [TWIN_OBJECT] * 3,
                    [[500.0, 50.0, 500.9, 300.0], [600., 100., 730., 100.5]],
                    [[9800., 9700., 9990., 9980.], [9000.5, 9100.25, 9999.75, 9900.5], [9990., 9990., 9999., 9999.5]],
                    _objects(rng, 52, 1000, 5000)])
    l4 = np.concatenate([[2], rng.integers(1, 21, 9), TWIN_CLASSES, [3, 7], [6, 8, 6], rng.integers(1, 21, 52)])
    nine_up = float(np.nextafter(np.float32(9), np.float32(10)))
    special = np.array([TIE_BOX, [0., 0., 9., NINE_DOWN], [0., 0., nine_up, 9.], TWIN_OBJECT,
                        [500.2, 50., 500.6, 300.], [500.0, 60., 500.5, 290.], [500.3, 50., 500.8, 250.],
                        [600., 100.1, 720., 100.4], [610., 100., 730., 100.3], [605., 100.2, 725., 100.5],
                        [9801.5, 9699.25, 9988., 9981.], [9010.5, 9110.25, 9989.75, 9890.5], [9990., 9990.5, 9999., 9999.25],
                        [9990.25, 9990., 9990.75, 9999.5]])
    e4 = np.vstack([special, _jitter(rng, TWIN_OBJECT, 12, 0.15)] + [_jitter(rng, b, 3, 0.25) for b in g4[1:10]]
                   + [_jitter(rng, b, 2, 0.3) for b in g4[18:70]])
    e4 = np.vstack([e4, _objects(rng, 255 - e4.shape[0], 30, 6000)])
    ex[4], gt[4], lab[4] = e4, g4, l4
    # image 6: 257 boxes round five objects
    g6 = _objects(rng, 5, 10, 400)
    ex[6] = np.vstack([_jitter(rng, b, 40, 0.35) for b in g6] + [_objects(rng, 57, 0, 500)])
    gt[6], lab[6] = g6, np.array([1, 20, 20, 13, 2])
    # images 0, 2, 3: objects but no example box; 1: boxes but no object; 5: one of each; 7: nothing
    for i, n in ((0, 2), (2, 1), (3, 3)):
        ex[i], gt[i], lab[i] = none, _objects(rng, n, 10, 300), rng.integers(1, 21, n)
    ex[1], gt[1], lab[1] = _objects(rng, 3, 0, 300), none, np.zeros(0)
    gt[5], lab[5] = _objects(rng, 1, 50, 200), np.array([11])
    ex[5] = _jitter(rng, gt[5][0], 1, 0.1)
    ex[7], gt[7], lab[7] = none, none, np.zeros(0)
    ex = [np.asarray(e, np.float64).reshape(-1, 4).astype(np.float32) for e in ex]
    gt = [np.asarray(g, np.float64).reshape(-1, 4).astype(np.float32) for g in gt]
    lab = [np.asarray(l).astype(np.int64) for l in lab]
    assert tuple(e.shape[0] for e in ex) == EX_COUNTS and tuple(g.shape[0] for g in gt) == GT_COUNTS
    return ex, gt, lab


def offsets_of(arrays):
    return np.concatenate([[0], np.cumsum([a.shape[0] for a in arrays])]).astype(np.int32)


def reference_targets(setting):
    """The yardstick on every image of offsets_case: [(targets f32 [E, 5], max_overlaps f64 [E])]."""
    ex, gt, lab = offsets_case()
    c = DR.DetCfg(**TARGET_SETTINGS[setting])
    out = []
    for e, g, l in zip(ex, gt, lab):
        t, mo = DR.compute_targets(e, g, l, c)
        out.append((t, mo.astype(np.float64)))
    return out


STATS_NCLS = (2, 21, 81, 257, 300)
STATS_IMAGES = {2: 3, 21: 5, 81: 6, 257: 8, 300: 16}      # 16 x 300 cells: 19 blocks of k_det_stats_image; 2 of k_det_stats_set
DYADIC = (0.5, -0.25, 0.125, 1.0)
STAT_CLASS = dict(spread=1, one_row=2, four_same=3, two_and_two=4, one_image=5, no_row=6, one_dyadic=7, four_dyadic=8)


@functools.lru_cache(maxsize=None)
def _stats_case(ncls):
    rng = np.random.Generator(np.random.PCG64(500 + ncls))
    n = STATS_IMAGES[ncls]
    rows = [[] for _ in range(n)]
    live = [i for i in range(n) if i != n - 2]            # image n - 2 has no row at all
    rand4 = lambda: np.concatenate([0.3 * rng.standard_normal(2), 0.5 * rng.standard_normal(2)]).astype(np.float32)
    put = lambda im, label, v: rows[im].append([label] + [float(x) for x in v])
    S = STAT_CLASS
    for im in live:                                       # a class spread over every image
        for _ in range(3 + im % 4):
            put(im, S["spread"], rand4())
    if ncls > 8:
        put(live[0], S["one_row"], rand4())               # one row: the std is 0, tiny or nan
        v = rand4()
        for _ in range(4):                                # four identical rows in one image
            put(live[1], S["four_same"], v)
        v = rand4()
        for im in (live[0], live[0], live[-1], live[-1]):  # and two and two in the first and the last image
            put(im, S["two_and_two"], v)
        for _ in range(10):                               # ten distinct rows, all in one image
            put(live[1], S["one_image"], rand4())
        put(live[-1], S["one_dyadic"], DYADIC)            # squares and sums without a rounding: a tiny positive variance
        for _ in range(4):
            put(live[0], S["four_dyadic"], DYADIC)
        for c in range(9, ncls):
            for _ in range(int(rng.choice([0, 1, 1, 2, 3, 5, 20]))):
                put(int(rng.choice(live)), c, rand4())
    for im in live:                                       # background rows, as the target kernel leaves them
        for _ in range(5):
            put(im, 0, np.zeros(4))
    for im, label in ((live[0], ncls), (live[-1], ncls + 5), (live[0], 1000.0), (live[1], 2.5), (live[1], -1.0)):
        put(im, label, rand4())                           # labels no kernel may count
    out = []
    for r in rows:
        a = np.array(r, np.float32).reshape(-1, 5)
        out.append(np.ascontiguousarray(a[rng.permutation(a.shape[0])]))
    return out


def stats_case(ncls):
    """Per image the un-normalised targets f32 [E, 5] (fresh copies): see STAT_CLASS for what the classes 1 .. 8 hold; the
    classes from 9 on have 0, 1, 2, 3, 5 or 20 random rows anywhere; every image but one also has background rows and
    rows whose label is ncls, ncls + 5, 1000, 2.5 or -1."""
    return [t.copy() for t in _stats_case(ncls)]


def reference_stats(ncls, eps=DR.EPS):
    """(counts, means, stds, normalised targets stacked) of the yardstick."""
    ts = stats_case(ncls)
    counts, means, stds = DR.target_stats(ts, ncls, DR.DetCfg(eps=eps), True)
    return counts, means, stds, np.vstack(ts)


def same_or_both_nan(got, want):
    """Bit for bit wherever `want` is no nan; nan where it is (a nan's sign and payload are not compared)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))
