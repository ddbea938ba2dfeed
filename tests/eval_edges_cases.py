"""Inputs that put az_rank_unit / az_voc_eval / az_coco_eval / az_recall_match on the edges of their kernels' constants
(DESIGN, "Evaluation edges"), and the ranking's reference.  Shared by test_eval_edges_host.py, which checks that every
builder holds what its name promises, and test_gpu_eval_edges.py (not collected)."""
import numpy as np

import coco_cases

# the constants of az_voc.hip / az_coco.hip / az_eval.hip the sizes below derive from
AZ_WAVE, VT, VTILE, SCH, REG_CLAIMS, MAXDET, CT, RM_T = 64, 256, 2048, 1024, 2048, 100, 256, 256


# ---------------------------------------------------------------------------------------------------- ranking
def rank_ref(n_classes, n_images, score, det_off):
    """(by_seg, by_class) of rank_by_score as a chain of documented-stable sorts.  NumPy's sort puts NaN last and
    compares -0 == +0, as MATLAB's sort(-conf) and COCOeval's mergesort do."""
    score = np.asarray(score, np.float64)
    seg = np.repeat(np.arange(n_classes * n_images), np.diff(np.asarray(det_off, np.int64)))
    o = np.argsort(-score, kind="stable")
    by_seg = o[np.argsort(seg[o], kind="stable")]
    by_class = o[np.argsort((seg // n_images)[o], kind="stable")]
    return by_seg.astype(np.uint32), by_class.astype(np.uint32)


RANK_SIZES = [1, AZ_WAVE - 1, AZ_WAVE, AZ_WAVE + 1, VT - 1, VT, VT + 1, VTILE - 1, VTILE, VTILE + 1, 2 * VTILE,
              2 * VTILE + 1, 4 * VTILE, 4 * VTILE + 1, 5 * VTILE + 1]
RANK_PATTERNS = ["distinct", "quarters", "equal", "mixed_sign"]
# with D beyond this the [digit][tile] table has more than 1024 chunks of SCH counts: k_voc_scan's per > 1
RANK_BIG_D = 1024 * SCH // 256 * VTILE + VTILE + 1


def scores(pattern, D, seed=0):
    rng = np.random.RandomState(seed)
    if pattern == "distinct":
        return (rng.permutation(D) + 1.0) / (D + 1.0)
    if pattern == "quarters":
        return rng.randint(0, 5, D) / 4.0
    if pattern == "equal":
        return np.full(D, 0.5)
    if pattern == "mixed_sign":
        return np.round(rng.normal(0.0, 2.0, D), 1) * 10.0 ** rng.randint(-3, 4, D)
    raise ValueError(pattern)


def random_offsets(S, D, seed=0):
    rng = np.random.RandomState(seed)
    return np.concatenate([[0], np.sort(rng.randint(0, D + 1, S - 1)), [D]]).astype(np.int64)


def rank_size_case(D, pattern):
    """3 classes x 5 images, random segment sizes."""
    return 3, 5, scores(pattern, D, seed=D), random_offsets(15, D, seed=D + 1)


SCORE_BASE_BITS = 0x3FE5555555555555


def one_byte_scores(byte, D=3000, seed=0):
    """Scores equal in every byte but `byte` (0: lowest mantissa byte ... 7: sign and high exponent bits): only that
    key pass decides an order, the other seven must keep it.  All finite."""
    rng = np.random.RandomState(seed + byte)
    bits = np.uint64(SCORE_BASE_BITS) ^ (rng.randint(0, 256, D).astype(np.uint64) << np.uint64(8 * byte))
    return bits.view(np.float64)


def special_scores(D=3000, seed=0):
    """Quantised scores of both signs with +0, -0, +-inf, positive and negative denormals and NaNs (either sign bit,
    two payloads) sprinkled in, several of each."""
    rng = np.random.RandomState(seed)
    s = np.round(rng.normal(0.0, 1.0, D), 1)
    nan2 = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    vals = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.5e-310, -2.5e-310, np.nan, -np.nan, nan2]
    pos = rng.permutation(D)[:6 * len(vals)]
    s[pos] = np.tile(vals, 6)
    return s


# (n_classes, n_images, D)
RANK_LAYOUTS = [(1, 1, 3000), (1, 2, 3000), (2, 1, 3000), (1, 256, 3000), (1, 257, 3000), (256, 1, 3000), (257, 1, 3000),
                (3, 100, 3000), (300, 3, 3000), (65537, 1, 70000), (1, 65537, 70000)]


def rank_layout_case(C, N, D):
    return C, N, scores("quarters", D, seed=C + N), random_offsets(C * N, D, seed=C * 7 + N)


def rank_empty_segment_cases():
    """name -> (C, N, score, det_off): empty segments at the head, in the middle, at the tail; all in the last one."""
    C, N, D = 5, 8, 3000
    S = C * N
    out = {}
    for name, live in (("head", range(12, S)), ("middle", list(range(0, 9)) + list(range(27, S))), ("tail", range(0, 22)),
                       ("last_only", [S - 1])):
        live = list(live)
        cnt = np.zeros(S, np.int64)
        cnt[live] = np.random.RandomState(len(live)).multinomial(D, np.ones(len(live)) / len(live))
        out[name] = (C, N, scores("quarters", D, seed=len(live)), np.concatenate([[0], np.cumsum(cnt)]))
    return out


def rank_big_case():
    D = RANK_BIG_D
    rng = np.random.RandomState(84)
    return 3, 100, rng.randint(0, 1 << 20, D) / float(1 << 20), random_offsets(300, D, seed=85)


# ---------------------------------------------------------------------------------------------------- VOC
def voc_iou(b, g):
    """VOCevaldet's overlap of one detection with [k,4] boxes (1-based corners), -inf where they do not intersect."""
    g = np.asarray(g, np.float64).reshape(-1, 4)
    iw = np.minimum(b[2], g[:, 2]) - np.maximum(b[0], g[:, 0]) + 1
    ih = np.minimum(b[3], g[:, 3]) - np.maximum(b[1], g[:, 1]) + 1
    ua = (b[2] - b[0] + 1) * (b[3] - b[1] + 1) + (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1) - iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((iw > 0) & (ih > 0), iw * ih / ua, -np.inf)


def _grid_boxes(G):
    j = np.arange(G)
    x, y = 1.0 + 30.0 * (j % 100), 1.0 + 30.0 * (j // 100)
    return np.stack([x, y, x + 19.0, y + 19.0], 1)


# (first, duplicate) candidates: (3, 40) two lanes of one round; (0, 64) and (5, 69) j and j + 64, one lane;
# (60, 66) and (1, 128) a low j in a high lane, a higher j in a lower lane; (10, 127); (7, 2047) the last register bit;
# (100, 2048), (2040, 2050), (2046, 2111) register claim against HBM claim
VOC_TIE_PAIRS = [(3, 40), (0, 64), (5, 69), (60, 66), (10, 127), (1, 128), (7, 2047), (100, 2048), (2040, 2050),
                 (2046, 2111)]


def voc_tie_pairs(G):
    return [(a, b) for a, b in VOC_TIE_PAIRS if b < G]


def voc_gt_count_case(G, n):
    """One segment, G boxes on a grid, box b of every pair in voc_tie_pairs(G) an exact copy of box a and exactly one of
    the two difficult (so taking the wrong one changes the result).  The detections sit exactly on boxes, two per
    target: the first copies take ranks 0 .., the second copies follow -- a claimed box is met again, in a later chunk
    of 64 detections when n > 64.  Targets: every pair, the boxes next to the lane / register edges, the last box."""
    gb = _grid_boxes(G)
    gd = (np.arange(G) % 5 == 4).astype(np.uint8)
    pairs = voc_tie_pairs(G)
    for k, (a, b) in enumerate(pairs):
        gb[b] = gb[a]
        gd[a], gd[b] = (0, 1) if k % 2 == 0 else (1, 0)
    targets = [a for a, _ in pairs]
    for j in (G - 1, 62, 63, 64, 65, 2047, 2048, 2049, 2050, 2051, 2100, G // 2):
        if 0 <= j < G and j not in targets and all(j != b for _, b in pairs):
            targets.append(j)
    rng = np.random.RandomState(G * 1000 + n)
    rest = [j for j in rng.permutation(G).tolist() if j not in targets and all(j != b for _, b in pairs)]
    targets = (targets + rest)[:(n + 1) // 2]
    while len(targets) < (n + 1) // 2:                       # fewer boxes than n / 2: meet some a third, fourth time
        targets = targets + targets
    targets = targets[:(n + 1) // 2]
    order = targets + targets
    box = gb[order][:n].copy()
    if n % 2:
        box[-1] = [5000.0, 5000.0, 5010.0, 5010.0]           # the odd one out overlaps nothing
    conf = 1.0 - np.arange(n) / float(2 * n)
    return 1, 1, box, conf, np.array([0, n]), gb, gd, np.array([0, G])


VOC_G = [AZ_WAVE - 1, AZ_WAVE, AZ_WAVE + 1, 2 * AZ_WAVE, 2 * AZ_WAVE + 1, REG_CLAIMS - 1, REG_CLAIMS, REG_CLAIMS + 1,
         REG_CLAIMS + AZ_WAVE]
VOC_N = [64, 65, 129]


def voc_claim_across_chunks_case():
    """130 detections of one image: the one at rank 10 takes box 0, its copy at rank 70 (the second chunk of 64) finds it
    claimed; the rest overlap nothing."""
    n = 130
    gb = np.array([[1.0, 1.0, 20.0, 20.0], [101.0, 1.0, 120.0, 20.0], [201.0, 1.0, 220.0, 20.0]])
    box = np.stack([np.array([5000.0 + 30 * k, 5000.0, 5019.0 + 30 * k, 5019.0]) for k in range(n)])
    conf = 1.0 - np.arange(n) / 1000.0                       # file order = rank order
    box[10] = gb[0]
    box[70] = gb[0]
    box[100] = gb[2]
    return 1, 1, box, conf, np.array([0, n]), gb, np.zeros(3, np.uint8), np.array([0, 3])


VOC_MIN_OVERLAPS = [0.0, 0.3, 0.5, 0.7, 1.0]


def voc_min_overlap_case():
    """One box per image on an integer grid with a detection that covers 100, 70, 69, 50, 49, 30, 29 and 1 of its 100
    pixels and nothing else (ov = pixels / 100 exactly), one a column larger than its box (100 / 110), and one that
    overlaps nothing."""
    sq, bar = [1.0, 1.0, 10.0, 10.0], [1.0, 1.0, 100.0, 1.0]
    pairs = [(sq, sq), (sq, [1.0, 1.0, 10.0, 7.0]), (bar, [1.0, 1.0, 69.0, 1.0]), (sq, [1.0, 1.0, 10.0, 5.0]),
             (sq, [1.0, 1.0, 7.0, 7.0]), (sq, [1.0, 1.0, 10.0, 3.0]), (bar, [1.0, 1.0, 29.0, 1.0]), (sq, [1.0, 1.0, 1.0, 1.0]),
             (sq, [1.0, 1.0, 11.0, 10.0]), (sq, [50.0, 50.0, 60.0, 60.0])]
    N = len(pairs)
    conf = np.round(np.linspace(0.9, 0.1, N), 3)
    return (1, N, np.array([d for _, d in pairs]), conf, np.arange(N + 1), np.array([g for g, _ in pairs]),
            np.zeros(N, np.uint8), np.arange(N + 1))


def voc_score_edge_case():
    """2 classes x 3 images with negative scores, +0 / -0 ties, one NaN and one inf; every other detection sits on a
    ground-truth box of its segment."""
    rng = np.random.RandomState(31)
    vals = [-1.5, 0.0, -0.0, 0.25, -0.0, 0.0, np.nan, np.inf, -3e-310, 2.0, -1.5, 0.25, 0.0, -7.0]
    C, N = 2, 3
    box, conf, dcnt, gb, gcnt = [], [], [], [], []
    for s in range(C * N):
        g = _grid_boxes(4) + 200.0 * s
        gb.append(g)
        gcnt.append(4)
        n = 9 + s
        b = np.where((np.arange(n) % 2 == 0)[:, None], g[np.arange(n) % 4], g[np.arange(n) % 4] + 2000.0)
        box.append(b)
        conf.append(np.array([vals[(3 * s + k * 5) % len(vals)] for k in range(n)]))
        dcnt.append(n)
    conf = np.concatenate(conf)
    keep_nan = np.nonzero(np.isnan(conf))[0]
    conf[keep_nan[1:]] = -2.25                               # one NaN, one inf
    keep_inf = np.nonzero(np.isinf(conf))[0]
    conf[keep_inf[1:]] = 4.0
    gd = (rng.rand(C * N * 4) < 0.2).astype(np.uint8)
    return (C, N, np.vstack(box), conf, np.concatenate([[0], np.cumsum(dcnt)]), np.vstack(gb), gd,
            np.concatenate([[0], np.cumsum(gcnt)]))


# name -> class index in voc_class_curve_case
VOC_CURVE_CLASSES = {"n1": 0, "n255": 1, "empty_mid": 2, "n256": 3, "n0": 4, "n257": 5, "n513": 6, "nan_lead_300": 7,
                     "all_difficult": 8, "npos0_300": 9, "empty_end": 10}
VOC_CURVE_COUNTS = {"n1": 1, "n255": 255, "empty_mid": 0, "n256": 256, "n0": 0, "n257": 257, "n513": 513,
                    "nan_lead_300": 350, "all_difficult": 40, "npos0_300": 300, "empty_end": 0}


def voc_class_curve_case():
    """11 classes x 3 images in one call (VOC_CURVE_CLASSES): detection counts 0, 1, 255, 256, 257, 513 around
    k_voc_class's chunk of 256; a class with neither detections nor boxes in the middle and at the end; a class whose
    first 300 ranked detections sit on a difficult box (prec = 0 / 0 over a whole chunk) before 50 that count; a class
    whose detections all do; a class with 300 detections and only difficult boxes (npos = 0)."""
    rng = np.random.RandomState(77)
    N = 3
    names = sorted(VOC_CURVE_CLASSES, key=VOC_CURVE_CLASSES.get)
    box, conf, dcnt, gb, gd, gcnt = [], [], [], [], [], []
    for name in names:
        n = VOC_CURVE_COUNTS[name]
        per = [n // N + (1 if i < n % N else 0) for i in range(N)]
        for i in range(N):
            k = 0 if name.startswith("empty") else 6
            g = _grid_boxes(k) + 10.0 * i
            d = np.zeros(k, np.uint8)
            if k:
                d[1] = 1
            if name == "npos0_300":
                d[:] = 1
            m = per[i]
            if name == "nan_lead_300":                       # 100 per image on the difficult box score above 1
                b = np.vstack([np.tile(g[1], (100, 1)),
                               g[rng.choice([0, 2, 3, 4, 5], m - 100)] + rng.choice([0.0, 3.0, 40.0], (m - 100, 1))])
                c = np.concatenate([2.0 + np.round(rng.rand(100), 2), np.round(rng.rand(m - 100), 2)])
            elif name == "all_difficult":
                b = np.tile(g[1], (m, 1)) + rng.choice([0.0, 1.0], (m, 1))
                c = np.round(rng.rand(m), 1)
            else:
                b = g[rng.randint(0, 6, m)] + rng.choice([0.0, 3.0, 40.0], (m, 1)) if k else np.zeros((0, 4))
                c = np.round(rng.rand(m), 2)
            box.append(b.reshape(-1, 4)); conf.append(c); dcnt.append(m)
            gb.append(g); gd.append(d); gcnt.append(k)
    return (len(names), N, np.vstack(box), np.concatenate(conf), np.concatenate([[0], np.cumsum(dcnt)]),
            np.vstack(gb), np.concatenate(gd), np.concatenate([[0], np.cumsum(gcnt)]))


def voc_many_segments_case():
    """4 classes x 5000 images = 20 000 segments (more than the 16 384 waves k_voc_match launches), about 3 000
    detections and 4 000 boxes spread thinly."""
    rng = np.random.RandomState(20000)
    C, N = 4, 5000
    S = C * N
    dcnt = (rng.rand(S) < 0.12).astype(np.int64) * rng.randint(1, 3, S)
    gcnt = (rng.rand(S) < 0.15).astype(np.int64) * rng.randint(1, 3, S)
    dcnt[-1], gcnt[-1] = 2, 2
    D, G = int(dcnt.sum()), int(gcnt.sum())
    goff = np.concatenate([[0], np.cumsum(gcnt)])
    gb = _grid_boxes(4)[rng.randint(0, 4, G)]
    seg = np.repeat(np.arange(S), dcnt)
    box = _grid_boxes(4)[rng.randint(0, 4, D)] + rng.choice([0.0, 2.0, 9.0], (D, 1))
    conf = np.round(rng.rand(D), 2)
    gd = (rng.rand(G) < 0.1).astype(np.uint8)
    return C, N, box, conf, np.concatenate([[0], np.cumsum(dcnt)]), gb, gd, goff


# ---------------------------------------------------------------------------------------------------- COCO
COCO_G = [63, 64, 65, 66, 128, 129, 200]


def coco_specials(G):
    """(crowd boxes, boxes with an area outside 'medium', (first, duplicate) pairs) of coco_gt_count_case(G)."""
    crowd = [10] + [j for j in range(AZ_WAVE, G) if j % 4 == 1]
    small = [20] + [j for j in range(AZ_WAVE, G) if j % 4 == 2]
    dups = [(30, 50)] + [(a, b) for a, b in ((63, 64), (127, 128)) if b < G]
    return crowd, small, dups


def coco_gt_count_case(G):
    """One segment of G 40 x 40 boxes on a grid (area 1600: 'medium'); past j = 63 every fourth box is a crowd box and
    every fourth has area 500 (ignored in 'medium' and 'large'); box 64 copies box 63 (128 copies 127), so the last box
    of the highest IoU is decided across the register / HBM claim edge.  Three detections sit on every crowd box and
    every pair (the pairs' score highest), others on and beside plain boxes; quantised scores."""
    j = np.arange(G)
    gb = np.stack([50.0 * (j % 20), 50.0 * (j // 20), np.full(G, 40.0), np.full(G, 40.0)], 1)
    area = np.full(G, 1600.0)
    crowd = np.zeros(G, np.uint8)
    cr, sm, dups = coco_specials(G)
    crowd[cr] = 1
    area[sm] = 500.0
    for a, b in dups:
        gb[b] = gb[a]
    dets = []
    for t in [a for a, _ in dups] + cr[:3] + cr[-2:]:
        dets += [gb[t]] * 3
    for t in sm[:2] + sm[-1:]:
        dets += [gb[t], gb[t] + [4.0, 0.0, 0.0, 0.0]]
    for t in (0, 31, 61, 62, G - 1, G - 2):
        dets += [gb[t] + [4.0, 0.0, 0.0, 0.0], gb[t] + [0.0, 8.0, 0.0, 0.0], gb[t] + [12.0, 0.0, 0.0, 0.0]]
    dets += [np.array([3000.0, 3000.0, 10.0, 10.0]), np.array([3000.0, 100.0, 200.0, 200.0])]
    dets = np.array(dets)[:MAXDET]
    rng = np.random.RandomState(G)
    score = rng.randint(0, 8, len(dets)) / 8.0
    score[:3 * len(dups)] += 1.0                             # the pairs' detections rank before any other on their boxes
    o = rng.permutation(len(dets))
    return {"n_classes": 1, "n_images": 1, "det_box": dets[o], "det_score": score[o],
            "det_off": np.array([0, len(dets)]), "gt_box": gb, "gt_area": area, "gt_crowd": crowd, "gt_off": np.array([0, G])}


COCO_SEG_SIZES = [99, 100, 101, 164, 165]


def _coco_fill(rng, K, N, dcounts, gcounts):
    """Random detections near random grid boxes, segment (k, i) with dcounts[k][i] detections and gcounts[k][i] boxes."""
    dets, gts = [], []
    for k in range(K):
        for i in range(N):
            boxes = []
            for _ in range(gcounts[k][i]):
                b = [float(rng.randint(0, 20) * 8), float(rng.randint(0, 20) * 8), float(rng.choice([16, 32, 40, 96])),
                     float(rng.choice([16, 32, 48, 96]))]
                gts.append((k, i, b, float(rng.choice([b[2] * b[3], 1024.0, 9216.0])), int(rng.rand() < 0.1)))
                boxes.append(b)
            for _ in range(dcounts[k][i]):
                if boxes and rng.rand() < 0.7:
                    g = boxes[rng.randint(len(boxes))]
                    b = [g[0] + 4 * rng.randint(-1, 2), g[1] + 4 * rng.randint(-1, 2), max(4.0, g[2] + 4 * rng.randint(-2, 3)),
                         max(4.0, g[3] + 4 * rng.randint(-2, 3))]
                else:
                    b = [float(rng.randint(0, 30) * 8), float(rng.randint(0, 30) * 8), 32.0, 32.0]
                dets.append((k, i, [float(v) for v in b], float(rng.randint(0, 20)) / 20.0))
    perm = rng.permutation(len(dets))
    return coco_cases.pack(K, N, [dets[j] for j in perm], gts)


def coco_segment_size_case():
    """One category, five images with 99, 100, 101, 164 and 165 detections (MAXDET = 100; 165 = 2 * 64 + 37)."""
    return _coco_fill(np.random.RandomState(165), 1, len(COCO_SEG_SIZES), [COCO_SEG_SIZES], [[6] * len(COCO_SEG_SIZES)])


COCO_ACC_COUNTS = [CT - 1, CT, CT + 1, 600]


def coco_acc_chunk_case():
    """Four categories with 255, 256, 257 and 600 detections over 8 images, around k_coco_acc's chunk of 256."""
    N = 8
    dc = [[n // N + (1 if i < n % N else 0) for i in range(N)] for n in COCO_ACC_COUNTS]
    return _coco_fill(np.random.RandomState(256), len(COCO_ACC_COUNTS), N, dc, [[5] * N] * len(COCO_ACC_COUNTS))


# npig -> true positives, recall TP / npig on a recall threshold (1, 1, .5, .57, 1, .5, .5)
COCO_NPIG = {1: 1, 3: 3, 50: 25, 100: 57, 101: 101, 102: 51, 250: 125}


def coco_npig_case():
    """One category per npig of COCO_NPIG, its boxes dealt over 5 images; a detection exactly on each of the first TP
    boxes, every third detection a false positive in between."""
    N = 5
    dets, gts = [], []
    for k, (npig, tp) in enumerate(sorted(COCO_NPIG.items())):
        for j in range(npig):
            gts.append((k, j % N, [50.0 * (j // N % 10), 50.0 * (j // N // 10), 40.0, 40.0], 1600.0, 0))
        for j in range(tp):
            score = 1.0 - j / 256.0
            dets.append((k, j % N, gts[len(gts) - npig + j][2], score))
            if j % 3 == 1:
                dets.append((k, j % N, [4000.0, 4000.0, 40.0, 40.0], score))
    return coco_cases.pack(len(COCO_NPIG), N, dets, gts)


def coco_layout_cases():
    """name -> set: categories without boxes (with and without detections), with boxes and no detections, K = 1,
    K = 257 on a tiny set."""
    box = [0.0, 0.0, 40.0, 40.0]
    near = [4.0, 0.0, 40.0, 40.0]
    out = {}
    # category 0 plain, 1 no boxes but detections, 2 nothing at all, 3 boxes and no detections, 4 plain
    out["mixed"] = coco_cases.pack(5, 2, [(0, 0, box, .9), (0, 1, near, .8), (1, 0, box, .7), (1, 1, box, .7),
                                          (4, 1, near, .6), (4, 1, box, .6)],
                                   [(0, 0, box, 1600.0, 0), (0, 1, box, 1600.0, 0), (3, 0, box, 1600.0, 0),
                                    (3, 1, box, 500.0, 1), (4, 1, box, 1600.0, 0)])
    out["k1"] = coco_cases.pack(1, 3, [(0, 0, box, .9), (0, 2, near, .9), (0, 2, box, .9)],
                                [(0, 0, box, 1600.0, 0), (0, 2, box, 1600.0, 0), (0, 1, box, 1600.0, 0)])
    dets, gts = [], []
    for k in (0, 1, 128, 255, 256):
        gts.append((k, 0, box, 1600.0, 0))
        dets += [(k, 0, near, .5), (k, 0, box, .25 + (k % 2) * .5)]
    dets.append((200, 0, box, .5))
    out["k257"] = coco_cases.pack(257, 1, dets, gts)
    return out


COCO_CASE_NAMES = ["gt_%d" % G for G in COCO_G] + ["segment_sizes", "acc_chunk", "npig", "layout_mixed", "layout_k1",
                                                   "layout_k257"]


def coco_cases_all():
    out = {"gt_%d" % G: coco_gt_count_case(G) for G in COCO_G}
    out.update(segment_sizes=coco_segment_size_case(), acc_chunk=coco_acc_chunk_case(), npig=coco_npig_case())
    out.update({"layout_" + k: v for k, v in coco_layout_cases().items()})
    return out


# ---------------------------------------------------------------------------------------------------- recall matching
RECALL_K = [RM_T - 1, RM_T, RM_T + 1, 300]
# (k1, k2): columns whose maxima tie -- (5, 200) meet in the reduction over threads, the lower column in the lower
# thread; (2, 256) there too, the higher column in the lower thread; (1, 257) in thread 1's own stride
RECALL_TIES = [(5, 200), (2, 256), (1, 257)]


def recall_ties(K):
    return [(a, b) for a, b in RECALL_TIES if b < K]


def recall_case(K, extra=20):
    """One image: K 20 x 20 ground-truth boxes far apart, K + extra candidates.  Every box has a jittered candidate.
    For every pair of recall_ties(K) the two boxes lie side by side under one wide candidate (overlap 400 / 1200 with
    both, their column maximum), the first box has a second candidate at 400 / 1600, the second one at 400 / 2000:
    which box is taken first decides what the other is left with.  Box 30 copies box 31 and the last candidate copies
    the first (plain duplicates)."""
    rng = np.random.RandomState(K)
    k = np.arange(K)
    gx, gy = 200.0 * (k % 16), 200.0 * (k // 16)
    gt = np.stack([gx, gy, gx + 19.0, gy + 19.0], 1)
    cand = gt + np.floor(rng.uniform(-4, 5, (K, 4)))
    plain = np.array([j for j in range(K) if all(j not in p for p in recall_ties(K))])
    more = gt[plain[rng.randint(0, plain.size, extra)]] + np.floor(rng.uniform(-9, 10, (extra, 4)))
    tied = []
    for a, b in recall_ties(K):
        x, y = gt[a, 0], gt[a, 1]
        gt[b] = [x + 40.0, y, x + 59.0, y + 19.0]
        cand[a] = [x, y, x + 59.0, y + 19.0]                 # over both: 400 / 1200
        cand[b] = [x, y, x + 19.0, y + 79.0]                 # box a only: 400 / 1600
        tied.append([x + 40.0, y, x + 59.0, y + 99.0])       # box b only: 400 / 2000
    gt[30] = gt[31]
    cand = np.vstack([cand, more] + ([np.array(tied)] if tied else []))
    cand[-1 - len(tied)] = cand[0]
    return cand, gt
