"""NumPy restatement of the detection diagnosis ("Detection diagnosis"): every false positive of a VOC
evaluation typed after Hoiem et al. (ECCV 2012) and the AP recomputed with each type fixed, after TIDE (Bolya et al.,
ECCV 2020).  It walks detections one at a time, as voc_eval_ref.evaldet does, and is the definition az_det_diag_eval is
held to.  Also the case builders of test_ddiag_host.py / test_gpu_ddiag.py.  Test infrastructure only: no product file
imports it."""
import math

import numpy as np

import voc_eval_ref as V

IGN, TP, DUP, LOC, SIM, OTH, BG = range(7)
N_TYPES, N_VARIANTS, MAX_CUTS = 7, 8, 16
TYPE_NAMES = ("IGN", "TP", "DUP", "LOC", "SIM", "OTH", "BG")
VOC_CLASSES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
               "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
# Hoiem's sets: vehicles 0, animals 1, furniture 2, person 3; bottle 4 and tvmonitor 5 on their own
VOC_GROUPS = np.array([0, 0, 1, 0, 4, 0, 0, 1, 2, 1, 2, 1, 1, 0, 3, 2, 1, 2, 0, 5], np.int32)


def overlap(bb, g):
    """VOCevaldet's overlap in its operation order; None where the boxes do not intersect."""
    iw = min(bb[2], g[2]) - max(bb[0], g[0]) + 1
    ih = min(bb[3], g[3]) - max(bb[1], g[1]) + 1
    if iw > 0 and ih > 0:
        ua = (bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + (g[2] - g[0] + 1) * (g[3] - g[1] + 1) - iw * ih
        return iw * ih / ua
    return None


def variant_tp_fp(v, ty, fixed):
    """What a detection of type `ty` counts as under variant v: (tp, fp)."""
    if ty == TP:
        return 1, 0
    if ty == IGN:
        return 0, 0
    if ty == LOC and v in (2, 7):
        return (1, 0) if fixed else (0, 0)
    removed = {1: DUP, 3: SIM, 4: OTH, 5: BG}.get(v)
    if v == 7 or ty == removed:
        return 0, 0
    return 0, 1


def cut_count(cut, npos, n):
    x = cut * float(npos)
    return n if x >= n else int(math.floor(x))


def diag_flat(n_classes, n_images, det_box, det_conf, det_off, gt_box, gt_diff, gt_off, min_overlap=0.5, bg_overlap=0.1,
              metric_07=True, class_group=None, cuts=()):
    """The segment layout of az_det_diag_eval (class-major segments, as az_voc_eval's)."""
    C, N = int(n_classes), int(n_images)
    if not np.isfinite(np.asarray(cuts, np.float64)).all():
        raise ValueError("diag_flat: the cuts must be finite")      # az_det_diag_eval refuses them: inf * (npos = 0) is NaN
    det_box = np.asarray(det_box, np.float64).reshape(-1, 4)
    det_conf = np.asarray(det_conf, np.float64).ravel()
    gt_box = np.asarray(gt_box, np.float64).reshape(-1, 4)
    gt_diff = np.asarray(gt_diff).ravel().astype(bool)
    det_off, gt_off = np.asarray(det_off, np.int64), np.asarray(gt_off, np.int64)
    D, G = int(det_off[-1]), int(gt_off[-1])
    group = np.arange(C) if class_group is None else np.asarray(class_group)
    gl = [[float(v) for v in g] for g in gt_box]
    out = {"type": np.zeros(D, np.int8), "ov_same": np.zeros(D), "arg_same": np.full(D, -1, np.int32),
           "ov_other": np.zeros(D), "other_class": np.full(D, -1, np.int32), "loc_fixed": np.zeros(D, np.uint8),
           "gt_claim": np.full(G, -1, np.int32), "type_table": np.zeros((C, N_TYPES), np.int64),
           "miss": np.zeros(C, np.int64), "fp_at": np.zeros((C, len(cuts), N_TYPES), np.int64),
           "npos": np.zeros(C, np.int64), "ap_fix": np.zeros((C, N_VARIANTS))}
    ty, fixed, claim = out["type"], out["loc_fixed"], out["gt_claim"]
    for c in range(C):
        lo, hi = int(det_off[c * N]), int(det_off[(c + 1) * N])
        img = np.repeat(np.arange(N), np.diff(det_off[c * N:(c + 1) * N + 1]))
        order = lo + np.argsort(-det_conf[lo:hi], kind="stable")
        for d in order:
            i = int(img[d - lo])
            bb = [float(v) for v in det_box[d]]
            g0, g1 = int(gt_off[c * N + i]), int(gt_off[c * N + i + 1])
            ovs, js = -np.inf, -1
            for j in range(g0, g1):
                ov = overlap(bb, gl[j])
                if ov is not None and ov > ovs:
                    ovs, js = ov, j - g0
            ovo, co = -np.inf, -1
            for c2 in range(C):
                if c2 == c:
                    continue
                for j in range(int(gt_off[c2 * N + i]), int(gt_off[c2 * N + i + 1])):
                    ov = overlap(bb, gl[j])
                    if ov is not None and ov > ovo:
                        ovo, co = ov, c2
            if js >= 0 and ovs >= min_overlap:
                if gt_diff[g0 + js]:
                    t = IGN
                elif claim[g0 + js] < 0:
                    t = TP
                    claim[g0 + js] = d
                else:
                    t = DUP
            elif js >= 0 and ovs >= bg_overlap:
                t = LOC
            elif co >= 0 and ovo >= bg_overlap:
                t = SIM if group[c] == group[co] else OTH
            else:
                t = BG
            ty[d] = t
            out["ov_same"][d], out["arg_same"][d] = (ovs, js) if js >= 0 else (0.0, -1)
            out["ov_other"][d], out["other_class"][d] = (ovo, co) if co >= 0 else (0.0, -1)
        # the TIDE rule: a second walk, once the whole class (so every segment of it) is matched
        taken = set()
        for d in order:
            if ty[d] != LOC:
                continue
            i = int(img[d - lo])
            g = int(gt_off[c * N + i]) + int(out["arg_same"][d])
            if not gt_diff[g] and claim[g] < 0 and g not in taken:
                taken.add(g)
                fixed[d] = 1
        ga, gb = int(gt_off[c * N]), int(gt_off[(c + 1) * N])
        npos = int((~gt_diff[ga:gb]).sum())
        out["npos"][c] = npos
        out["miss"][c] = int((~gt_diff[ga:gb] & (claim[ga:gb] < 0)).sum())
        tr = ty[order] if order.size else np.zeros(0, np.int8)
        out["type_table"][c] = np.bincount(tr, minlength=N_TYPES)
        for k, cut in enumerate(cuts):
            out["fp_at"][c, k] = np.bincount(tr[:cut_count(float(cut), npos, order.size)], minlength=N_TYPES)
        n_tp, n_fix = int((tr == TP).sum()), int(fixed[order].sum()) if order.size else 0
        for v in range(N_VARIANTS):
            np_v = n_tp if v == 6 else (n_tp + n_fix if v == 7 else npos)
            pairs = [variant_tp_fp(v, int(ty[d]), int(fixed[d])) for d in order]
            tp = np.cumsum(np.array([p[0] for p in pairs], np.float64))
            fp = np.cumsum(np.array([p[1] for p in pairs], np.float64))
            with np.errstate(divide="ignore", invalid="ignore"):
                rec = tp / float(np_v) if np_v else tp / np.zeros_like(tp)
                prec = tp / (fp + tp)
                out["ap_fix"][c, v] = V.ap11(rec, prec) if metric_07 else V.xvocap(rec, prec)
    return out


def to_match(ty):
    """az_voc_eval's match from the types: TP +1, IGN 0, everything else -1."""
    ty = np.asarray(ty)
    return np.where(ty == TP, 1, np.where(ty == IGN, 0, -1)).astype(np.int8)


# ------------------------------------------------------------------------------------------------------------- cases
def pack(C, N, dets, gts):
    """dets: (class, image, box, conf) in file order within a segment; gts: (class, image, box, difficult).
    -> the argument tuple (C, N, det_box, det_conf, det_off, gt_box, gt_diff, gt_off)."""
    S = C * N
    db = [[] for _ in range(S)]
    gb = [[] for _ in range(S)]
    for c, i, b, s in dets:
        db[c * N + i].append(list(b) + [s])
    for c, i, b, d in gts:
        gb[c * N + i].append(list(b) + [d])
    dflat = np.array([r for s in db for r in s], np.float64).reshape(-1, 5)
    gflat = np.array([r for s in gb for r in s], np.float64).reshape(-1, 5)
    doff = np.concatenate([[0], np.cumsum([len(s) for s in db])]).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum([len(s) for s in gb])]).astype(np.int64)
    return (C, N, np.ascontiguousarray(dflat[:, :4]), dflat[:, 4].copy(), doff, np.ascontiguousarray(gflat[:, :4]),
            gflat[:, 4].astype(np.uint8), goff)


def sub_image(case, i):
    """Image i of a case as a one-image case, and the rows (detections, boxes) it takes from the joint arrays."""
    C, N, db, dc, doff, gb, gd, goff = case
    dr = np.concatenate([np.arange(doff[c * N + i], doff[c * N + i + 1]) for c in range(C)] + [np.zeros(0, np.int64)]).astype(np.int64)
    gr = np.concatenate([np.arange(goff[c * N + i], goff[c * N + i + 1]) for c in range(C)] + [np.zeros(0, np.int64)]).astype(np.int64)
    d1 = np.concatenate([[0], np.cumsum([doff[c * N + i + 1] - doff[c * N + i] for c in range(C)])]).astype(np.int64)
    g1 = np.concatenate([[0], np.cumsum([goff[c * N + i + 1] - goff[c * N + i] for c in range(C)])]).astype(np.int64)
    return (C, 1, db[dr], dc[dr], d1, gb[gr], gd[gr], g1), dr, gr


def grid_box(j):
    """20 x 20 boxes 30 apart, 100 to a row (eval_edges_cases._grid_boxes)."""
    x, y = 1.0 + 30.0 * (j % 100), 1.0 + 30.0 * (j // 100)
    return [x, y, x + 19.0, y + 19.0]


def shifted(b, frac):
    """b moved right by frac of its width, on whole pixels."""
    s = float(round((b[2] - b[0] + 1) * frac))
    return [b[0] + s, b[1], b[2] + s, b[3]]


def random_case(C, N, seed, n_det=(0, 6), n_gt=(0, 4), p_diff=0.15):
    """Random sets on a coarse pixel grid: detections on, beside and far from boxes of their own and other classes,
    quantised scores (ties), some difficult boxes."""
    rng = np.random.RandomState(seed)
    dets, gts, per_img, own = [], [], [[] for _ in range(N)], {}
    for c in range(C):
        for i in range(N):
            for _ in range(rng.randint(n_gt[0], n_gt[1] + 1)):
                x, y = float(rng.randint(0, 12) * 16), float(rng.randint(0, 10) * 16)
                b = [x + 1, y + 1, x + float(rng.choice([16, 32, 48])), y + float(rng.choice([16, 32, 48]))]
                gts.append((c, i, b, int(rng.rand() < p_diff)))
                per_img[i].append(b)
                own.setdefault((c, i), []).append(b)
    for c in range(C):
        for i in range(N):
            for _ in range(rng.randint(n_det[0], n_det[1] + 1)):
                if per_img[i] and rng.rand() < 0.85:
                    pool = own[(c, i)] if (c, i) in own and rng.rand() < 0.6 else per_img[i]
                    g = pool[rng.randint(len(pool))]
                    w = g[2] - g[0] + 1
                    sx = float(rng.choice([0, 0, 0, 4, 8, 16, 24])) * (1 if rng.rand() < 0.5 else -1)
                    b = [g[0] + sx, g[1] + float(rng.choice([0, 0, 4, 12])), g[2] + sx, g[3]]
                    if rng.rand() < 0.1:
                        b = [g[0], g[1], g[0] + w * 2, g[3]]
                else:
                    b = [900.0 + 8 * rng.randint(0, 10), 900.0, 930.0 + 8 * rng.randint(0, 10), 940.0]
                dets.append((c, i, b, float(rng.randint(0, 16)) / 16.0))
    return pack(C, N, dets, gts)


def hand_case():
    """3 classes x 2 images, 12 detections, every type, a fixed and an unfixed LOC, a missed object.  Classes 0 and 1
    share a group; class 2 is on its own.  Boxes are 10 x 10 unless said; the answers are written out in
    test_ddiag_host.py.
      image 0: class 0 boxes A (1,1) and B (101,1) difficult and E (301,1); class 1 box C (201,1); class 2 box F (1,101)
      image 1: class 0 box G0 (1,1); class 2 box H (101,1) difficult
    """
    def sq(x, y, w=10, h=10):
        return [float(x), float(y), float(x + w - 1), float(y + h - 1)]
    A, B, E, Cb, F, G0, H = sq(1, 1), sq(101, 1), sq(301, 1), sq(201, 1), sq(1, 101), sq(1, 1), sq(101, 1)
    gts = [(0, 0, A, 0), (0, 0, B, 1), (0, 0, E, 0), (1, 0, Cb, 0), (2, 0, F, 0), (0, 1, G0, 0), (2, 1, H, 1)]
    dets = [
        # class 0, image 0 (file order; ranks by conf)
        (0, 0, A, 0.9),                       # d0  TP on A
        (0, 0, A, 0.8),                       # d1  DUP
        (0, 0, B, 0.7),                       # d2  IGN (difficult)
        (0, 0, sq(306, 1), 0.6),              # d3  LOC on E: 50 / 150 = 1/3, fixed (E is never claimed)
        (0, 0, sq(307, 1), 0.5),              # d4  LOC on E: 40 / 160 = 1/4, not fixed (d3 took E)
        (0, 0, Cb, 0.4),                      # d5  SIM: class 1's box, same group
        (0, 0, F, 0.3),                       # d6  OTH: class 2's box
        (0, 0, sq(601, 601), 0.2),            # d7  BG
        # class 0, image 1
        (0, 1, sq(1, 1, 10, 20), 0.95),       # d8  TP on G0 at exactly 0.5
        (0, 1, H, 0.1),                       # d9  OTH on a difficult box of class 2
        # class 1, image 0
        (1, 0, sq(205, 1), 0.9),              # d10 LOC on C: 60 / 140 = 3/7, fixed; C is missed
        # class 2, image 0
        (2, 0, F, 0.5),                       # d11 TP on F
    ]
    return pack(3, 2, dets, gts), np.array([0, 0, 1], np.int32)


def wave_case(n_det, n_gt, C=3, seed=0):
    """One image, C classes: class 1 has n_det detections, the image n_gt boxes over all classes (dealt round the
    classes), every box on the grid.  Detections sit on boxes of any class, beside them, and nowhere."""
    rng = np.random.RandomState(seed + 1000 * n_det + n_gt)
    gts = [(j % C, 0, grid_box(j), int(rng.rand() < 0.15)) for j in range(n_gt)]
    dets = []
    for k in range(n_det):
        g = grid_box(int(rng.randint(0, n_gt)))
        r = rng.rand()
        b = g if r < 0.5 else (shifted(g, 0.6) if r < 0.8 else [9000.0, 9000.0, 9019.0, 9019.0])
        dets.append((1 % C, 0, b, float(rng.randint(0, 32)) / 32.0))
    for c in range(C):
        if c != 1 % C:
            dets.append((c, 0, grid_box(int(rng.randint(0, n_gt))), 0.5))
    return pack(C, 1, dets, gts)


# (first, copy) positions in the image's (class, position) list, chosen as eval_edges_cases.VOC_TIE_PAIRS are: either side of
# box 63 / 64, two lanes of one round, j and j + 64 in one lane, a low j in a high lane against a higher j in a lower lane
TIE_PAIRS = [(63, 64), (3, 40), (0, 65), (5, 69), (60, 66), (10, 127), (1, 128), (62, 129)]


def tie_case(same):
    """One image, 2 classes, 130 boxes.  same: class 0 owns all 130 boxes, box b of every pair copies box a and exactly
    one of the two is difficult; class 0's detections sit exactly on the pairs, so the first maximum decides IGN
    against TP.  not same: classes 1 .. 130 own one box each (131 classes), the pairs' classes alternate between the
    detection class's group and another, so the first maximum decides SIM against OTH and names other_class."""
    M = 130
    boxes = [grid_box(j) for j in range(M)]
    pairs = [(a, b) for a, b in TIE_PAIRS]
    used = set()
    keep = []
    for a, b in pairs:                         # a box takes part in one pair only
        if a in used or b in used:
            continue
        used.update((a, b))
        keep.append((a, b))
    diff = np.zeros(M, np.uint8)
    for k, (a, b) in enumerate(keep):
        boxes[b] = boxes[a]
        diff[a], diff[b] = (0, 1) if k % 2 == 0 else (1, 0)
    dets = [(0, 0, boxes[a], 1.0 - k / 64.0) for k, (a, _) in enumerate(keep)]
    dets += [(0, 0, boxes[j], 0.25) for j in range(M) if j not in used]          # every lane's box is a maximum once
    if same:
        return pack(2, 1, dets, [(0, 0, boxes[j], int(diff[j])) for j in range(M)]), None, keep
    C = M + 1
    group = np.zeros(C, np.int32)
    for k, (a, b) in enumerate(keep):
        group[1 + a], group[1 + b] = (0, 7) if k % 2 == 0 else (7, 0)
    return pack(C, 1, dets, [(1 + j, 0, boxes[j], int(diff[j])) for j in range(M)]), group, keep


def threshold_case():
    """2 classes x 4 images.  Image 0: a 10x10 detection in a 10x20 box of its class (exactly 0.5).  Image 1: a 10x1
    box of its class inside a 10x10 detection (exactly 0.1).  Image 2: the 10x1 box belongs to the other class.
    Image 3: a detection that overlaps nothing."""
    gts = [(0, 0, [1.0, 1.0, 10.0, 20.0], 0), (0, 1, [1.0, 1.0, 10.0, 1.0], 0), (1, 2, [1.0, 1.0, 10.0, 1.0], 0),
           (1, 3, [1.0, 1.0, 10.0, 10.0], 0)]
    sq = [1.0, 1.0, 10.0, 10.0]
    dets = [(0, 0, sq, 0.9), (0, 1, sq, 0.8), (0, 2, sq, 0.7), (0, 3, [500.0, 500.0, 509.0, 509.0], 0.6)]
    return pack(2, 4, dets, gts)


def difficult_case():
    """2 classes (different groups) x 1 image: class 0's difficult box A with a detection on it (IGN) and one shifted
    off it (LOC, not fixed); class 1's difficult box B with a class 0 detection on it (OTH)."""
    A, B = grid_box(0), grid_box(5)
    gts = [(0, 0, A, 1), (1, 0, B, 1)]
    dets = [(0, 0, A, 0.9), (0, 0, shifted(A, 0.6), 0.8), (0, 0, B, 0.7)]
    return pack(2, 1, dets, gts)


def chunk_case():
    """One class x 1 image, 130 detections in rank order = file order, 4 boxes.  Ranks 3 / 70: TP on box 0 and its DUP
    in the second chunk of 64.  Ranks 5 / 69: two LOC on the unclaimed box 1, only the first fixed.  Rank 2: a LOC on
    box 2, which the TP at rank 100 claims: not fixed.  Box 3 is missed.  The rest overlap nothing."""
    n = 130
    gb = [grid_box(0), grid_box(3), grid_box(6), grid_box(9)]
    box = [[5000.0 + 30 * k, 5000.0, 5019.0 + 30 * k, 5019.0] for k in range(n)]
    box[3], box[70] = gb[0], gb[0]
    box[5], box[69] = shifted(gb[1], 0.6), shifted(gb[1], 0.5)
    box[2], box[100] = shifted(gb[2], 0.6), gb[2]
    dets = [(0, 0, box[k], 1.0 - k / 1000.0) for k in range(n)]
    return pack(1, 1, dets, [(0, 0, g, 0) for g in gb])


def score_case():
    """2 classes x 2 images whose confidences hold ties, +0 / -0, one NaN, +inf and -inf."""
    vals = [0.5, 0.5, 0.0, -0.0, np.nan, np.inf, -np.inf, 0.5, -1.0, 0.25, 0.25, 2.0]
    gts = [(c, i, grid_box(3 * c + i + k * 7), 0) for c in range(2) for i in range(2) for k in range(3)]
    dets = []
    for k, v in enumerate(vals * 2):
        c, i = k % 2, (k // 2) % 2
        g = grid_box(3 * c + i + (k % 3) * 7)
        dets.append((c, i, g if k % 4 else shifted(g, 0.6), v))
    return pack(2, 2, dets, gts)


def cuts_case():
    """One class, 1 image: npos = 4, 10 detections (4 TP, 2 DUP, 4 BG interleaved)."""
    gb = [grid_box(j) for j in range(4)]
    seq = [gb[0], [9000.0, 1.0, 9019.0, 20.0], gb[1], gb[0], gb[2], [9100.0, 1.0, 9119.0, 20.0], gb[3], gb[3],
           [9200.0, 1.0, 9219.0, 20.0], [9300.0, 1.0, 9319.0, 20.0]]
    dets = [(0, 0, b, 1.0 - k / 16.0) for k, b in enumerate(seq)]
    return pack(1, 1, dets, [(0, 0, g, 0) for g in gb])


# integer (4 * 0.5), fractional (4 * 0.6 -> 2), 0, past the 10 detections
CUTS_EDGE = (0.0, 0.5, 0.6, 1.0, 2.4, 2.5, 3.0, 1e300)


def class_count_case(C, seed=0):
    """C classes x 2 images; boxes and detections in a handful of classes around the edges of the class-id radix byte
    (0, 1, 255, 256, C - 1 where they exist), a detection of each on a box of the next listed class."""
    live = sorted(set(c for c in (0, 1, 2, 20, 255, 256, C - 1) if c < C))
    rng = np.random.RandomState(seed + C)
    gts, dets = [], []
    for k, c in enumerate(live):
        for i in range(2):
            gts.append((c, i, grid_box(10 * k + i), int(k == 2)))
            gts.append((c, i, grid_box(10 * k + i + 300), 0))
    for k, c in enumerate(live):
        nxt = (k + 1) % len(live)
        for i in range(2):
            dets.append((c, i, grid_box(10 * k + i), 0.9))
            dets.append((c, i, grid_box(10 * k + i), 0.8))
            dets.append((c, i, shifted(grid_box(10 * k + i + 300), 0.6), float(rng.randint(0, 8)) / 8))
            dets.append((c, i, grid_box(10 * nxt + i), 0.5))
            dets.append((c, i, [8000.0, 8000.0, 8019.0, 8019.0], 0.4))
    return pack(C, 2, dets, gts)


def other_tie_case():
    """4 classes x 1 image: classes 1 and 3 own the same box; class 2's and class 0's detections on it name class 1
    (the lower class wins the tie), class 1's names class 3."""
    b = grid_box(0)
    return pack(4, 1, [(0, 0, b, 0.5), (1, 0, shifted(b, 2.0), 0.5), (2, 0, b, 0.5), (1, 0, b, 0.4)],
                [(3, 0, b, 0), (1, 0, shifted(b, 2.0), 0), (1, 0, b, 1)])


def many_segments_case():
    """4 classes x 5000 images = 20 000 segments (more than the waves k_ddiag_match launches), 0-3 rows each."""
    rng = np.random.RandomState(20000)
    C, N = 4, 5000
    S = C * N
    dcnt = (rng.rand(S) < 0.15).astype(np.int64) * rng.randint(1, 4, S)
    gcnt = (rng.rand(S) < 0.2).astype(np.int64) * rng.randint(1, 4, S)
    dcnt[-1], gcnt[-1] = 3, 3
    D, G = int(dcnt.sum()), int(gcnt.sum())
    grid = np.array([grid_box(j) for j in range(4)])
    gb = grid[rng.randint(0, 4, G)]
    box = grid[rng.randint(0, 4, D)] + rng.choice([0.0, 2.0, 9.0, 14.0], (D, 1))
    conf = np.round(rng.rand(D), 2)
    gd = (rng.rand(G) < 0.1).astype(np.uint8)
    return C, N, box, conf, np.concatenate([[0], np.cumsum(dcnt)]), gb, gd, np.concatenate([[0], np.cumsum(gcnt)])


def voc07_case(n_images=4952, n_classes=20, seed=2007):
    """The VOC07-test-sized synthetic set of test_gpu_voc_eval.test_voc07_scale (the README's VOC row): about 40
    detections and 1.2 boxes per (class, image), three detections in ten near a box of their segment."""
    rng = np.random.RandomState(seed)
    C, N = n_classes, n_images
    dcnt = rng.poisson(40, C * N)
    gcnt = rng.poisson(1.2, C * N)
    D, G = int(dcnt.sum()), int(gcnt.sum())
    det_off, goff = np.concatenate([[0], np.cumsum(dcnt)]), np.concatenate([[0], np.cumsum(gcnt)])
    gx = rng.uniform(0, 400, (G, 2))
    gw = rng.uniform(20, 200, (G, 2))
    gb = np.round(np.concatenate([gx, gx + gw], 1), 0) + 1
    gd = (rng.rand(G) < 0.1).astype(np.uint8)
    dx = rng.uniform(0, 400, (D, 2))
    dw = rng.uniform(20, 200, (D, 2))
    db = np.round(np.concatenate([dx, dx + dw], 1), 1) + 1
    seg = np.repeat(np.arange(C * N), dcnt)
    near = (rng.rand(D) < 0.3) & (gcnt[seg] > 0)
    gi = goff[seg[near]] + (rng.rand(int(near.sum())) * gcnt[seg[near]]).astype(np.int64)
    db[near] = np.round(gb[gi] + rng.normal(0, 4, (int(near.sum()), 4)), 1)
    conf = np.round(rng.rand(D), 3)
    return C, N, db, conf, det_off, gb, gd, goff
