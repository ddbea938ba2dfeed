"""NumPy restatement of az_coco_diag_eval ("Detection diagnosis, COCO protocol"), written loop for loop on top of
coco_eval_ref.evaluate_img / bb_iou so that the kernels can be held to it bit for bit, the cases the CPU and GPU tests share,
and a hand-worked set of 13 detections whose types, fixes and variant APs are written out as fractions.  Slow, for tests only."""
from fractions import Fraction

import numpy as np

import coco_eval_ref as R
from coco_cases import pack

IGN, TP, DUP, LOC, SIM, OTH, BG = range(7)
T, NR, NV = len(R.IOU_THRS), len(R.REC_THRS), 8
A_ALL = R.AREA_RNG[0]
KEYS = ("n_classes", "n_images", "det_box", "det_score", "det_off", "gt_box", "gt_area", "gt_crowd", "gt_off")
INT_KEYS = ("arg_same", "other_class", "type", "loc_fixed", "gt_claim", "npos", "type_table", "miss")


def args(c):
    return [c[k] for k in KEYS]


def _pair(d, g):
    """bbIou of one detection with one plain box, or None where w <= 0 or h <= 0 (the pair does not count)."""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return None
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return None
    return float(R.bb_iou([d], [g], [0])[0, 0])


def accumulate_one(tps, fps, npig):
    """accumulate's inner loop for one threshold: tps / fps bool [nd] in the class-ranked order.  -> (q [101], recall)."""
    tp = np.cumsum(tps).astype(dtype=float)
    fp = np.cumsum(fps).astype(dtype=float)
    nd = len(tp)
    rc = tp / npig
    pr = tp / (fp + tp + np.spacing(1))
    q = np.zeros((NR,)).tolist()
    recall = rc[-1] if nd else 0
    pr = pr.tolist()
    for i in range(nd - 1, 0, -1):
        if pr[i] > pr[i - 1]:
            pr[i - 1] = pr[i]
    inds = np.searchsorted(rc, R.REC_THRS, side="left")
    try:
        for ri, pi in enumerate(inds):
            q[ri] = pr[pi]
    except IndexError:
        pass
    return np.array(q), recall


def diag(n_classes, n_images, det_box, det_score, det_off, gt_box, gt_area, gt_crowd, gt_off, bg_overlap=0.1,
         class_group=None):
    """Same inputs and outputs as AzContext.coco_diag_eval (without ap_fix / stats_fix: ffi.coco_diag_means adds them)."""
    K, N = int(n_classes), int(n_images)
    det_box = np.asarray(det_box, np.float64).reshape(-1, 4)
    gt_box = np.asarray(gt_box, np.float64).reshape(-1, 4)
    det_off, gt_off = np.asarray(det_off, np.int64), np.asarray(gt_off, np.int64)
    D, G = len(det_score), len(gt_area)
    group = list(range(K)) if class_group is None else [int(g) for g in class_group]
    counts = [not gt_crowd[q] and not (gt_area[q] < A_ALL[0] or gt_area[q] > A_ALL[1]) for q in range(G)]
    out = {"ov_same": np.zeros(D), "arg_same": -np.ones(D, np.int32), "ov_other": np.zeros(D),
           "other_class": -np.ones(D, np.int32), "type": -np.ones((T, D), np.int8), "loc_fixed": np.zeros((T, D), np.uint8),
           "gt_claim": -np.ones((T, G), np.int32), "npos": np.zeros(K, np.int64), "type_table": np.zeros((K, T, 7), np.int64),
           "miss": np.zeros((K, T), np.int64), "prec_fix": -np.ones((NV, T, NR, K)), "recall_fix": -np.ones((NV, T, K))}
    image_boxes = [[(kk, q) for kk in range(K) for q in range(gt_off[kk * N + i], gt_off[kk * N + i + 1])] for i in range(N)]
    evals = {}
    for k in range(K):
        for i in range(N):
            s = k * N + i
            dts = [{"bbox": [float(v) for v in det_box[p]], "score": float(det_score[p]),
                    "area": float(det_box[p, 2]) * float(det_box[p, 3]), "id": p + 1, "pos": p}
                   for p in range(det_off[s], det_off[s + 1])]
            gts = [{"bbox": [float(v) for v in gt_box[q]], "area": float(gt_area[q]), "iscrowd": int(gt_crowd[q]),
                    "id": q + 1, "pos": q - gt_off[s]} for q in range(gt_off[s], gt_off[s + 1])]
            e = R.evaluate_img(dts, gts, A_ALL, R.MAX_DETS[-1])
            evals[s] = e
            if e is None:
                continue
            g0 = int(gt_off[s])
            fixed_onto = np.zeros((T, G), bool)
            for dind, p in enumerate(e["dtPos"]):                 # the segment's first 100, in rank order
                d = [float(v) for v in det_box[p]]
                best_s, arg_s, best_o, cls_o = None, -1, None, -1
                for kk, q in image_boxes[i]:                      # (category, position) order: the first maximum wins
                    if not counts[q]:
                        continue
                    o = _pair(d, [float(v) for v in gt_box[q]])
                    if o is None:
                        continue
                    if kk == k:
                        if best_s is None or o > best_s:
                            best_s, arg_s = o, q - g0
                    elif best_o is None or o > best_o:
                        best_o, cls_o = o, kk
                out["ov_same"][p], out["arg_same"][p] = (best_s, arg_s) if best_s is not None else (0.0, -1)
                out["ov_other"][p], out["other_class"][p] = (best_o, cls_o) if best_o is not None else (0.0, -1)
                for t in range(T):
                    m, ig = int(e["dtGtPos"][t, dind]), bool(e["dtIgnore"][t, dind])
                    if ig:
                        ty = IGN                                  # matched to an ignored box, or unmatched and out of range
                    elif m >= 0:
                        ty = TP
                        out["gt_claim"][t, g0 + m] = p
                    elif best_s is not None and best_s >= R.IOU_THRS[t]:
                        ty = DUP
                    elif best_s is not None and best_s >= bg_overlap:
                        ty = LOC
                    elif best_o is not None and best_o >= bg_overlap:
                        ty = SIM if group[k] == group[cls_o] else OTH
                    else:
                        ty = BG
                    out["type"][t, p] = ty
            for t in range(T):                                    # TIDE's rule, once the segment's claims are made
                for dind, p in enumerate(e["dtPos"]):
                    if out["type"][t, p] != LOC:
                        continue
                    g = g0 + int(out["arg_same"][p])
                    if out["gt_claim"][t, g] < 0 and not fixed_onto[t, g]:
                        fixed_onto[t, g] = True
                        out["loc_fixed"][t, p] = 1
    for k in range(K):
        glo, ghi = int(gt_off[k * N]), int(gt_off[(k + 1) * N])
        dlo, dhi = int(det_off[k * N]), int(det_off[(k + 1) * N])
        cnt = np.array(counts[glo:ghi], bool)
        out["npos"][k] = int(cnt.sum())
        for t in range(T):
            out["miss"][k, t] = int((cnt & (out["gt_claim"][t, glo:ghi] < 0)).sum())
            for ty in range(7):
                out["type_table"][k, t, ty] = int((out["type"][t, dlo:dhi] == ty).sum())
        # accumulate(): the segments' kept detections in image order, then the stable sort by -score
        E = [evals[k * N + i] for i in range(N)]
        E = [e for e in E if e is not None]
        if len(E) == 0:
            continue
        pos = np.array([p for e in E for p in e["dtPos"]], np.int64)
        scores = np.array([float(det_score[p]) for p in pos])
        pos = pos[np.argsort(-scores, kind="mergesort")]
        for t in range(T):
            ty = out["type"][t, pos]
            fx = out["loc_fixed"][t, pos].astype(bool)
            ntp = int((ty == TP).sum())
            for v in range(NV):
                fix = v in (2, 7)
                tps = (ty == TP) | (fix & (ty == LOC) & fx)
                fps = ~tps & (ty >= DUP)
                if v == 7:
                    fps = np.zeros_like(fps)
                elif 1 <= v <= 5:
                    fps = fps & (ty != v + 1)                     # the type the variant ignores: 1 DUP .. 5 BG
                npig = ntp if v == 6 else (ntp + int(fx.sum()) if v == 7 else int(out["npos"][k]))
                if npig == 0:
                    continue
                out["prec_fix"][v, t, :, k], out["recall_fix"][v, t, k] = accumulate_one(tps, fps, npig)
    return out


def same(got, want, what=""):
    """Every output of the entry equal: the integers, and the f64 outputs bit for bit."""
    for key in INT_KEYS:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)
    for key in ("ov_same", "ov_other", "prec_fix", "recall_fix"):
        a, b = np.ascontiguousarray(got[key], np.float64), np.ascontiguousarray(want[key], np.float64)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, key)


# ---------------------------------------------------------------------------------------------------------- hand-worked
# Three categories on one image; category 0 and 1 share a group, category 2 is on its own.  Every box is 10 high and starts
# at y = 0, so an IoU is the ratio of two widths.  Ground truth of category 0: A [0, 40 wide], B [100, 40], a crowd box C
# [200, 40], G [500, 40]; category 1: E [300, 40]; category 2: F [400, 40].
_H = lambda x, w: [float(x), 0.0, float(w), 10.0]                # noqa: E731
HAND_GT = [(0, 0, _H(0, 40), 400.0, 0), (0, 0, _H(100, 40), 400.0, 0), (0, 0, _H(200, 40), 400.0, 1),
           (0, 0, _H(500, 40), 400.0, 0), (1, 0, _H(300, 40), 400.0, 0), (2, 0, _H(400, 40), 400.0, 0)]
# category 0's detections by rank (d0 .. d11), then category 1's only one; the file holds them in reverse (lowest first)
HAND_RANKED = [
    (0, 0, _H(0, 40), .95),      # d0  A, IoU 1: TP everywhere
    (0, 0, _H(0, 50), .90),      # d1  A, IoU .8: A is taken -> DUP up to .80, LOC from .85 (A claimed: not fixed)
    (0, 0, _H(100, 64), .85),    # d2  B, IoU .625: TP up to .60; LOC from .65; at .65 - .80 d4, ranked lower, claims B: not fixed
    (0, 0, _H(100, 20), .80),    # d3  B, IoU .5 exactly: DUP at .50 (B taken by d2), LOC above (B claimed: not fixed)
    (0, 0, _H(100, 50), .75),    # d4  B, IoU .8: DUP up to .60, TP at .65 - .80
    (0, 0, _H(200, 40), .70),    # d5  the crowd box: IGN everywhere
    (0, 0, _H(300, 40), .65),    # d6  E of category 1, same group: SIM
    (0, 0, _H(400, 80), .60),    # d7  F of category 2, IoU .5, another group: OTH
    (0, 0, _H(600, 10), .55),    # d8  nothing: BG
    (0, 0, _H(0, 200), .50),     # d9  A, IoU .2: LOC (A claimed: not fixed)
    (0, 0, _H(500, 100), .45),   # d10 G, IoU .4: LOC, nothing claims G: fixed
    (0, 0, _H(500, 160), .40),   # d11 G, IoU .25: LOC, the second on G: not fixed
    (1, 0, _H(300, 40), .90),    # category 1's TP
]
HAND = pack(3, 1, HAND_RANKED[::-1], HAND_GT)
HAND_GROUP = np.array([0, 0, 1], np.int32)
HAND_INDEX = [11 - r for r in range(12)]                          # input index of d0 .. d11; category 1's detection is input 12
HAND_TYPES = {0: [TP, DUP, TP, DUP, DUP, IGN, SIM, OTH, BG, LOC, LOC, LOC],      # IoU 0.50
              5: [TP, DUP, LOC, LOC, TP, IGN, SIM, OTH, BG, LOC, LOC, LOC]}      # IoU 0.75
HAND_FIXED = {0: [10], 5: [10]}                                    # ranks of the fixed rows
HAND_CLAIM = {0: [0, 2, -1, -1], 5: [0, 4, -1, -1]}                 # rank of the detection that claimed A, B, C, G
_F = Fraction
# category 0's AP (the mean of the 101 interpolated precisions) per (threshold index, variant).  npos = 3: 34 recall
# thresholds lie at or below 1/3, 33 more at or below 2/3, 34 above; with npig = 2 it is 51 and 50.
#   IoU .50 plain: TPs at (tp 1, fp 0) and (tp 2, fp 1): (34 * 1 + 33 * 2/3) / 101
#   IoU .75 plain: TPs at (1, 0) and (2, 3):             (34 * 1 + 33 * 2/5) / 101
HAND_AP = {
    (0, 0): (34 + 33 * _F(2, 3)) / 101,
    (0, 1): _F(67, 101),                                          # no DUP rows: both TPs at precision 1
    (0, 2): (34 + 33 * _F(2, 3) + 34 * _F(3, 9)) / 101,           # d10 a TP behind 6 false positives: 3/9; d9, d11 ignored
    (0, 3): (34 + 33 * _F(2, 3)) / 101, (0, 4): (34 + 33 * _F(2, 3)) / 101, (0, 5): (34 + 33 * _F(2, 3)) / 101,
    (0, 6): (51 + 50 * _F(2, 3)) / 101,                           # npig = 2
    (0, 7): _F(1),
    (5, 0): (34 + 33 * _F(2, 5)) / 101,
    (5, 1): (34 + 33 * _F(2, 4)) / 101,                           # d1 gone: d4 at (2, 2)
    (5, 2): (34 + 33 * _F(2, 3) + 34 * _F(3, 7)) / 101,           # d2, d3 ignored: d4 at (2, 1); d10 at (3, 4)
    (5, 3): (34 + 33 * _F(2, 5)) / 101, (5, 4): (34 + 33 * _F(2, 5)) / 101, (5, 5): (34 + 33 * _F(2, 5)) / 101,
    (5, 6): (51 + 50 * _F(2, 5)) / 101,
    (5, 7): _F(1),
}


# ---------------------------------------------------------------------------------------------------------------- cases
def grid_box(j, w=16.0, h=16.0):
    """Box j of a grid of disjoint 16 x 16 cells, 40 apart, 16 to a row."""
    return [40.0 * (j % 16), 40.0 * (j // 16), w, h]


def wave_case(n_own, n_other_before, n_other_after, crowd_at=(), n_det=12):
    """One image, three categories; category 1 is the one under test with n_own boxes, categories 0 and 2 hold the other
    boxes of the image before and behind them in the index.  Detections of category 1 sit on own boxes (exact, and
    shifted by a quarter), on other categories' boxes and far away; crowd_at: positions among the own boxes that are crowd
    boxes, each with two detections on it."""
    gts, dets, j = [], [], 0
    for _ in range(n_other_before):
        gts.append((0, 0, grid_box(j), 256.0, 0)); j += 1
    own0 = j
    for p in range(n_own):
        gts.append((1, 0, grid_box(j), 256.0, 1 if p in crowd_at else 0)); j += 1
    oth0 = j
    for _ in range(n_other_after):
        gts.append((2, 0, grid_box(j), 256.0, 0)); j += 1
    rng = np.random.RandomState(n_own * 1000 + n_other_before * 10 + n_other_after)
    picks = sorted(set([0, n_own - 1, min(62, n_own - 1), min(63, n_own - 1), min(64, n_own - 1)]
                       + rng.randint(0, n_own, n_det).tolist()))
    sc = 0.99
    for p in picks:
        b = grid_box(own0 + p)
        dets.append((1, 0, b, sc)); sc -= 0.004
        dets.append((1, 0, [b[0] + 4.0, b[1], b[2], b[3]], sc)); sc -= 0.004      # IoU 12/20 = .6
        dets.append((1, 0, [b[0] + 8.0, b[1], b[2], b[3]], sc)); sc -= 0.004      # IoU 8/24 = 1/3
    for p in crowd_at:
        dets.append((1, 0, grid_box(own0 + p), 0.995)); dets.append((1, 0, grid_box(own0 + p), 0.5))
    for q in ([0, n_other_before - 1] if n_other_before else []) + ([oth0 + n_other_after - 1] if n_other_after else []):
        b = grid_box(q)                                                           # another category's box: IoU 14/18
        dets.append((1, 0, [b[0] + 2.0, b[1], b[2], b[3]], sc)); sc -= 0.004
    dets.append((1, 0, [9000.0, 9000.0, 5.0, 5.0], sc))
    dets.append((0, 0, grid_box(own0), 0.5)); dets.append((2, 0, grid_box(own0 + n_own - 1), 0.5))
    perm = rng.permutation(len(dets))
    return pack(3, 1, [dets[q] for q in perm], gts)


TIE_PAIRS = [(l, l + 65) for l in range(63)] + [(63, 64)]         # an `a` in every lane; the last pair across the chunk edge


def tie_case(same_class):
    """130 boxes of one image in two (same_class) or three categories.  For every pair (a, b) of TIE_PAIRS a detection
    overlaps boxes a and b -- and nothing else -- with the same IoU: the first must win, in every lane and across the
    chunk edge 63 / 64.  Box j sits at x = 100 j, 20 x 20; box b of a pair is moved below its a, 10 apart."""
    n = 130
    gts, dets = [], []
    for j in range(n):
        gts.append([100.0 * j, 0.0, 20.0, 20.0])
    for a, b in TIE_PAIRS:
        gts[b] = [gts[a][0], 30.0, 20.0, 20.0]
        dets.append([gts[a][0], 10.0, 20.0, 30.0])                                 # 10 rows of each: IoU 200 / 800 both
    if same_class:
        g = [(0, 0, bx, 400.0, 0) for bx in gts]
        d = [(0, 0, bx, 0.9 - 0.01 * q) for q, bx in enumerate(dets)]
        return pack(1, 1, d, g), None
    # detections of category 0; the boxes belong to categories 1 (rows 0 .. 69) and 2 (the rest)
    g = [(1 if j < 70 else 2, 0, bx, 400.0, 0) for j, bx in enumerate(gts)]
    d = [(0, 0, bx, 0.9 - 0.01 * q) for q, bx in enumerate(dets)]
    return pack(3, 1, d, g), np.array([0, 0, 1], np.int32)


def crowd_case():
    """Crowd boxes before, between and past position 63 of a 70-box segment, each met by two detections (both IGN), a
    detection that overlaps a crowd box more than a plain one (arg_same stays the plain box) and crowd boxes of another
    category under a detection (never ov_other)."""
    crowd = (0, 30, 63, 64, 69)
    gts = [(0, 0, grid_box(j), 256.0, 1 if j in crowd else 0) for j in range(70)]
    gts.append((1, 0, grid_box(80), 256.0, 1))
    dets = []
    for q, j in enumerate(crowd):
        dets += [(0, 0, grid_box(j), 0.9 - 0.01 * q), (0, 0, grid_box(j), 0.5 - 0.01 * q)]
    b30, b31 = grid_box(30), grid_box(31)
    dets.append((0, 0, [b30[0] + 2.0, b30[1], 46.0, 16.0], 0.3))                  # crowd 30: 14 of 46 wide; plain 31: IoU 8 / 54
    dets.append((0, 0, grid_box(80), 0.2))                                        # on category 1's crowd box: BG
    dets.append((0, 0, b31, 0.1))
    return pack(2, 1, dets, gts), crowd


def cap_case(n):
    """n detections in one segment, the best-scored last in the file on box 0; box 1's only detection scores lowest."""
    far = [(0, 0, [500.0 + 20 * j, 500.0, 5.0, 5.0], 0.9 - 0.001 * j) for j in range(n - 2)]
    dets = [(0, 0, [50.0, 50.0, 10.0, 10.0], 0.01)] + far + [(0, 0, [0.0, 0.0, 10.0, 10.0], 0.99)]
    return pack(1, 1, dets, [(0, 0, [0.0, 0.0, 10.0, 10.0], 100.0, 0), (0, 0, [50.0, 50.0, 10.0, 10.0], 100.0, 0)])


def bg_edge_case():
    """IoU exactly 0.1: [0, 0, 10, 10] against [0, 0, 10, 100], of the own category and of another."""
    return pack(2, 1, [(0, 0, [0.0, 0.0, 10.0, 10.0], .9), (0, 0, [200.0, 0.0, 10.0, 10.0], .8)],
                [(0, 0, [0.0, 0.0, 10.0, 100.0], 1000.0, 0), (1, 0, [200.0, 0.0, 10.0, 100.0], 1000.0, 0)])


def loc_case():
    """The fix rule: row 0 LOC on box 0, which a lower-ranked TP (row 2) claims: not fixed; rows 3 and 4 LOC on box 1,
    which nothing claims: the first is fixed; row 1 (IoU .6 on box 2) is TP at .50 and LOC, fixed, from .65."""
    return pack(1, 1, [(0, 0, [0.0, 0.0, 40.0, 10.0], .9), (0, 0, [204.0, 0.0, 16.0, 16.0], .8), (0, 0, [0.0, 0.0, 10.0, 10.0], .7),
                       (0, 0, [100.0, 0.0, 30.0, 10.0], .6), (0, 0, [100.0, 0.0, 25.0, 10.0], .5)],
                [(0, 0, [0.0, 0.0, 10.0, 10.0], 100.0, 0), (0, 0, [100.0, 0.0, 10.0, 10.0], 100.0, 0),
                 (0, 0, [200.0, 0.0, 16.0, 16.0], 256.0, 0)])


def class_count_case(K):
    """K categories on 2 images: every category has a box per image at its own grid cell, a TP, a duplicate, a shifted
    row, a row on the next category's box (SIM / OTH), a far row; one category in three has a crowd box with a row on it."""
    gts, dets = [], []
    for k in range(K):
        for i in range(2):
            b, nb = grid_box(k), grid_box((k + 1) % K)
            gts.append((k, i, b, 256.0, 0))
            if k % 3 == 2:
                gts.append((k, i, [b[0], b[1] + 20.0, 16.0, 16.0], 256.0, 1))
                dets.append((k, i, [b[0], b[1] + 20.0, 16.0, 16.0], .65))
            dets += [(k, i, b, .9), (k, i, b, .8), (k, i, [b[0] + 8.0, b[1], 16.0, 16.0], .7), (k, i, [9000.0, 0.0, 4.0, 4.0], .5)]
            if K > 1:
                dets.append((k, i, nb, .6))
    return pack(K, 2, dets, gts)


def many_segments_case(K=4, N=5000):
    """20 000 segments; one image in three has boxes and detections."""
    rng = np.random.RandomState(7)
    gts, dets = [], []
    for i in range(0, N, 3):
        k = int(rng.randint(K))
        b = grid_box(int(rng.randint(32)))
        gts.append((k, i, b, 256.0, int(rng.rand() < 0.1)))
        gts.append(((k + 1) % K, i, grid_box(40), 256.0, 0))
        dets.append((k, i, [b[0] + 4.0 * rng.randint(0, 4), b[1], 16.0, 16.0], float(rng.randint(1, 20)) / 20.0))
        dets.append((k, i, [b[0] + 4.0 * rng.randint(0, 4), b[1], 16.0, 16.0], float(rng.randint(1, 20)) / 20.0))
        dets.append((int(rng.randint(K)), i, grid_box(40 + int(rng.randint(2))), float(rng.randint(1, 20)) / 20.0))
    return pack(K, N, dets, gts)


def sub_image(c, i):
    """Image i of a packed case as a case of its own, with the rows it takes of the detections and the boxes."""
    K, N = c["n_classes"], c["n_images"]
    dr = np.concatenate([np.arange(c["det_off"][k * N + i], c["det_off"][k * N + i + 1]) for k in range(K)]).astype(np.int64)
    gr = np.concatenate([np.arange(c["gt_off"][k * N + i], c["gt_off"][k * N + i + 1]) for k in range(K)]).astype(np.int64)
    doff = np.concatenate([[0], np.cumsum([c["det_off"][k * N + i + 1] - c["det_off"][k * N + i] for k in range(K)])])
    goff = np.concatenate([[0], np.cumsum([c["gt_off"][k * N + i + 1] - c["gt_off"][k * N + i] for k in range(K)])])
    return {"n_classes": K, "n_images": 1, "det_box": c["det_box"][dr], "det_score": c["det_score"][dr], "det_off": doff,
            "gt_box": c["gt_box"][gr], "gt_area": c["gt_area"][gr], "gt_crowd": c["gt_crowd"][gr], "gt_off": goff}, dr, gr
