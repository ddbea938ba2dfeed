"""NumPy restatement of az_diag_eval's contract (include/aznet_hip.h; DESIGN §4, "Proposal diagnosis"), image by image, and
the seeded cases the diagnosis tests share (tests/test_diag_host.py, tests/test_gpu_diag.py, tests/perf_diag.py).  Built from the reference's
arithmetic: train_ref.zoom_labels (bbox_zoom_labels, lib/utils/bbox.pyx:20-60) and the oracle's bbox_overlaps
(bbox.pyx:132-172).

  diag_eval(case, ...)      every output of az_diag_eval for a case
  best_iou_on_set(case)     best IoU from ONE bbox_overlaps call over the whole set (the per-image value must equal it)
  case builders             dicts of per-image lists: anchors [m,4], zoom f32 [m], level i32 [m], gt [k,4], props [n,4]
"""
import numpy as np

import train_ref
from oracle import az_oracle as orc

AZ_MAX_LEVELS = 16
EMB_REG, EMB_OBJ = 0.25, 0.5            # cfg.SEAR.EMB_REG_THRESH / EMB_OBJ_THRESH
CUTS = (10, 50, 100, 300, 1000, 2000)
EDGES = (32 ** 2, 96 ** 2)


def _f64(a):
    return np.asarray(a, dtype=np.float64).reshape(-1, 4)


def make_case(anchors, zoom, level, gt, props):
    n = len(anchors)
    assert len(zoom) == n and len(level) == n and len(gt) == n and len(props) == n
    return {"anchors": [_f64(a) for a in anchors], "zoom": [np.asarray(z, dtype=np.float32).ravel() for z in zoom],
            "level": [np.asarray(l, dtype=np.int32).ravel() for l in level], "gt": [_f64(g) for g in gt],
            "props": [_f64(p) for p in props]}


def sub_case(case, i):
    return {k: [v[i]] for k, v in case.items()}


def holds(anchors, gt, min_obj):
    """[m,k] bool: anchor holds object (bbox.pyx:48-58 without the area-ratio gate)."""
    gt_area = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    iw = np.minimum(anchors[:, None, 2], gt[None, :, 2]) - np.maximum(anchors[:, None, 0], gt[None, :, 0]) + 1
    ih = np.minimum(anchors[:, None, 3], gt[None, :, 3]) - np.maximum(anchors[:, None, 1], gt[None, :, 1]) + 1
    with np.errstate(invalid="ignore"):
        return (iw > 0) & (ih > 0) & (iw * ih / (gt_area[None, :] + 1e-14) >= min_obj)


def diag_eval(case, tz, emb_reg=EMB_REG, emb_obj=EMB_OBJ, iou_thresh=0.5, cuts=CUTS, edges=EDGES):
    cuts = [int(c) for c in cuts]
    level_table = np.zeros((AZ_MAX_LEVELS, 4), np.int64)
    recall_table = np.zeros((len(cuts) + 1, 4), np.int64)
    labels, best_iou, best_rank, first_hit, deepest = [], [], [], [], []
    for a, z, lv, g, p in zip(case["anchors"], case["zoom"], case["level"], case["gt"], case["props"]):
        lab = train_ref.zoom_labels(a, g, emb_reg, emb_obj)
        zoomed = z.astype(np.float64) >= np.where(lv == 0, 0.0, float(tz))
        labels.append(lab.astype(np.uint8))
        for col, m in enumerate((np.ones(lv.shape, bool), zoomed, lab, zoomed & lab)):
            np.add.at(level_table[:, col], lv[m], 1)
        k = g.shape[0]
        if k == 0:
            continue
        if p.shape[0]:
            ov = orc.bbox_overlaps(p, g)                         # [n,k]
            br = ov.argmax(axis=0)                               # the first maximum
            bi = ov[br, np.arange(k)]
            hit = ov >= iou_thresh
            fh = np.where(hit.any(axis=0), hit.argmax(axis=0), -1)
        else:
            bi, br, fh = np.zeros(k), np.full(k, -1), np.full(k, -1)
        if a.shape[0]:
            h = holds(a, g, emb_obj)
            dl = np.where(h, lv[:, None], -1).max(axis=0)
        else:
            dl = np.full(k, -1)
        area = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
        col = np.where(area < edges[0], 1, np.where(area < edges[1], 2, 3))
        for c, cut in enumerate(cuts + [None]):
            m = np.ones(k, bool) if cut is None else (fh >= 0) & (fh < cut)
            recall_table[c, 0] += int(m.sum())
            np.add.at(recall_table[c], col[m], 1)
        best_iou.append(bi); best_rank.append(br); first_hit.append(fh); deepest.append(dl)

    def cat(xs, dt):
        return np.concatenate([np.zeros(0, dt)] + [np.asarray(x, dtype=dt) for x in xs])
    return {"anchor_label": cat(labels, np.uint8), "level_table": level_table, "best_iou": cat(best_iou, np.float64),
            "best_rank": cat(best_rank, np.int32), "first_hit": cat(first_hit, np.int32),
            "deepest_level": cat(deepest, np.int32), "recall_table": recall_table}


def best_iou_on_set(case):
    """Best IoU of every object from one bbox_overlaps call over all proposals and all objects of the set, masked to the
    object's own image."""
    P = np.vstack([np.zeros((0, 4))] + case["props"])
    G = np.vstack([np.zeros((0, 4))] + case["gt"])
    if G.shape[0] == 0:
        return np.zeros(0)
    if P.shape[0] == 0:
        return np.zeros(G.shape[0])
    pi = np.repeat(np.arange(len(case["props"])), [p.shape[0] for p in case["props"]])
    gi = np.repeat(np.arange(len(case["gt"])), [g.shape[0] for g in case["gt"]])
    ov = np.where(pi[:, None] == gi[None, :], orc.bbox_overlaps(P, G), -1.0)
    return np.maximum(ov.max(axis=0), 0.0)


KEYS = ("anchor_label", "level_table", "best_iou", "best_rank", "first_hit", "deepest_level", "recall_table")


def assert_same(got, want, what=""):
    """Integer tables, labels, ranks and levels exactly; best_iou bit for bit."""
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if k == "best_iou":
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (what, k)
        else:
            assert np.array_equal(g, w), (what, k, g, w)


# ------------------------------------------------------------------------------------------------------------- cases
def random_boxes(rng, n, W, H, quarter):
    """n boxes inside W x H from integer (or quarter-pixel) coordinates."""
    step = 4 if quarter else 1
    x1 = rng.randint(0, (W - 8) * step, n) / float(step)
    y1 = rng.randint(0, (H - 8) * step, n) / float(step)
    w = rng.randint(4 * step, W // 2 * step, n) / float(step)
    h = rng.randint(4 * step, H // 2 * step, n) / float(step)
    return np.stack([x1, y1, np.minimum(x1 + w, W - 1.0), np.minimum(y1 + h, H - 1.0)], 1).reshape(-1, 4)


def random_image(rng, m, k, n, W=500, H=375, quarter=False):
    """(anchors, zoom, level, gt, props): a root anchor first (level 0), the rest at levels 1..5 in level-major order;
    some proposals are jittered or exact copies of objects so that IoUs cross the threshold and tie."""
    gt = np.floor(random_boxes(rng, k, W, H, False))
    anchors = random_boxes(rng, m, W, H, quarter)
    level = np.sort(rng.randint(1, 6, m)).astype(np.int32)
    if m:
        anchors[0] = [0, 0, W - 1.0, H - 1.0]
        level[0] = 0
    zoom = rng.uniform(0, 1, m).astype(np.float32)
    props = random_boxes(rng, n, W, H, quarter)
    if n and k:
        j = rng.randint(0, n, min(n, 2 * k))
        props[j] = gt[rng.randint(0, k, j.size)] + rng.randint(-6, 7, (j.size, 4)) / (4.0 if quarter else 1.0)
        if n > 3:
            props[n - 1] = props[1]                               # a duplicate: equal IoUs, the first must win
    return anchors, zoom, level, gt, props


def case_from_counts(counts, seed, quarter=False):
    rng = np.random.RandomState(seed)
    cols = [random_image(rng, m, k, n, quarter=quarter) for m, k, n in counts]
    return make_case(*[[c[j] for c in cols] for j in range(5)])


OFFSET_COUNTS = [(1, 0, 0), (5, 2, 0), (0, 0, 3), (40, 1, 1), (3, 3, 64), (700, 70, 300), (1, 1, 65), (0, 0, 0)]


def offsets_case():
    """Eight images by (anchors, objects, proposals): empty ones first, in the middle and last; one, 64 and 65 proposals."""
    return case_from_counts(OFFSET_COUNTS, 501)


def random_case(n_images=64, seed=777):
    """0-12 objects, 1-900 anchors, 0-400 proposals per image; integer and quarter-pixel coordinates by image."""
    rng = np.random.RandomState(seed)
    cols = []
    for i in range(n_images):
        m, k, n = int(rng.randint(1, 901)), int(rng.randint(0, 13)), int(rng.randint(0, 401))
        cols.append(random_image(rng, m, k, n, quarter=bool(i & 1)))
    return make_case(*[[c[j] for c in cols] for j in range(5)])


WAVE_COUNTS = (1, 63, 64, 65, 127, 128, 129, 300)
WAVE_TIES = ((3, 67), (64, 65), (0, 299))


def wave_case():
    """One object per image against 1 ... 300 proposals (weak ones, IoU < 0.5 with it), then three images of 300 with the
    identical best proposal at two ranks.  Returns (case, expected best_rank per image)."""
    rng = np.random.RandomState(99)
    gt = np.array([[100.0, 80.0, 219.0, 199.0]])
    imgs, want = [], []

    def weak(n):
        # shifted copies: IoU with gt between 0 and ~0.4, all different from the strong proposal's
        d = rng.randint(40, 100, (n, 2)).astype(np.float64)
        return np.hstack((gt[:, :2] + d, gt[:, 2:] + d))
    strong = gt + np.array([[3.0, 2.0, -1.0, 4.0]])
    for n in WAVE_COUNTS:
        p = weak(n)
        r = n - 1 if n % 2 else n // 2
        p[r] = strong
        imgs.append(p); want.append(r)
    for r0, r1 in WAVE_TIES:
        p = weak(300)
        p[r0] = strong; p[r1] = strong
        imgs.append(p); want.append(r0)
    n = len(imgs)
    root = np.array([[0.0, 0.0, 499.0, 374.0]])
    return make_case([root] * n, [np.array([0.5])] * n, [np.array([0])] * n, [gt] * n, imgs), np.array(want, np.int32)


def levels_case():
    """One image, anchors at levels 0 ... AZ_MAX_LEVELS-1 stored deepest FIRST, all holding object 0; object 1 is held by
    the levels 0-2 only (a shallower anchor later in memory than a deeper one); object 2 by none."""
    obj = np.array([[40.0, 40.0, 59.0, 59.0], [200.0, 100.0, 239.0, 139.0], [450.0, 300.0, 469.0, 319.0]])
    anchors, level = [], []
    for l in range(AZ_MAX_LEVELS - 1, -1, -1):
        if l <= 2:
            anchors.append([0.0, 0.0, 300.0 - l, 200.0 - l])      # holds objects 0 and 1
        else:
            anchors.append([30.0 - l, 30.0 - l, 70.0 + l, 70.0 + l])   # holds object 0 only
        level.append(l)
    zoom = np.linspace(0.1, 0.9, AZ_MAX_LEVELS).astype(np.float32)
    props = np.array([[40.0, 40.0, 59.0, 59.0]])
    case = make_case([np.array(anchors)], [zoom], [np.array(level)], [obj], [props])
    return case, np.array([AZ_MAX_LEVELS - 1, 2, -1], np.int32)


TZ_EXACT = float(np.float32(0.3))       # a threshold that IS a float32: zoom == tz happens exactly


def threshold_case():
    """The exact-threshold pairs, one image each; returns (case, notes) where notes name what each image holds.
      0  object [0,0,9,9] against proposal [0,0,9,4]: IoU exactly 0.5
      1  first_hit == cuts[0] - 1 (9) and, second object, == cuts[0] (10)
      2  objects of 32x32 (area 1024: medium), 31x33 (1023: small), 96x96 (9216: large), 95x97 (9215: medium)
      3  anchors: level 1 with zoom == tz, level 1 just below tz, level 0 with zoom below tz (still zoomed)
      4  an anchor covering exactly half of the object (coverage == 0.5 up to the 1e-14), and one whose area is exactly
         4x the object's (area ratio == 0.25 up to the 1e-14)"""
    root = np.array([[0.0, 0.0, 499.0, 374.0]])
    z1, l1 = np.array([0.5], np.float32), np.array([0])
    imgs = []
    imgs.append((root, z1, l1, np.array([[0.0, 0.0, 9.0, 9.0]]), np.array([[0.0, 0.0, 9.0, 4.0]])))
    g = np.array([[100.0, 100.0, 149.0, 149.0], [300.0, 200.0, 349.0, 249.0]])
    far = np.tile(np.array([[0.0, 0.0, 5.0, 5.0]]), (11, 1))
    p = far.copy()
    p[9] = g[0]
    p[10] = g[1]
    imgs.append((root, z1, l1, g, p))
    g = np.array([[10.0, 10.0, 41.0, 41.0], [100.0, 10.0, 130.0, 42.0], [10.0, 100.0, 105.0, 195.0],
                  [200.0, 100.0, 294.0, 196.0]])
    imgs.append((root, z1, l1, g, g[:1].copy()))
    below = np.nextafter(np.float32(TZ_EXACT), np.float32(0))
    a = np.array([[0.0, 0.0, 499.0, 374.0], [0.0, 0.0, 249.0, 187.0], [250.0, 0.0, 499.0, 187.0]])
    imgs.append((a, np.array([0.1, TZ_EXACT, below], np.float32), np.array([0, 1, 1]),
                 np.array([[20.0, 20.0, 99.0, 99.0]]), np.zeros((0, 4))))
    # object 20x20 (area 400); anchor A covers its left half (10 columns: coverage 200/400), area 40x40 = 4 * 400
    g = np.array([[100.0, 100.0, 119.0, 119.0]])
    a = np.array([[70.0, 90.0, 109.0, 129.0], [100.0, 100.0, 139.0, 139.0]])
    imgs.append((a, np.array([0.9, 0.9], np.float32), np.array([1, 2]), g, np.zeros((0, 4))))
    return make_case(*[[im[j] for im in imgs] for j in range(5)])


def perf_case(n_images=4952, n_props=300, seed=4952):
    """A VOC07-test-sized set: 300 proposals per image, anchors and objects drawn as in random_case."""
    rng = np.random.RandomState(seed)
    cols = []
    for i in range(n_images):
        m, k = int(rng.randint(1, 901)), int(rng.randint(0, 13))
        cols.append(random_image(rng, m, k, n_props, quarter=bool(i & 1)))
    return make_case(*[[c[j] for c in cols] for j in range(5)])
