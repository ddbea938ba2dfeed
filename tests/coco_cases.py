"""COCO box evaluation inputs shared by the CPU and GPU tests: hand cases (expected numbers worked out in
test_coco_host.py) and seeded random sets, all in az_coco_eval's class-major (category, image) segments."""
import numpy as np


def pack(K, N, dets, gts):
    """dets: (k, i, [x, y, w, h], score); gts: (k, i, [x, y, w, h], area, iscrowd); file order kept per segment."""
    def order(rows):
        seg = np.array([r[0] * N + r[1] for r in rows], np.int64)
        o = np.argsort(seg, kind="stable")
        off = np.zeros(K * N + 1, np.int64)
        off[1:] = np.cumsum(np.bincount(seg, minlength=K * N)) if len(rows) else 0
        return o, off
    do, doff = order(dets)
    go, goff = order(gts)
    return {"n_classes": K, "n_images": N,
            "det_box": np.array([dets[j][2] for j in do], np.float64).reshape(-1, 4),
            "det_score": np.array([dets[j][3] for j in do], np.float64), "det_off": doff,
            "gt_box": np.array([gts[j][2] for j in go], np.float64).reshape(-1, 4),
            "gt_area": np.array([gts[j][3] for j in go], np.float64),
            "gt_crowd": np.array([gts[j][4] for j in go], np.uint8), "gt_off": goff}


def _far(n, score0):
    return [(0, 0, [500.0 + 20 * j, 500.0, 5.0, 5.0], score0 - 0.001 * j) for j in range(n)]


CASES = {
    # IoU exactly 0.75 (det a) and exactly 0.5 (det b, the box already taken)
    "iou_edges": pack(1, 1, [(0, 0, [0, 0, 40, 10], .9), (0, 0, [0, 0, 60, 10], .8)],
                      [(0, 0, [0, 0, 30, 10], 300.0, 0)]),
    # one crowd box matched by two detections (both ignored), then a plain TP
    "crowd_twice": pack(1, 1, [(0, 0, [0, 0, 10, 10], .9), (0, 0, [0, 0, 10, 10], .8), (0, 0, [50, 50, 10, 10], .7)],
                        [(0, 0, [0, 0, 10, 10], 100.0, 1), (0, 0, [50, 50, 10, 10], 100.0, 0)]),
    # an ignored (crowd) box first in the file with the higher IoU: the plain box wins up to 0.8, the crowd box after
    "ignored_first": pack(1, 1, [(0, 0, [0, 0, 12, 10], .9)],
                          [(0, 0, [0, 0, 20, 10], 200.0, 1), (0, 0, [0, 0, 10, 10], 100.0, 0)]),
    # areas exactly 32^2 and 96^2: in both neighbouring ranges
    "area_edges": pack(1, 1, [(0, 0, [0, 0, 32, 32], .9), (0, 0, [100, 0, 96, 96], .8)],
                       [(0, 0, [0, 0, 32, 32], 1024.0, 0), (0, 0, [100, 0, 96, 96], 9216.0, 0)]),
    # 120 detections on one (image, category): the best-scored is the 111th in the file; the only one on the second
    # box scores lowest and falls past the first 100
    "over_100": pack(1, 1, _far(110, .5) + [(0, 0, [0, 0, 10, 10], .99)] + _far(8, .3)
                     + [(0, 0, [50, 50, 10, 10], .01)],
                     [(0, 0, [0, 0, 10, 10], 100.0, 0), (0, 0, [50, 50, 10, 10], 100.0, 0)]),
    # equal scores on two images: image order decides (the FP of image 0 ranks first)
    "tie_images": pack(1, 2, [(0, 0, [200, 200, 10, 10], .5), (0, 1, [0, 0, 10, 10], .5)],
                       [(0, 0, [0, 0, 10, 10], 100.0, 0), (0, 1, [0, 0, 10, 10], 100.0, 0)]),
    # category 1 has detections but no ground truth: -1 and left out of the means
    "no_gt_class": pack(2, 1, [(0, 0, [0, 0, 10, 10], .9), (1, 0, [0, 0, 10, 10], .8)],
                        [(0, 0, [0, 0, 10, 10], 100.0, 0)]),
    # detections on an image without ground truth are false positives
    "dets_no_gt_image": pack(1, 2, [(0, 0, [0, 0, 10, 10], .9), (0, 1, [0, 0, 10, 10], .95)],
                             [(0, 0, [0, 0, 10, 10], 100.0, 0)]),
    # rc = 0.5 exactly on recThrs[50]: searchsorted 'left' lands on the first TP
    "rc_on_threshold": pack(1, 1, [(0, 0, [0, 0, 10, 10], .9), (0, 0, [300, 300, 10, 10], .8),
                                   (0, 0, [100, 100, 10, 10], .7)],
                            [(0, 0, [0, 0, 10, 10], 100.0, 0), (0, 0, [100, 100, 10, 10], 100.0, 0)]),
}


def random_set(seed, K=None, N=None):
    """Boxes on a coarse grid (so IoU ties and exact thresholds occur), quantised scores (ties), crowd boxes, areas on
    the range edges, empty segments and now and then more than 100 detections in one segment."""
    rng = np.random.RandomState(seed)
    K = K or int(rng.randint(1, 5))
    N = N or int(rng.randint(1, 7))
    dets, gts = [], []
    for k in range(K):
        for i in range(N):
            ng = int(rng.choice([0, 0, 1, 2, 3, 5, 8, 70]))
            boxes = []
            for _ in range(ng):
                b = [float(rng.randint(0, 20) * 4), float(rng.randint(0, 20) * 4), float(rng.choice([8, 16, 32, 40, 96, 120])),
                     float(rng.choice([8, 16, 32, 48, 96, 120]))]
                area = rng.choice([b[2] * b[3], 1024.0, 9216.0, b[2] * b[3] * 0.7])
                gts.append((k, i, b, float(area), int(rng.rand() < 0.15)))
                boxes.append(b)
            nd = int(rng.choice([0, 1, 2, 4, 10, 30, 105])) if rng.rand() < 0.9 else 0
            for _ in range(nd):
                if boxes and rng.rand() < 0.6:
                    g = boxes[rng.randint(len(boxes))]
                    b = [g[0] + 4 * rng.randint(-2, 3), g[1] + 4 * rng.randint(-2, 3), max(4.0, g[2] + 4 * rng.randint(-3, 4)),
                         max(4.0, g[3] + 4 * rng.randint(-3, 4))]
                else:
                    b = [float(rng.randint(0, 30) * 4), float(rng.randint(0, 30) * 4), float(rng.choice([4, 8, 32, 64])),
                         float(rng.choice([4, 8, 32, 64]))]
                dets.append((k, i, [float(v) for v in b], float(rng.randint(0, 20)) / 20.0))
    perm = rng.permutation(len(dets))                    # the file's interleaving of segments
    return pack(K, N, [dets[j] for j in perm], gts)


def big_set(seed=18, N=40504, K=80):
    """val2014-sized: N images, K categories, up to 100 detections per image over all categories (vectorised)."""
    rng = np.random.RandomState(seed)
    ng = rng.poisson(7.3, N).clip(0, 60)
    g_img = np.repeat(np.arange(N), ng)
    G = g_img.size
    g_cat = rng.randint(0, K, G)
    gxy = rng.uniform(0, 500, (G, 2))
    gwh = rng.uniform(4, 300, (G, 2))
    g_box = np.hstack([gxy, gwh])
    g_area = gwh[:, 0] * gwh[:, 1] * rng.uniform(0.5, 1.0, G)
    g_crowd = (rng.rand(G) < 0.01).astype(np.uint8)
    nd = rng.randint(20, 101, N)
    d_img = np.repeat(np.arange(N), nd)
    Dn = d_img.size
    d_cat = rng.randint(0, K, Dn)
    d_box = np.hstack([rng.uniform(0, 500, (Dn, 2)), rng.uniform(4, 300, (Dn, 2))])
    # a third of the detections sit near a ground-truth box of their image
    gstart = np.concatenate([[0], np.cumsum(ng)])
    has = ng[d_img] > 0
    pick = np.nonzero(has & (rng.rand(Dn) < 0.33))[0]
    src = gstart[d_img[pick]] + (rng.rand(pick.size) * ng[d_img[pick]]).astype(np.int64)
    d_box[pick] = g_box[src] + rng.normal(0, 6, (pick.size, 4))
    d_box[pick, 2:] = np.maximum(d_box[pick, 2:], 1.0)
    d_cat[pick] = g_cat[src]
    d_box = np.floor(d_box * 100) / 100
    d_score = np.round(rng.rand(Dn), 3)

    def order(cat, img):
        seg = cat.astype(np.int64) * N + img
        o = np.argsort(seg, kind="stable")
        off = np.zeros(K * N + 1, np.int64)
        off[1:] = np.cumsum(np.bincount(seg, minlength=K * N))
        return o, off
    do, doff = order(d_cat, d_img)
    go, goff = order(g_cat, g_img)
    return {"n_classes": K, "n_images": N, "det_box": d_box[do], "det_score": d_score[do], "det_off": doff,
            "gt_box": g_box[go], "gt_area": g_area[go], "gt_crowd": g_crowd[go], "gt_off": goff}


# the 80 category ids of COCO's instances files (1..90 with gaps)
COCO_CAT_IDS = [i for i in range(1, 91) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]


def fabricate_annotations(seed=18, n_images=7, with_annotations=True):
    """A small instances_*.json as a dict: image ids out of order, boxes overhanging the border, fractional and
    zero-size boxes, crowd boxes, area fields unlike w*h."""
    rng = np.random.RandomState(seed)
    ids = [int(v) for v in rng.choice(np.arange(1, 600), n_images, replace=False)]
    images = [{"id": i, "file_name": "COCO_val2014_%012d.jpg" % i, "width": int(rng.randint(40, 640)),
               "height": int(rng.randint(40, 480))} for i in ids]
    cats = [{"id": c, "name": "c%d" % c, "supercategory": "s"} for c in COCO_CAT_IDS]
    anns, aid = [], 1
    for im in images:
        for _ in range(int(rng.randint(0, 6))):
            W, H = im["width"], im["height"]
            x = float(np.round(rng.uniform(-20, W), 2))
            y = float(np.round(rng.uniform(-20, H), 2))
            w = float(np.round(rng.choice([0.0, rng.uniform(1, 40), rng.uniform(40, 400)]), 2))
            h = float(np.round(rng.uniform(0.5, 300), 2))
            anns.append({"id": aid, "image_id": im["id"], "category_id": int(rng.choice(COCO_CAT_IDS[:12])),
                         "bbox": [x, y, w, h], "area": float(np.round(w * h * rng.uniform(0.4, 1.0), 3)),
                         "iscrowd": int(rng.rand() < 0.15)})
            aid += 1
    anns = [anns[j] for j in rng.permutation(len(anns))]     # annotations of an image interleaved with others'
    d = {"images": images, "categories": cats}
    if with_annotations:
        d["annotations"] = anns
    return d


def make_devkit(root, val=None):
    """<root>/annotations/{instances_train2014, instances_val2014, image_info_test2014, image_info_test-dev2015}.json
    and <root>/images/<file_name> (empty files).  Returns root as a string."""
    import json
    import os
    root = str(root)
    os.makedirs(os.path.join(root, "annotations"))
    os.makedirs(os.path.join(root, "images"))
    sets = {"instances_val2014": val or fabricate_annotations(18), "instances_train2014": fabricate_annotations(19, 4),
            "image_info_test2014": fabricate_annotations(20, 3, False),
            "image_info_test-dev2015": fabricate_annotations(21, 3, False)}
    for name, d in sets.items():
        with open(os.path.join(root, "annotations", name + ".json"), "w") as f:
            json.dump(d, f)
        for im in d["images"]:
            open(os.path.join(root, "images", im["file_name"]), "wb").close()
    return root
