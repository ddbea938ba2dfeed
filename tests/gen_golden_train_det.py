#!/usr/bin/env python3
"""Golden vectors for the detection net's training data layer, produced by the REFERENCE's own lib/roi_data_layer/roidb.py
and minibatch.py, imported from a temp copy of the reference tree made by oracle.gen_golden.build_reference (tabs expanded,
lib2to3; nothing of the reference is copied into the repo).  Recorded in tests/golden/g21_train_det.npz:

  c<i>_{ex,gt,labels}              a single-image case (f32 boxes as the roidb stores them)
  c<i>_{targets,max_overlaps}      _compute_targets on it: [E,5] f32 un-normalised, [E] (f64; f32 without objects)
  set_{means,stds}, c<i>_norm      add_bbox_regression_targets over the cases as one roidb (21 classes)
  syn_*                            prepare_roidb + add_bbox_regression_targets on synthetic_375x500_8 with flips (ground truth
                                   from this project's SyntheticImdb, proposals syn_prop<i> made here from a seed and handed to
                                   the reference as its proposals.pkl)
  mb<k>_*                          four minibatches over it (IMS_PER_BATCH 1 and 2) with their seeds and np.random's state after
Under this NumPy npr.choice rejects the float sizes get_minibatch computes, so _sample_rois is called directly with Python
ints, after the npr.randint call get_minibatch makes first; _get_bbox_regression_labels slices with the float class of the
compact targets, which this NumPy refuses too: it is handed the same table with column 0 as Python ints.

The generator asserts what keeps the reference itself inside the tests' caps: every class that occurs has at least two
distinct positive targets (stds > 0), and there is no nan or inf anywhere.

With --edges it records tests/golden/g22_train_det_edges.npz instead and leaves g21 alone: the cases of
tests/det_edges_ref.py (built there from seeds, so only what the reference answers is stored):

  t<s><i>_{targets,max_overlaps}   _compute_targets on image i of offsets_case under TARGET_SETTINGS[s] (cfg.EPS,
                                   TRAIN.BBOX_THRESH and TRAIN.BG_THRESH_LO set to it), images without example boxes included
  s<K>_{means,stds,norm}           add_bbox_regression_targets over stats_case(K) with K classes: its _compute_targets is
                                   answered with the case's un-normalised targets, so that the reference's own statistics
                                   and normalisation run on rows that no box geometry would give (one row, identical rows,
                                   labels past K).  nan and inf are recorded as the reference gives them.

Run:  python tests/gen_golden_train_det.py [--edges]     (needs the reference tree; not collected by pytest)
"""
import importlib
import os
import pickle
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from oracle import gen_golden as gg          # noqa: E402
import det_train_ref as DR                   # noqa: E402

GOLD = os.path.join(HERE, "golden")
NUM_CLASSES = 21


def state_arrays(prefix, g):
    st = np.random.get_state()
    g[prefix + "_keys"] = np.asarray(st[1], dtype=np.uint32)
    g[prefix + "_pos"] = np.array([st[2], st[3]], dtype=np.int64)
    g[prefix + "_gauss"] = np.array(st[4], dtype=np.float64)


class Dense(object):
    """What the reference reads of a roidb's sparse gt_overlaps."""

    def __init__(self, classes):
        self.a = np.zeros((len(classes), NUM_CLASSES))
        self.a[np.arange(len(classes)), np.asarray(classes, dtype=np.int64)] = 1.0
        self.shape = self.a.shape

    def toarray(self):
        return self.a


class FakeNet(object):
    name = "golden_az_net"


class FakeImdb(object):
    def __init__(self, name, sizes, roidb):
        self.name, self.sizes, self.roidb = name, sizes, roidb
        self.image_index = list(range(len(roidb)))

    def image_path_at(self, i):
        return "fake://%d" % i

    def image_size(self, i):
        return self.sizes[i]


def jitter(rng, box, n, amount, w, h):
    """n copies of a box with its corners moved by up to `amount` of its sides, inside the image."""
    bw, bh = box[2] - box[0], box[3] - box[1]
    d = rng.uniform(-amount, amount, (n, 4)) * np.array([bw, bh, bw, bh])
    out = box[None, :] + d
    out[:, 0::2] = np.clip(out[:, 0::2], 0, w - 1)
    out[:, 1::2] = np.clip(out[:, 1::2], 0, h - 1)
    out = np.stack([np.minimum(out[:, 0], out[:, 2]), np.minimum(out[:, 1], out[:, 3]),
                    np.maximum(out[:, 0], out[:, 2]), np.maximum(out[:, 1], out[:, 3])], 1)
    return np.round(out, 1)


def random_boxes(rng, n, w, h):
    x = np.sort(rng.uniform(0, w - 1, (n, 2)), axis=1)
    y = np.sort(rng.uniform(0, h - 1, (n, 2)), axis=1)
    return np.round(np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1), 1)


def cases():
    """(ex f32 [E,4] with the objects as its last rows, gt f32 [G,4], labels int [G]) per case."""
    rng = np.random.RandomState(21)
    W, H = 500, 375
    out = []

    def add(props, gt, labels):
        gt = np.asarray(gt, np.float32).reshape(-1, 4)
        out.append((np.vstack((np.asarray(props, np.float64).reshape(-1, 4), gt)).astype(np.float32), gt,
                    np.asarray(labels, np.int64)))

    # 0: three objects, near and far boxes
    gt = np.array([[30., 40., 180., 200.], [250., 100., 420., 330.], [100., 220., 200., 300.]])
    add(np.vstack([jitter(rng, b, 12, 0.25, W, H) for b in gt] + [random_boxes(rng, 40, W, H)]), gt, [3, 7, 3])
    # 1: an image without objects
    add(random_boxes(rng, 20, W, H), np.zeros((0, 4)), [])
    # 2: two identical objects of different classes: the FIRST maximum's label
    gt = np.array([[60., 80., 240., 270.], [60., 80., 240., 270.], [300., 50., 460., 150.]])
    add(np.vstack([jitter(rng, b, 10, 0.2, W, H) for b in gt] + [random_boxes(rng, 20, W, H)]), gt, [5, 9, 9])
    # 3: IoU exactly 0.5 (box [0,0,9,9] in object [0,0,9,19]: 100 / 200), just below it, and boxes under one pixel wide
    gt = np.array([[0., 0., 9., 19.], [100.0, 50.0, 100.9, 300.0], [200., 100., 330., 100.5]])
    props = np.array([[0., 0., 9., 9.], [0., 0., 9., 8.9], [0., 1., 9., 19.], [0., 0., 8., 19.],
                      [100.2, 50., 100.6, 300.], [100.0, 60., 100.5, 290.], [100.3, 50., 100.8, 250.],
                      [200., 100.1, 320., 100.4], [210., 100., 330., 100.3], [205., 100.2, 325., 100.5]])
    # (the thin objects share the classes of case 0: alone, their dw or dh would all be log(1 / 1) = 0 and the std 0)
    add(np.vstack([props, random_boxes(rng, 10, W, H)]), gt, [1, 3, 7])
    # 4: many objects of many classes
    gt = np.floor(random_boxes(rng, 12, W, H))
    gt = gt[((gt[:, 2] - gt[:, 0]) > 30) & ((gt[:, 3] - gt[:, 1]) > 30)]
    add(np.vstack([jitter(rng, b, 8, 0.3, W, H) for b in gt] + [random_boxes(rng, 30, W, H)]), gt,
        rng.randint(10, 21, gt.shape[0]))
    return out


def synthetic_proposals(gt_roidb, w, h):
    """A recorded proposals list for the unflipped images: jittered objects and random boxes; image 2 with no box in the
    background band [0.1, 0.5), image 4 with fewer foreground boxes than a batch's quota."""
    rng = np.random.RandomState(22)
    props = []
    for i, e in enumerate(gt_roidb):
        gt = e["boxes"].astype(np.float64)
        near = np.vstack([jitter(rng, b, 10, 0.12, w, h) for b in gt])
        mid = np.vstack([jitter(rng, b, 14, 0.45, w, h) for b in gt])
        far = random_boxes(rng, 110, w, h)
        if i == 2:
            cand = np.vstack((near, far))
            mo = DR.iou_matrix(cand, gt).max(axis=1)
            p = cand[(mo >= 0.5) | (mo < 0.1)]
        elif i == 4:
            cand = np.vstack((mid, far))
            mo = DR.iou_matrix(cand, gt).max(axis=1)
            p = np.vstack((near[:2], cand[mo < 0.5]))
        else:
            p = np.vstack((near, mid, far))
        props.append(p.astype(np.float32))
    return props


class Width(object):
    """What add_bbox_regression_targets reads of gt_overlaps: the number of classes."""

    def __init__(self, num_classes):
        self.shape = (1, num_classes)


def record_edges(R, cfg):
    import det_edges_ref as E
    g = {}
    ex, gt, lab = E.offsets_case()
    keep = (cfg.EPS, cfg.TRAIN.BBOX_THRESH, cfg.TRAIN.BG_THRESH_LO)
    for key in sorted(E.TARGET_SETTINGS):
        s = E.TARGET_SETTINGS[key]
        cfg.EPS, cfg.TRAIN.BBOX_THRESH, cfg.TRAIN.BG_THRESH_LO = s["eps"], s["bbox_thresh"], s["bg_lo"]
        for i in range(len(ex)):
            t, mo = R._compute_targets(ex[i], gt[i], lab[i])
            assert t.dtype == np.float32 and t.shape == (ex[i].shape[0], 5)
            g["t%s%d_targets" % (key, i)], g["t%s%d_max_overlaps" % (key, i)] = t.copy(), np.asarray(mo).copy()
        print("setting %s: positives per image %s" % (key, [int((g["t%s%d_targets" % (key, i)][:, 0] > 0).sum()) for i in range(len(ex))]))
    cfg.EPS, cfg.TRAIN.BBOX_THRESH, cfg.TRAIN.BG_THRESH_LO = keep
    ref_targets = R._compute_targets
    try:
        for K in E.STATS_NCLS:
            ts = E.stats_case(K)
            R._compute_targets = lambda ex_rois, gt_rois, labels: (ts[int(ex_rois[0])].copy(), np.zeros(0))
            roidb = [{"ex_boxes": np.array([i]), "gt_boxes": None, "gt_labels": None, "gt_overlaps": Width(K)} for i in range(len(ts))]
            with np.errstate(all="ignore"):
                means, stds = R.add_bbox_regression_targets(roidb)
            g["s%d_means" % K], g["s%d_stds" % K] = means, stds
            g["s%d_norm" % K] = np.vstack([e["bbox_targets"] for e in roidb])
            assert g["s%d_norm" % K].dtype == np.float32
            print("%d classes, %d images, %d rows: %d nan stds, %d stds below 1e-6" % (K, len(ts), g["s%d_norm" % K].shape[0],
                  int(np.isnan(stds).sum()), int((stds < 1e-6).sum())))
    finally:
        R._compute_targets = ref_targets
    path = os.path.join(GOLD, "g22_train_det_edges.npz")
    np.savez_compressed(path, **g)
    print("wrote %s: %d KB" % (path, os.path.getsize(path) // 1024))


def main(edges=False):
    tmp = tempfile.mkdtemp(prefix="azref_")
    try:
        _, _, _, T, C = gg.build_reference(tmp)
        lib = os.path.join(tmp, "py", "lib")
        files = [os.path.join(lib, "roi_data_layer", f) for f in ("roidb.py", "minibatch.py")]
        for f in files:
            src = open(f).read().expandtabs(8)
            src = re.sub(r"\)\s*/\s*2\b", ")//2", src)          # (Python 2's integer division of a len() by two)
            open(f, "w").write(src)
        subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n"] + files,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        open(os.path.join(lib, "roi_data_layer", "__init__.py"), "w").close()
        if not hasattr(np, "float"):
            np.float = float                      # (the reference's astype(np.float))
        R = importlib.import_module("roi_data_layer.roidb")
        M = importlib.import_module("roi_data_layer.minibatch")
        from utils.blob import prep_im_for_blob
        assert R.__file__.startswith(tmp) and M.__file__.startswith(tmp)
        cfg = C.cfg
        assert cfg.EPS == 1e-14 and cfg.TRAIN.BBOX_THRESH == cfg.TRAIN.FG_THRESH == cfg.TRAIN.BG_THRESH_HI == 0.5
        assert cfg.TRAIN.BG_THRESH_LO == 0.1 and cfg.TRAIN.BATCH_SIZE == 128 and cfg.TRAIN.FG_FRACTION == 0.25
        if edges:
            return record_edges(R, cfg)
        g = {}

        def check_stats(roidb, stds, what):
            seen = set()
            for e in roidb:
                t = e["bbox_targets"]
                assert np.all(np.isfinite(t)) and np.all(np.isfinite(e["max_overlaps"])), what
                seen |= set(int(c) for c in t[:, 0] if c > 0)
            stds = np.asarray(stds).reshape(-1, 4)
            for c in seen:
                assert np.all(stds[c] > 0), "%s: class %d has std 0" % (what, c)
            return sorted(seen)

        # ---- single-image cases ------------------------------------------------------------------------------------
        cs = cases()
        roidb = []
        for i, (ex, gt, labels) in enumerate(cs):
            t, mo = R._compute_targets(ex, gt, labels)
            g["c%d_ex" % i], g["c%d_gt" % i], g["c%d_labels" % i] = ex, gt, labels
            g["c%d_targets" % i], g["c%d_max_overlaps" % i] = t.copy(), mo.copy()
            assert t.dtype == np.float32
            roidb.append({"ex_boxes": ex, "gt_boxes": gt, "gt_labels": labels, "gt_overlaps": Dense(labels)})
            print("case %d: E=%d G=%d positives=%d  max_overlaps %s" % (i, ex.shape[0], gt.shape[0], int((t[:, 0] > 0).sum()), mo.dtype))
        mo3 = g["c3_max_overlaps"]
        assert mo3[0] == 0.5 and g["c3_targets"][0, 0] == 1 and mo3[1] < 0.5 and g["c3_targets"][1, 0] == 0
        w3 = (g["c3_ex"][:, 2] - g["c3_ex"][:, 0])[g["c3_targets"][:, 0] == 3]
        assert w3.size >= 2 and np.all(w3 < 1), "no positive under one pixel wide"
        tie = DR.iou_matrix(g["c2_ex"], g["c2_gt"])
        pos2 = g["c2_targets"][:, 0] > 0
        assert set(g["c2_targets"][(tie[:, 0] == tie.max(axis=1)) & pos2, 0].tolist()) == {5.0}, "the first maximum's label"
        means, stds = R.add_bbox_regression_targets(roidb)
        g["set_means"], g["set_stds"] = means, stds
        for i, e in enumerate(roidb):
            g["c%d_norm" % i] = e["bbox_targets"].copy()
        g["n_cases"] = np.array(len(cs))
        print("classes of the cases:", check_stats(roidb, stds, "cases"))

        # ---- synthetic_375x500_8 with flips --------------------------------------------------------------------------
        sys.path.insert(0, os.path.join(REPO, "az-net_amd", "lib"))
        for m in [k for k in sys.modules if k == "datasets" or k.startswith("datasets.")]:
            del sys.modules[m]
        keep = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "detect" or k.startswith("detect.")}
        from datasets.synthetic import SyntheticImdb
        ours = SyntheticImdb(375, 500, 8)
        props = synthetic_proposals(ours.gt_roidb(), 500, 375)
        ours.append_flipped_images()
        sys.modules.update(keep)
        sroidb = [{"boxes": e["boxes"], "gt_overlaps": Dense(e["gt_classes"]), "flipped": e["flipped"]} for e in ours.roidb]
        fake = FakeImdb(ours.name, [(375, 500)] * len(sroidb), sroidb)
        cfg.ROOT_DIR, cfg.EXP_DIR = tmp, "golden"
        out_dir = C.get_output_dir(fake, FakeNet())
        os.makedirs(out_dir)
        with open(os.path.join(out_dir, "proposals.pkl"), "wb") as f:
            pickle.dump([p.copy() for p in props], f, pickle.HIGHEST_PROTOCOL)
        assert cfg.TRAIN.USE_FLIPPED
        R.prepare_roidb(fake, {"full": FakeNet()})
        smeans, sstds = R.add_bbox_regression_targets(sroidb)
        g["syn_means"], g["syn_stds"] = smeans, sstds
        g["syn_n"] = np.array(len(sroidb))
        for i, p in enumerate(props):
            g["syn_prop%d" % i] = p
        for i, e in enumerate(sroidb):
            g["syn%d_flipped" % i] = np.array(e["flipped"])
            g["syn%d_ex_boxes" % i] = e["ex_boxes"]
            g["syn%d_gt_boxes" % i] = e["gt_boxes"]
            g["syn%d_gt_labels" % i] = np.asarray(e["gt_labels"], dtype=np.int64)
            g["syn%d_bbox_targets" % i] = e["bbox_targets"]
            g["syn%d_max_overlaps" % i] = e["max_overlaps"]
            assert e["ex_boxes"].dtype == np.float32 and e["gt_boxes"].dtype == np.float32 and e["bbox_targets"].dtype == np.float32
        print("classes of the synthetic set:", check_stats(sroidb, sstds, "synthetic"))
        mo2, mo4 = sroidb[2]["max_overlaps"], sroidb[4]["max_overlaps"]
        assert not np.any((mo2 >= 0.1) & (mo2 < 0.5)) and np.any(mo2 < 0.1), "image 2 must have an empty background band"
        assert 0 < int((mo4 >= 0.5).sum()) < 16, "image 4 must have fewer foreground boxes than any quota"

        # ---- minibatches: what get_minibatch computes for these entries ------------------------------------------------
        _, im_scale = prep_im_for_blob(np.zeros((375, 500, 3), dtype=np.float32), cfg.PIXEL_MEANS, cfg.TRAIN.SCALES[0],
                                       cfg.TRAIN.MAX_SIZE)
        g["mb_im_scale"] = np.array(im_scale)
        ref_labels = M._get_bbox_regression_labels

        def with_int_classes(data, num_classes):
            t = np.asarray(data).astype(object)
            for r in range(t.shape[0]):
                t[r, 0] = int(t[r, 0])
            return ref_labels(t, num_classes)
        M._get_bbox_regression_labels = with_int_classes
        batches = [((2,), 31), ((4, 11), 32), ((12,), 33), ((7, 10), 34)]      # (2: fallback pool; 4 and 12 = 4 flipped: few fg)
        for b, (inds, seed) in enumerate(batches):
            np.random.seed(seed)
            np.random.randint(0, high=len(cfg.TRAIN.SCALES), size=len(inds))
            per = cfg.TRAIN.BATCH_SIZE // len(inds)
            fg = int(np.round(cfg.TRAIN.FG_FRACTION * per))
            rois, labs, tg, lw = [], [], [], []
            for j, i in enumerate(inds):
                l, _, r, t, w = M._sample_rois(sroidb[i], fg, per, NUM_CLASSES)
                r = M._project_im_rois(r, im_scale)
                rois.append(np.hstack((j * np.ones((r.shape[0], 1)), r)))
                labs.append(l), tg.append(t), lw.append(w)
            g["mb%d_inds" % b], g["mb%d_seed" % b] = np.array(inds), np.array(seed)
            g["mb%d_rois" % b] = np.vstack(rois).astype(np.float32)
            g["mb%d_labels" % b] = np.hstack(labs).astype(np.float32)
            g["mb%d_bbox_targets" % b] = np.vstack(tg).astype(np.float32)
            g["mb%d_bbox_loss_weights" % b] = np.vstack(lw).astype(np.float32)
            state_arrays("mb%d_state" % b, g)
            for k in ("rois", "labels", "bbox_targets", "bbox_loss_weights"):
                assert np.all(np.isfinite(g["mb%d_%s" % (b, k)]))
            print("batch %d: images %s, %d rows, %d foreground" % (b, inds, g["mb%d_rois" % b].shape[0], int((g["mb%d_labels" % b] > 0).sum())))
        g["n_batches"] = np.array(len(batches))
        path = os.path.join(GOLD, "g21_train_det.npz")
        np.savez_compressed(path, **g)
        print("wrote %s: %d KB" % (path, os.path.getsize(path) // 1024))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(edges="--edges" in sys.argv[1:])
