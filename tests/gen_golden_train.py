#!/usr/bin/env python3
"""Golden vectors for the training data layer, produced by the REFERENCE's own lib/az_data_layer/roidb.py and
minibatch.py, imported from a temp copy of the reference tree made by oracle.gen_golden.build_reference (tabs expanded,
lib2to3; nothing of the reference is copied into the repo).  Recorded in tests/golden/g20_train_roidb.npz:

  c<i>_{size,gt,seed}            a single-image case
  c<i>_{ex_boxes,zoom_gt,used}   _compute_ex_rois after np.random.seed(seed): boxes f64 (before the roidb's f32 cast),
                                 labels, uniform doubles drawn
  c<i>_zoom_of_ex                _compute_zoom_labels(ex_boxes, gt): the unit entry's case (zoom_gt is of the boxes
                                 before clipping)
  c<i>_targets                   _compute_targets on the f32 boxes, un-normalised [T,7] f64
  set_{means,stds}, c<i>_ntargets   add_adjacent_prediction_targets over the cases as one imdb
  syn_*                          prepare_roidb + add_adjacent_prediction_targets on synthetic_375x500_8 with flips after
                                 np.random.seed(3) (ground truth from this project's SyntheticImdb), the np.random state
                                 afterwards, and minibatches sampled from it (SCALE_ADJ_CONF off and on)
Under this NumPy npr.choice rejects the float sizes get_minibatch computes, so _sample_rois is called directly with
integers, after the npr.randint call get_minibatch makes first; _get_adjacent_targets indexes with the floats of the
compact targets, which this NumPy refuses too: it is handed the table with its two index columns as Python ints.

Run:  python tests/gen_golden_train.py     (needs the reference tree; not collected by pytest)
"""
import importlib
import os
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
import train_ref                             # noqa: E402

GOLD = os.path.join(HERE, "golden")


class CountingRandom(object):
    """numpy.random with `random` counting the doubles drawn."""

    def __init__(self):
        self.used = 0

    def random(self, size=None):
        self.used += int(size)
        return np.random.random(size=size)

    def __getattr__(self, k):
        return getattr(np.random, k)


class Ones(object):
    def __init__(self, k):
        self.k = k

    def toarray(self):
        return np.ones((self.k, 1))


class FakeImdb(object):
    def __init__(self, name, sizes, roidb, cache):
        self.name, self.sizes, self.roidb, self.cache_path = name, sizes, roidb, cache
        self.image_index = list(range(len(roidb)))

    def image_path_at(self, i):
        return "fake://%d" % i

    def image_size(self, i):
        return self.sizes[i]


def state_arrays(prefix, g):
    st = np.random.get_state()
    g[prefix + "_keys"] = np.asarray(st[1], dtype=np.uint32)
    g[prefix + "_pos"] = np.array([st[2], st[3]], dtype=np.int64)
    g[prefix + "_gauss"] = np.array(st[4], dtype=np.float64)


def cases():
    rng = np.random.RandomState(20)

    def rand_gt(h, w, k, lo=0.08, hi=0.5):
        bw = rng.uniform(lo, hi, k) * w
        bh = rng.uniform(lo, hi, k) * h
        x1 = rng.uniform(0, w - 1 - bw)
        y1 = rng.uniform(0, h - 1 - bh)
        return np.floor(np.stack([x1, y1, x1 + bw, y1 + bh], 1))

    out = [((375, 500), rand_gt(375, 500, 3), 1), ((500, 375), rand_gt(500, 375, 3), 2),
           ((600, 1000), rand_gt(600, 1000, 4), 3),
           ((375, 500), np.zeros((0, 4)), 4),                                           # no objects
           ((375, 500), np.array([[20., 30., 420., 330.], [300., 200., 340., 260.]]), 5),  # > a quarter: never embedded
           # two identical objects; one centred in the whole-image region so that mirrored sub-regions tie
           ((375, 500), np.array([[60., 80., 140., 170.], [60., 80., 140., 170.], [150., 87., 349., 287.]]), 6),
           ((375, 500), np.array([[100., 50., 103., 250.], [0., 300., 200., 304.], [496., 10., 499., 60.]]), 7),  # thin
           ((375, 500), np.tile(np.array([[0., 0., np.floor(0.25 * 499), np.floor(0.5 * 374)]]), (10, 1)), 8),   # IoU 0 matches
           ((600, 800), rand_gt(600, 800, 14, 0.04, 0.3), 9),
           # 13 jittered copies of one object: all adjacent to the regions around it, so min(11, .) binds
           ((375, 500), np.array([[100., 80., 300., 260.]]) + np.round(rng.uniform(-6, 6, (13, 4))), 10)]
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="azref_")
    try:
        _, _, _, T, C = gg.build_reference(tmp)
        lib = os.path.join(tmp, "py", "lib")
        files = [os.path.join(lib, "az_data_layer", f) for f in ("roidb.py", "minibatch.py")]
        for f in files:
            src = open(f).read().expandtabs(8)
            open(f, "w").write(src)
        subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n"] + files,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        open(os.path.join(lib, "az_data_layer", "__init__.py"), "w").close()
        R = importlib.import_module("az_data_layer.roidb")
        M = importlib.import_module("az_data_layer.minibatch")
        from utils.blob import prep_im_for_blob
        assert R.__file__.startswith(tmp) and M.__file__.startswith(tmp)
        cfg = C.cfg
        cfg.TRAIN.USE_CACHE = False
        c = train_ref.TrainCfg()
        g = {}
        cs = cases()
        roidb, trace = [], {}
        for i, (size, gt, seed) in enumerate(cs):
            cnt = CountingRandom()
            R.npr = cnt
            np.random.seed(seed)
            ex, zl = R._compute_ex_rois(size, gt)
            R.npr = np.random
            ex32, gt32 = ex.astype(np.float32), gt.astype(np.float32)
            t = np.asarray(R._compute_targets(gt32, ex32), dtype=np.float64).reshape(-1, 7)
            train_ref.compute_targets(gt32, ex32, c, trace)
            g["c%d_size" % i] = np.array(size)
            g["c%d_gt" % i] = gt
            g["c%d_seed" % i] = np.array(seed)
            g["c%d_ex_boxes" % i] = ex
            g["c%d_zoom_gt" % i] = zl.astype(bool)
            g["c%d_used" % i] = np.array(cnt.used)
            g["c%d_zoom_of_ex" % i] = np.asarray(R._compute_zoom_labels(ex, gt), dtype=bool)   # labels of the CLIPPED boxes
            g["c%d_targets" % i] = t
            g["c%d_ntargets" % i] = np.array(t.shape[0])
            roidb.append({"zoom_gt": zl.astype(bool), "ex_boxes": ex32, "gt_boxes": gt32})
            print("case %d: %s N=%d E=%d zoom=%d used=%d T=%d" % (i, size, gt.shape[0], ex.shape[0], int(zl.sum()),
                                                                  cnt.used, t.shape[0]))
        assert trace.get("zero_rounds", 0) >= 1 and trace.get("ties", 0) >= 1 and trace.get("bound", 0) >= 1, trace
        print("rounds won at overlap 0: %d; rounds with a tied maximum: %d; regions with more than 11 adjacent objects: %d"
              % (trace["zero_rounds"], trace["ties"], trace["bound"]))
        fake = FakeImdb("cases", [s for s, _, _ in cs], roidb, tmp)
        means, stds = R.add_adjacent_prediction_targets(fake)
        g["set_means"], g["set_stds"] = means, stds
        g["set_targets"] = np.vstack([np.asarray(e["bbox_targets"], dtype=np.float64).reshape(-1, 7) for e in roidb])
        g["n_cases"] = np.array(len(cs))

        # ---- synthetic_375x500_8 with flips, seed 3 ------------------------------------------------
        sys.path.insert(0, os.path.join(REPO, "az-net_amd", "lib"))
        for m in [k for k in sys.modules if k == "datasets" or k.startswith("datasets.")]:
            del sys.modules[m]
        keep = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "detect" or k.startswith("detect.")}
        from datasets.synthetic import SyntheticImdb
        ours = SyntheticImdb(375, 500, 8)
        ours.append_flipped_images()
        sys.modules.update(keep)
        sroidb = [{"boxes": e["boxes"], "gt_overlaps": Ones(e["boxes"].shape[0]), "flipped": e["flipped"]}
                  for e in ours.roidb]
        fake = FakeImdb(ours.name, [(375, 500)] * len(sroidb), sroidb, tmp)
        np.random.seed(3)
        R.prepare_roidb(fake)
        state_arrays("syn_state", g)
        smeans, sstds = R.add_adjacent_prediction_targets(fake)
        g["syn_means"], g["syn_stds"] = smeans, sstds
        g["syn_n"] = np.array(len(sroidb))
        for i, e in enumerate(sroidb):
            g["syn%d_boxes" % i] = e["boxes"]
            g["syn%d_flipped" % i] = np.array(e["flipped"])
            g["syn%d_ex_boxes" % i] = e["ex_boxes"]
            g["syn%d_zoom_gt" % i] = e["zoom_gt"]
            g["syn%d_gt_boxes" % i] = e["gt_boxes"]
            g["syn%d_bbox_targets" % i] = np.asarray(e["bbox_targets"], dtype=np.float64).reshape(-1, 7)
            assert e["ex_boxes"].dtype == np.float32 and e["zoom_gt"].dtype == bool and e["gt_boxes"].dtype == np.float32
        # minibatches: what get_minibatch computes for these entries (BATCH_SIZE 128, AZ_POS_FRACTION 0.5)
        _, im_scale = prep_im_for_blob(np.zeros((375, 500, 3), dtype=np.float32), cfg.PIXEL_MEANS, cfg.TRAIN.SCALES[0],
                                       cfg.TRAIN.MAX_SIZE)
        g["mb_im_scale"] = np.array(im_scale)
        # (this NumPy refuses the float region indices _get_adjacent_targets reads from the compact targets: it is handed
        #  the same table with columns 4-5 as Python ints, and runs unchanged)
        ref_gat = M._get_adjacent_targets

        def gat(compact, keep_inds, num_regions, num_classes):
            t = np.asarray(compact, dtype=np.float64).astype(object)
            for r in range(t.shape[0]):
                t[r, 4], t[r, 5] = int(t[r, 4]), int(t[r, 5])
            return ref_gat(t, keep_inds, num_regions, num_classes)
        M._get_adjacent_targets = gat
        batches = [((0, 9), False, 11), ((3, 12), True, 12), ((5,), False, 13), ((15, 2), True, 14)]
        for b, (inds, conf, seed) in enumerate(batches):
            cfg.SEAR.SCALE_ADJ_CONF = conf
            np.random.seed(seed)
            np.random.randint(0, high=len(cfg.TRAIN.SCALES), size=len(inds))
            per = cfg.TRAIN.BATCH_SIZE // len(inds)
            fg = int(np.round(cfg.TRAIN.AZ_POS_FRACTION * per))
            rois_blob, labs, tg, lw, zl = [], [], [], [], []
            for j, i in enumerate(inds):
                a, z, r, t, w = M._sample_rois(sroidb[i], fg, per)
                r = M._project_im_rois(r, im_scale)
                rois_blob.append(np.hstack((j * np.ones((r.shape[0], 1)), r)))
                labs.append(a), tg.append(t), lw.append(w), zl.append(z)
            g["mb%d_inds" % b] = np.array(inds)
            g["mb%d_conf" % b] = np.array(conf)
            g["mb%d_seed" % b] = np.array(seed)
            g["mb%d_rois" % b] = np.vstack(rois_blob).astype(np.float32)
            g["mb%d_adj_labels" % b] = np.vstack(labs).astype(np.float32)
            g["mb%d_adj_targets" % b] = np.vstack(tg).astype(np.float32)
            g["mb%d_adj_loss_weights" % b] = np.vstack(lw).astype(np.float32)
            g["mb%d_zoom_labels" % b] = np.hstack(zl).astype(np.float32)
            state_arrays("mb%d_state" % b, g)
        cfg.SEAR.SCALE_ADJ_CONF = False
        g["n_batches"] = np.array(len(batches))
        path = os.path.join(GOLD, "g20_train_roidb.npz")
        np.savez_compressed(path, **g)
        print("wrote %s: %d KB" % (path, os.path.getsize(path) // 1024))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
