#!/usr/bin/env python3
"""Golden vectors for the training data layer's edge cases (tests/train_edges_ref.py), produced by the REFERENCE's own
lib/az_data_layer/roidb.py with its cfg edited per case, imported from a temp copy of the reference tree made by
oracle.gen_golden.build_reference (the machinery of tests/gen_golden_train.py; nothing of the reference is copied into the
repo).  For every case the generator asserts that tests/train_ref.py gives the reference's bits: boxes, labels and doubles
used exactly, and the targets exactly (dw / dh included: the same glibc log).  Recorded in tests/golden/g23_train_roidb_edges.npz:

  L_<name>_{E,used,n_zoom,T,levels,sha_*}     group A (large levels): counts, the (P, PZ, CH) of every zoomed level, and the
                                              SHA-256 of ex_boxes as f64 and as f32, zoom_gt, the level table and the targets
  S_{E,used,sha_*} per image                  the shared-stream call of group A, image by image on one stream
  B_<name>_{size,gt,seed,ex_boxes,zoom_gt,used,targets}     group B (parameters, image sizes), in full
  BE_*                                        the batch with empty images: per image as B, on one stream
The large cases record no levels for what the reference itself cannot tell (its divide_region is one call): the level table
is train_ref's, whose boxes equal the reference's at every level or the final arrays would differ.

Run:  python tests/gen_golden_train_edges.py     (needs the reference tree; not collected by pytest)
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
import train_edges_ref as E                  # noqa: E402
from gen_golden_train import CountingRandom  # noqa: E402

GOLD = os.path.join(HERE, "golden")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def main():
    tmp = tempfile.mkdtemp(prefix="azref_")
    try:
        _, _, _, T, C = gg.build_reference(tmp)
        lib = os.path.join(tmp, "py", "lib")
        f = os.path.join(lib, "az_data_layer", "roidb.py")
        src = open(f).read().expandtabs(8)
        open(f, "w").write(src)
        subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", f], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        open(os.path.join(lib, "az_data_layer", "__init__.py"), "w").close()
        R = importlib.import_module("az_data_layer.roidb")
        assert R.__file__.startswith(tmp)
        cfg = C.cfg
        cfg.TRAIN.USE_CACHE = False
        g = {}

        def reference(size, gt, kw, seed=None, with_targets=True):
            """The reference on one image under cfg edited by `kw` (from np.random's current position when seed is None)
            -> (ex f64, labels, used, targets), checked against train_ref on the same doubles."""
            c = E.cfg_of(kw)
            with E.patched_cfg(cfg, {k: (np.array(v) if k in ("addregions", "subregion") else v) for k, v in kw.items()}):
                if seed is not None:
                    np.random.seed(seed)
                state = np.random.get_state()
                cnt = CountingRandom()
                R.npr = cnt
                try:
                    ex, zl = R._compute_ex_rois(size, gt)
                finally:
                    R.npr = np.random
                after = np.random.get_state()
                np.random.set_state(state)
                noise = np.random.random(cnt.used + 5)
                np.random.set_state(after)
                t = np.zeros((0, 7))
                if with_targets:
                    t = np.asarray(R._compute_targets(gt.astype(np.float32), ex.astype(np.float32)), dtype=np.float64).reshape(-1, 7)
            stats = {}
            b, z, u = train_ref.compute_ex_rois(size, gt, noise, c, stats)
            assert u == cnt.used and same(b, ex) and same(z, zl.astype(bool)), "train_ref differs from the reference (ex)"
            if with_targets:
                t2 = train_ref.compute_targets(gt, ex.astype(np.float32), c)
                assert same(t2, t), "train_ref differs from the reference (targets)"
            return ex, zl.astype(bool), cnt.used, t, stats

        # ---- A ------------------------------------------------------------------------------------------------------------
        for name, (size, gt, seed, kw, answer) in sorted(E.LEVEL_CASES.items()):
            ex, zl, used, t, stats = reference(size, gt, kw, seed)
            s = E.level_summary(stats)
            for k, v in E.level_digests(size, gt, ex, zl, used, t, s["levels"]).items():
                g["L_%s_%s" % (name, k)] = v
            print("A %-16s %s N=%d E=%d used=%d T=%d max P=%d PZ=%d CH=%d one parent=%d -> %s"
                  % (name, size, gt.shape[0], ex.shape[0], used, t.shape[0], s["max_P"], s["max_PZ"], s["max_CH"],
                     s["max_parent"], answer))
        np.random.seed(E.SHARED_STREAM["seed"])
        for i, (size, gt) in enumerate(E.SHARED_STREAM["images"]):
            ex, zl, used, t, stats = reference(size, gt, E.SHARED_STREAM["kw"])
            for k, v in E.level_digests(size, gt, ex, zl, used, t, E.level_summary(stats)["levels"]).items():
                g["S%d_%s" % (i, k)] = v
            print("A shared stream %d: %s N=%d E=%d used=%d" % (i, size, gt.shape[0], ex.shape[0], used))
        # ---- B ------------------------------------------------------------------------------------------------------------
        for name, size, gt, seed, kw in E.param_cases():
            ex, zl, used, t, _ = reference(size, gt, kw, seed)
            for k, v in (("size", np.array(size)), ("gt", gt), ("seed", np.array(seed)), ("ex_boxes", ex), ("zoom_gt", zl),
                         ("used", np.array(used)), ("targets", t)):
                g["B_%s_%s" % (name, k)] = v
            print("B %-12s %s N=%d E=%d zoom=%d used=%d T=%d" % (name, size, gt.shape[0], ex.shape[0], int(zl.sum()), used,
                                                                 t.shape[0]))
        np.random.seed(E.EMPTY_BATCH["seed"])
        for i, (size, gt) in enumerate(E.empty_batch_images()):
            ex, zl, used, t, _ = reference(size, gt, E.EMPTY_BATCH["kw"])
            for k, v in (("ex_boxes", ex), ("zoom_gt", zl), ("used", np.array(used)), ("targets", t)):
                g["BE%d_%s" % (i, k)] = v
        path = os.path.join(GOLD, "g23_train_roidb_edges.npz")
        np.savez_compressed(path, **g)
        print("wrote %s: %d KB" % (path, os.path.getsize(path) // 1024))
        assert os.path.getsize(path) < 810 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
