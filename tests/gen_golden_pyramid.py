#!/usr/bin/env python3
"""Golden vectors for multi-scale test pyramids (cfg.TEST.SCALES with several entries), produced by the REFERENCE's own
lib/detect/test.py imported from the reference tree in a temp dir by oracle.gen_golden.build_reference (nothing of the
reference is copied into the repo).  Recorded in tests/golden/g19_pyramid.npz:

  blob_<k>_{shape,targets,max_size,scales,blob}   _get_image_blob of an image of that shape (the stub cv2 resizes to
                                                  zeros of the scaled shape, so the blob has the reference's padded shape)
  c<i>_{boxes,scales,dedup,batch}                 a dedup case: the boxes and settings
  c<i>_{rois,index,inv}                           _get_rois_blob of every BATCH_SIZE chunk and np.unique of its hash
                                                  (test.py:195-218): rois [P,5] f32, index global, inverse numbered
                                                  across chunks in chunk order
The cases: five-scale VGG pyramids (one capped by MAX_SIZE, so two levels tie exactly), boxes of every level,
degenerate (zero-area: all levels tie) and overhanging boxes, exact and near duplicates, dedup 1/16, 0.5 and 1, chunks of
several BATCH_SIZE, and one single-scale case.

Run:  python tests/gen_golden_pyramid.py     (needs the reference tree; not collected by pytest)
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from oracle import gen_golden as gg          # noqa: E402

GOLD = os.path.join(HERE, "golden")


def make_boxes(rng, n, h, w):
    """Boxes of every size from 4 px to the whole image (every pyramid level), overhangs, duplicates, degenerate boxes."""
    side = np.exp(rng.uniform(np.log(4.0), np.log(max(h, w) * 1.3), n))
    ar = np.exp(rng.uniform(-1.0, 1.0, n))
    bw, bh = side * ar, side / ar
    x1 = rng.uniform(-30, w - 10, n)
    y1 = rng.uniform(-30, h - 10, n)
    b = np.stack([x1, y1, x1 + bw, y1 + bh], 1)
    k = n // 8
    b[n - k:] = b[:k]                                            # exact duplicates
    b[n - 2 * k:n - k] = b[k:2 * k] + rng.uniform(-0.4, 0.4, (k, 4))   # near duplicates
    m = len(b[12::9])
    b[11::9] = b[10::9][:len(b[11::9])] + rng.uniform(-0.3, 0.3, (len(b[11::9]), 4))   # ... within a chunk
    b[12::9] = b[10::9][:m]                                      # exact duplicates within a chunk
    b[5, 2] = b[5, 0] - 1.0                                      # zero width: d_s = 224^2 at every level (a tie)
    b[6, 3] = b[6, 1] - 1.0
    b[7] = [0, 0, w - 1.0, h - 1.0]                              # the root
    return np.round(b, 2)


def main():
    tmp = tempfile.mkdtemp(prefix="azref_")
    try:
        _, _, _, T, C = gg.build_reference(tmp)
        g = {}
        blobs = [((375, 500), (480, 576, 688, 864, 1200), 2000), ((500, 375), (480, 576, 688, 864, 1200), 2000),
                 ((375, 500), (480, 600, 720), 1000), ((333, 500), (480, 600, 720, 864, 1200), 1000),
                 ((375, 500), (600,), 1000)]
        for k, (shape, targets, max_size) in enumerate(blobs):
            C.cfg.TEST.SCALES = targets
            C.cfg.TEST.MAX_SIZE = max_size
            blob, scales = T._get_image_blob(np.zeros(shape + (3,), dtype=np.uint8))
            g["blob_%d_shape" % k] = np.array(shape)
            g["blob_%d_targets" % k] = np.array(targets)
            g["blob_%d_max_size" % k] = np.array(max_size)
            g["blob_%d_scales" % k] = np.asarray(scales, dtype=np.float64)
            g["blob_%d_blob" % k] = np.array(blob.shape)
        rng = np.random.RandomState(19)
        cases = [(0, 300, 1. / 16., 64), (0, 300, 0.5, 64), (0, 300, 1.0, 100), (3, 400, 1. / 16., 128),
                 (3, 200, 0.5, 10000), (1, 250, 1. / 16., 64), (4, 120, 1. / 16., 64), (2, 150, 1.0, 32)]
        for i, (bk, n, dd, batch) in enumerate(cases):
            h, w = (int(x) for x in g["blob_%d_shape" % bk])
            scales = g["blob_%d_scales" % bk]
            boxes = make_boxes(rng, n, h, w)
            C.cfg.DEDUP_BOXES = dd
            rois_all, index, inv, off = [], [], [], 0
            for s in range(0, n, batch):
                rois = T._get_rois_blob(boxes[s:s + batch], scales)
                v = np.array([1, 1e3, 1e6, 1e9, 1e12])                      # test.py:212-214
                hashes = np.round(rois * C.cfg.DEDUP_BOXES).dot(v)
                _, ix, iv = np.unique(hashes, return_index=True, return_inverse=True)
                rois_all.append(rois)
                index.append(ix + s)
                inv.append(iv.ravel() + off)
                off += len(ix)
            g["c%d_boxes" % i] = boxes
            g["c%d_scales" % i] = scales
            g["c%d_dedup" % i] = np.array(dd)
            g["c%d_batch" % i] = np.array(batch)
            g["c%d_rois" % i] = np.concatenate(rois_all).astype(np.float32)
            g["c%d_index" % i] = np.concatenate(index).astype(np.int32)
            g["c%d_inv" % i] = np.concatenate(inv).astype(np.int32)
        g["n_cases"] = np.array(len(cases))
        g["n_blobs"] = np.array(len(blobs))
        np.savez_compressed(os.path.join(GOLD, "g19_pyramid.npz"), **g)
        for i in range(len(cases)):
            lv = g["c%d_rois" % i][:, 0]
            print("case %d: S=%d levels %s unique %d / %d" % (i, len(g["c%d_scales" % i]),
                                                               np.bincount(lv.astype(int)).tolist(),
                                                               len(g["c%d_index" % i]), len(lv)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
