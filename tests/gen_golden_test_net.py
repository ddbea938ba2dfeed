#!/usr/bin/env python3
"""Golden vectors for detection over saved proposals, produced by the REFERENCE's own `test_net`
(lib/detect/test.py:541-668, the last step of tools/test_det_net.py) imported from the reference tree in a
temp dir by oracle.gen_golden.build_reference (nothing of the reference is copied into the repo).

The 'full' Fast R-CNN net is a stub: its conv5_3 is a seeded map per image (seed 60 + image index, of the size
VGG16 gives the image blob), its head the seed-99 small detection head on the CPU (orc.det_head_forward).
Four stub images of two shapes (375x500, 500x375); saved proposals with exact and 1/16 duplicates, boxes
that overhang the image, one image without proposals and one with a single box; cfg.SEAR.BATCH_SIZE = 64,
so an image's boxes span several dedup chunks.  Recorded in tests/golden/g16_test_net.npz:

  shape<i>, prop<i>, prop_time    the images' (h, w) and the saved proposals.pkl contents
  scores<i>, boxes<i>             what im_detect returned per image (images with proposals only)
  det_<j>_<i>                     detections.pkl[j][i] (float32 [n,5]; an image without proposals: absent, it stays [])
  nms_<j>_<i>                     what evaluate_detections received ([] -> absent)
  stdout                          what test_net printed (times replaced by 0.000)
  relpath                         detections.pkl relative to cfg.ROOT_DIR

Run:  python tests/gen_golden_test_net.py     (needs the reference tree; not collected by pytest)
"""
import contextlib
import io
import os
import pickle
import re
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "az-net_amd", "lib"))
from oracle import gen_golden as gg          # noqa: E402
from oracle import az_oracle as orc          # noqa: E402
from aznet_hip import synth                  # noqa: E402

GOLD = os.path.join(HERE, "golden")
SHAPES = [(375, 500), (500, 375), (375, 500), (500, 375)]
BATCH = 64
MAP_SEED = 60


def scrub(text):
    return re.sub(r"\d+\.\d{3}s", "0.000s", text)


def make_proposals(seed=16):
    """Saved proposals of the four images: [0] 150 boxes (exact and 1/16 duplicates, overhangs), [1] none,
    [2] one box, [3] 200 boxes."""
    rng = np.random.RandomState(seed)

    def boxes(n, h, w):
        x1 = rng.uniform(-20, w - 30, n)
        y1 = rng.uniform(-20, h - 30, n)
        bw = rng.uniform(8, w * 0.8, n)
        bh = rng.uniform(8, h * 0.8, n)
        b = np.stack([x1, y1, x1 + bw, y1 + bh], 1)
        b[:, [0, 1]] = np.maximum(b[:, [0, 1]], -15.0)              # overhangs on every side
        b[:, 2] = np.minimum(b[:, 2], w + 40.0)
        b[:, 3] = np.minimum(b[:, 3], h + 40.0)
        k = n // 6
        b[n - k:n - k // 2] = b[:k - k // 2]                         # exact duplicates (some within a chunk, some not)
        b[n - k // 2:] = b[3:3 + k // 2] + rng.uniform(-0.6, 0.6, (k // 2, 4))   # 1/16 duplicates at the test scale
        dup = rng.randint(0, n, 12)
        b[dup[6:]] = b[dup[:6]]                                      # ... and scattered repeats
        return np.round(b, 1).astype(np.float64)
    return [boxes(150, *SHAPES[0]), np.zeros((0, 4)), boxes(1, *SHAPES[2]), boxes(200, *SHAPES[3])]


def map_shape(h, w):
    s = 600.0 / min(h, w)
    return synth.conv_out_size(int(round(h * s))), synth.conv_out_size(int(round(w * s)))


def main():
    tmp = tempfile.mkdtemp(prefix="azref_")
    try:
        cdiv, cnms, cbbox, T, C = gg.build_reference(tmp)
        import cv2                                            # the stub module of build_reference

        def imread(path):
            _, i, h, w = path.rsplit("/", 3)
            return synth.make_image(int(i), int(h), int(w))
        cv2.imread = imread
        C.cfg.ROOT_DIR = os.path.join(tmp, "root")
        C.cfg_set_path("test_net")
        C.cfg_set_mode("Test", 0.0)
        C.cfg.SEAR.BATCH_SIZE = BATCH
        dhead = synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)
        props = make_proposals()

        class FullNet(object):
            """caffe.Net(frcnn/test.prototxt) stand-in: seeded conv5_3 of the image being read, CPU head."""
            name = "frcnn_small"

            class _Blob(object):
                def reshape(self, *shape):
                    self.shape = shape

            def __init__(self):
                self.blobs = {k: self._Blob() for k in ("data", "rois", "conv5_3")}
                self.cur = None

            def forward(self, blobs=None, **kw):
                _, _, bh, bw = kw["data"].shape
                fmap = synth.make_feature_map(MAP_SEED + self.cur, synth.SMALL_DET_DIMS["C"], synth.conv_out_size(bh),
                                              synth.conv_out_size(bw))
                p, b = orc.det_head_forward(dhead, fmap[0], kw["rois"])
                out = {"cls_prob": p, "bbox_pred": b}
                for name in blobs or []:
                    out[name] = fmap
                return out
        net = FullNet()

        class Imdb(object):
            name = "stub_4img"
            image_index = list(range(len(SHAPES)))
            num_classes = 21
            classes = ["c%d" % i for i in range(21)]

            def image_path_at(self, i):
                net.cur = i
                return "synthetic:/%d/%d/%d" % ((i,) + SHAPES[i])

            def evaluate_detections(self, nms_dets, output_dir):
                self.nms_dets = nms_dets
                self.eval_dir = output_dir
        imdb = Imdb()
        prop_time = 0.25
        pf = os.path.join(tmp, "proposals.pkl")
        with open(pf, "wb") as f:
            pickle.dump({"boxes": props, "time": prop_time, "recall": 0}, f, pickle.HIGHEST_PROTOCOL)

        rec = {}
        inner = T.im_detect

        def recording(n, im, boxes, num_classes):
            s, b = inner(n, im, boxes, num_classes)
            rec[net.cur] = (s.copy(), b.copy())
            return s, b
        T.im_detect = recording
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            T.test_net({"full": net}, pf, imdb)
        T.im_detect = inner
        out_dir = C.get_output_dir(imdb, net)
        df = os.path.join(out_dir, "detections.pkl")
        with open(df, "rb") as f:
            all_boxes = pickle.load(f)
        assert imdb.eval_dir == out_dir and sorted(rec) == [0, 2, 3]
        g = {"batch_size": np.array(BATCH), "map_seed": np.array(MAP_SEED), "prop_time": np.array(prop_time),
             "n_img": np.array(len(SHAPES)), "stdout": np.array(scrub(buf.getvalue())),
             "relpath": np.array(os.path.relpath(df, C.cfg.ROOT_DIR))}
        for i, sh in enumerate(SHAPES):
            g["shape%d" % i] = np.array(sh)
            g["prop%d" % i] = props[i]
            if i in rec:
                g["scores%d" % i], g["boxes%d" % i] = rec[i]
            for j in range(1, 21):
                a = all_boxes[j][i]
                if isinstance(a, list):
                    assert a == [] and props[i].shape[0] == 0
                    assert isinstance(imdb.nms_dets[j][i], list)
                    continue
                assert a.dtype == np.float32 and a.shape[1] == 5
                g["det_%d_%d" % (j, i)] = a
                n = imdb.nms_dets[j][i]
                if not isinstance(n, list):
                    g["nms_%d_%d" % (j, i)] = n
        np.savez_compressed(os.path.join(GOLD, "g16_test_net.npz"), **g)
        print("test_net: detections per class/image", [[all_boxes[j][i].__len__() for i in range(4)] for j in (1, 2, 20)])
        print(g["stdout"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
