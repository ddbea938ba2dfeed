#!/usr/bin/env python3
"""Golden file of the diagnostic dump, produced by the REFERENCE's own detect.tune.test_proposals (lib/detect/tune.py:368-419)
imported from a temp copy (the recipe of oracle/gen_golden.py and oracle/gen_golden_next.py: lib2to3, stub caffe / cv2;
nothing of the reference is copied into the repo, and `np.object`, which NumPy removed, is aliased before the import):

  g24_az_results.mat   the AZ_results.mat the reference writes for a stub imdb of three images (100x64, 64x100, 120x160;
                       the second without objects) at cfg.SEAR.NUM_PROPOSALS = 50, Tz = 0.25 in Test mode.  The head
                       outputs are recorded from the oracle's small synthetic head in a first pass over the reference's
                       im_propose and REPLAYED (tests/helpers.ReplayNet, which checks the rois it is fed) while
                       test_proposals runs.

Run:  python tests/gen_golden_diag.py      (build container only; needs the reference tree)
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import numpy.ma            # noqa: F401  (before build_reference installs the np.bool / np.float aliases)
import scipy.io as sio
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, os.path.join(REPO, "az-net_amd", "lib"), REPO):
    sys.path.insert(0, p)
from oracle import gen_golden as gg          # noqa: E402
from oracle import gen_golden_next as gn     # noqa: E402
from aznet_hip import synth                  # noqa: E402
import helpers                               # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")
SHAPES = [(100, 64), (64, 100), (120, 160)]
GT = [np.array([[5, 8, 40, 60], [20, 30, 63, 99]], dtype=np.uint16), np.zeros((0, 4), dtype=np.uint16),
      np.array([[10, 10, 90, 70], [60, 40, 159, 119], [100, 5, 130, 30]], dtype=np.uint16)]


def main():
    tmp = tempfile.mkdtemp(prefix="azref_")
    try:
        _, _, _, _, C = gg.build_reference(tmp)
        np.object = object                                         # tune.py:375-379
        _, U = gn.import_more(tmp)
        head = synth.make_head(seed=77, **synth.SMALL_DIMS)
        images = {"/data/img%d.jpg" % i: synth.make_image(40 + i, h, w) for i, (h, w) in enumerate(SHAPES)}
        fmaps = {}
        for i, (h, w) in enumerate(SHAPES):
            s = 600.0 / min(h, w)
            if np.round(s * max(h, w)) > 1000:
                s = 1000.0 / max(h, w)
            hh, ww = int(round(h * s)), int(round(w * s))
            fmaps[(hh, ww)] = synth.make_feature_map(50 + i, synth.SMALL_DIMS["C"], synth.conv_out_size(hh),
                                                     synth.conv_out_size(ww))
        import cv2
        cv2.imread = lambda path: images[path]

        class StubImdb(object):
            name = "golden_diag"
            image_index = list(images.keys())
            roidb = [{"gt_overlaps": scipy.sparse.csr_matrix(np.eye(g.shape[0], 21, 1, dtype=np.float32))} for g in GT]

            def image_path_at(self, i):
                return self.image_index[i]

            def gt_roidb(self):
                return [{"boxes": g} for g in GT]

        C.cfg_set_path(None)
        C.cfg_set_mode("Test", 0.25)
        C.cfg.SEAR.NUM_PROPOSALS = 50
        C.cfg.SEAR.BATCH_SIZE = 10000
        # pass 1: record the head on the reference's own search, image by image
        full = gg.RecordingNet(head, feat_fn=lambda data: fmaps[(data.shape[2], data.shape[3])], name="golden_net")
        fcn = gg.RecordingNet(head, name="golden_net")
        # (one list in call order, as the traces of g7 / g11 hold them)
        order = []
        for net in (full, fcn):
            fwd = net.forward

            def spy(blobs=None, _fwd=fwd, _net=net, **kw):
                out = _fwd(blobs=blobs, **kw)
                order.append(_net.rec[-1])
                return out
            net.forward = spy
        for path in StubImdb.image_index:
            U.im_propose({"full": full, "fc": fcn}, images[path])
        g = {"ncalls": len(order), "fmap_shape": np.array([1, synth.SMALL_DIMS["C"], 1, 1])}
        for i, r in enumerate(order):
            for k in ("rois", "zoom_prob", "adj_prob", "adj_bbox"):
                g["c%d_%s" % (i, k)] = r[k]
            g["c%d_full" % i] = np.array(r["full"])
        # pass 2: the reference's test_proposals on the replayed head
        nets = {"full": helpers.ReplayNet(g, True, g["fmap_shape"], name="golden_net"),
                "fc": helpers.ReplayNet(g, False, g["fmap_shape"], name="golden_net")}
        U.test_proposals(nets, StubImdb())
        assert nets["full"].pos + nets["fc"].pos == len(order)
        out = os.path.join(C.get_output_dir(StubImdb(), nets["full"]), "AZ_results.mat")
        assert out.startswith(tmp)
        dst = os.path.join(GOLD, "g24_az_results.mat")
        shutil.copy(out, dst)
        m = sio.loadmat(dst)
        print({k: (v.dtype, v.shape) for k, v in m.items() if not k.startswith("__")})
        print("anchors", [m["anchor_boxes"][0, i].shape for i in range(3)], "proposals",
              [m["prop_boxes"][0, i].shape for i in range(3)], "bytes", os.path.getsize(dst))
        assert os.path.getsize(dst) < 64 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
