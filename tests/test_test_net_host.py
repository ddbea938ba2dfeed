"""CPU: detection over saved proposals (test_net, lib/detect/test.py:541-668) -- the oracle restatement pinned to
the reference's own run (tests/golden/g16_test_net.npz, tests/gen_golden_test_net.py), the CLI's flags and the
C-ABI entry of the batched head."""
import os
import sys

import numpy as np

from helpers import load

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")


def net_select_skipping_empty(per_image, num_classes, max_per_image=100):
    """orc.net_shared_select as test_net does it: per_image[i] is None for an image without proposals, which is
    skipped in both passes and keeps its [] placeholders (test.py:588-589, 647-649)."""
    import heapq
    num_images = len(per_image)
    max_per_set = 800 // (num_classes - 1) * num_images
    thresh = -np.inf * np.ones(num_classes)
    top_scores = [[] for _ in range(num_classes)]
    all_boxes = [[[] for _ in range(num_images)] for _ in range(num_classes)]
    for i, r in enumerate(per_image):
        if r is None:
            continue
        scores, boxes = r
        for j in range(1, num_classes):
            inds = np.where(scores[:, j] > thresh[j])[0]
            cls_scores = scores[inds, j]
            cls_boxes = boxes[inds, j * 4:(j + 1) * 4]
            top_inds = np.argsort(-cls_scores)[:max_per_image]
            cls_scores = cls_scores[top_inds]
            cls_boxes = cls_boxes[top_inds, :]
            for val in cls_scores:
                heapq.heappush(top_scores[j], val)
            if len(top_scores[j]) > max_per_set:
                while len(top_scores[j]) > max_per_set:
                    heapq.heappop(top_scores[j])
                thresh[j] = top_scores[j][0]
            all_boxes[j][i] = np.hstack((cls_boxes, cls_scores[:, np.newaxis])).astype(np.float32, copy=False)
    for j in range(1, num_classes):
        for i in range(num_images):
            if per_image[i] is None:
                continue
            inds = np.where(all_boxes[j][i][:, -1] > thresh[j])[0]
            all_boxes[j][i] = all_boxes[j][i][inds, :]
    return all_boxes, thresh


def _per_image(g):
    n = int(g["n_img"])
    return [(g["scores%d" % i], g["boxes%d" % i]) if g["prop%d" % i].shape[0] else None for i in range(n)]


def test_g16_bookkeeping_equals_the_restatement():
    from oracle import az_oracle as orc
    g = load("g16_test_net.npz")
    n = int(g["n_img"])
    per = _per_image(g)
    assert [p is None for p in per] == [False, True, False, False]
    want, _ = net_select_skipping_empty(per, 21)
    want_nms = orc.apply_nms(want, 0.5)             # cfg.TEST.NMS
    for j in range(1, 21):
        for i in range(n):
            if per[i] is None:
                assert want[j][i] == [] and "det_%d_%d" % (j, i) not in g.files and want_nms[j][i] == []
                continue
            assert np.array_equal(want[j][i], g["det_%d_%d" % (j, i)])
            k = "nms_%d_%d" % (j, i)
            w = want_nms[j][i]
            assert (isinstance(w, list) and k not in g.files) or np.array_equal(w, g[k])


def test_g16_im_detect_equals_oracle_frcnn_forward():
    """orc.frcnn_forward (CPU head, per-chunk dedup) gives the reference's im_detect outputs per image."""
    from aznet_hip import synth
    from oracle import az_oracle as orc
    g = load("g16_test_net.npz")
    dhead = synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)
    cfg = orc.OracleCfg(BATCH_SIZE=int(g["batch_size"]))
    for i in range(int(g["n_img"])):
        boxes = g["prop%d" % i]
        if boxes.shape[0] == 0:
            continue
        h, w = (int(x) for x in g["shape%d" % i])
        scale = 600.0 / min(h, w)
        fmap = synth.make_feature_map(int(g["map_seed"]) + i, synth.SMALL_DET_DIMS["C"],
                                      synth.conv_out_size(int(round(h * scale))), synth.conv_out_size(int(round(w * scale))))
        s, b = orc.frcnn_forward({"fc": orc.OracleDetNet(dhead)}, (h, w), scale, boxes, 21, {"conv5_3": fmap}, cfg)
        assert np.array_equal(s, g["scores%d" % i]) and np.array_equal(b, g["boxes%d" % i])


def test_g16_printed_lines_skip_empty_images():
    g = load("g16_test_net.npz")
    lines = str(g["stdout"]).splitlines()
    assert lines[:3] == ["im_detect: 1/4 0.000s 0.000s", "im_detect: 3/4 0.000s 0.000s", "im_detect: 4/4 0.000s 0.000s"]
    total = sum(g["prop%d" % i].shape[0] for i in range(4))
    assert lines[-1] == "On average, {0} boxes per image are generated".format(total / 4.0)


def test_test_det_net_accepts_every_reference_flag():
    sys.path[:0] = [TOOLS]
    try:
        import _cli
        import test_det_net
        p = _cli.build_parser("x", [_cli.COMMON, test_det_net.FLAGS])
        a = p.parse_args(["--gpu", "1", "--def", "frcnn/test.prototxt", "--net", "m.caffemodel", "--prop", "p.pkl",
                          "--cfg", "c.yml", "--wait", "", "--imdb", "voc_2007_test", "--comp", "--exp", "e",
                          "--batch-images", "4"])
    finally:
        sys.path.remove(TOOLS)
    assert (a.gpu_id, a.prototxt, a.caffemodel, a.prop, a.cfg_file, a.wait, a.imdb_name, a.comp_mode, a.exp_dir,
            a.batch_images) == (1, "frcnn/test.prototxt", "m.caffemodel", "p.pkl", "c.yml", False, "voc_2007_test", True,
                                "e", 4)


def test_binding_declares_az_detect_batch():
    from aznet_hip import ffi
    assert "az_detect_batch" in ffi.SYMBOLS
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    assert "int az_detect_batch(" in src


def test_detect_host_api_has_test_net():
    from detect import test as T
    from aznet_hip import net
    assert callable(T.test_net) and hasattr(net, "HipFrcnnNet")
