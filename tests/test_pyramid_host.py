"""CPU: multi-scale test pyramids (cfg.TEST.SCALES with several entries) -- the NumPy restatement of the reference's
pyramid projection and dedup (tests/pyramid_ref.py) against what the REFERENCE's own lib/detect/test.py recorded in
tests/golden/g19_pyramid.npz (tests/gen_golden_pyramid.py), the scale factors and padded blob shape of
detect.test, and a YAML with TEST.SCALES."""
import os

import numpy as np

import pyramid_ref as pr
from helpers import load


def test_restatement_reproduces_the_reference_dedup():
    g = load("g19_pyramid.npz")
    for i in range(int(g["n_cases"])):
        boxes, scales = g["c%d_boxes" % i], g["c%d_scales" % i]
        rois, index, inv = pr.chunked(boxes, scales, float(g["c%d_dedup" % i]), int(g["c%d_batch" % i]))
        assert rois.dtype == np.float32 and np.array_equal(rois, g["c%d_rois" % i]), i
        assert np.array_equal(index, g["c%d_index" % i]), i
        assert np.array_equal(inv, g["c%d_inv" % i]), i


def test_fixture_covers_ties_levels_and_dedup():
    g = load("g19_pyramid.npz")
    seen_levels, tie_cases, dup_cases = set(), 0, 0
    for i in range(int(g["n_cases"])):
        scales, rois = g["c%d_scales" % i], g["c%d_rois" % i]
        seen_levels |= {(len(scales), int(v)) for v in rois[:, 0]}
        tie_cases += int(len(scales) != len(np.unique(scales)))
        dup_cases += int(len(g["c%d_index" % i]) < len(rois))
        boxes = g["c%d_boxes" % i]
        if len(scales) > 1:
            zero = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1) == 0
            assert zero.any() and np.all(rois[zero, 0] == 0), i     # every level ties: np.argmin takes the first
    assert {(5, l) for l in range(5)} <= seen_levels and tie_cases >= 2 and dup_cases == int(g["n_cases"])
    assert sorted({float(g["c%d_dedup" % i]) for i in range(int(g["n_cases"]))}) == [1. / 16., 0.5, 1.0]


def test_im_scale_and_padded_blob_shape():
    from detect import config as C
    from detect import test as T
    g = load("g19_pyramid.npz")
    old = (C.cfg.TEST.SCALES, C.cfg.TEST.MAX_SIZE)
    try:
        for k in range(int(g["n_blobs"])):
            shape = tuple(int(x) for x in g["blob_%d_shape" % k])
            C.cfg.TEST.SCALES = tuple(int(x) for x in g["blob_%d_targets" % k])
            C.cfg.TEST.MAX_SIZE = int(g["blob_%d_max_size" % k])
            scales = T._im_scale(shape)
            assert np.array_equal(np.array(scales), g["blob_%d_scales" % k]), k
            assert np.array_equal(pr.scales_for(shape, C.cfg.TEST.SCALES, C.cfg.TEST.MAX_SIZE), g["blob_%d_scales" % k])
            assert pr.blob_shape(shape, scales) == tuple(int(x) for x in g["blob_%d_blob" % k]), k
    finally:
        C.cfg.TEST.SCALES, C.cfg.TEST.MAX_SIZE = old


def test_yaml_with_test_scales_merges(tmp_path):
    from detect import config as C
    old = (C.cfg.TEST.SCALES, C.cfg.TEST.MAX_SIZE)
    p = os.path.join(str(tmp_path), "pyr.yml")
    with open(p, "w") as f:
        f.write("TEST:\n  SCALES: [480, 576, 688, 864, 1200]\n  MAX_SIZE: 2000\n")
    try:
        C.cfg_from_file(p)
        assert tuple(C.cfg.TEST.SCALES) == (480, 576, 688, 864, 1200) and C.cfg.TEST.MAX_SIZE == 2000
    finally:
        C.cfg.TEST.SCALES, C.cfg.TEST.MAX_SIZE = old
