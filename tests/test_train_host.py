"""CPU: the training data layer's host logic against what the REFERENCE's own az_data_layer/roidb.py and minibatch.py
recorded (tests/golden/g20_train_roidb.npz).  The NumPy restatement tests/train_ref.py (explicit noise) equals the
goldens bit for bit -- it shares glibc's log with the reference here --, and stands in for the device entry points so
that imdb.append_flipped_images / image_size, prepare_roidb's np.random bookkeeping, the caches, the minibatch sampler
and AZDataLayer's index logic run without a GPU."""
import os
import pickle
import re

import numpy as np
import pytest

import train_ref as tr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g20_train_roidb.npz")
C = tr.TrainCfg()


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture()
def ref_backend():
    from az_data_layer import roidb as rdl
    rdl.set_backend(tr.RefBackend())
    yield rdl
    rdl.set_backend(None)


class FakeBlobCtx(object):
    """The image front-end's shape arithmetic without the GPU (cv2's dsize: round half to even)."""

    def image_blob(self, im, means, scale):
        return np.zeros((1, 3, int(np.round(im.shape[0] * scale)), int(np.round(im.shape[1] * scale))), np.float32)


def test_restatement_equals_reference(g):
    targets = []
    for i in range(int(g["n_cases"])):
        np.random.seed(int(g["c%d_seed" % i]))
        noise = np.random.random(int(g["c%d_used" % i]) + 3)
        size = tuple(int(v) for v in g["c%d_size" % i])
        ex, zl, used = tr.compute_ex_rois(size, g["c%d_gt" % i], noise, C)
        assert used == int(g["c%d_used" % i]), i
        assert np.array_equal(ex, g["c%d_ex_boxes" % i]) and np.array_equal(zl, g["c%d_zoom_gt" % i]), i
        assert np.array_equal(tr.zoom_labels(ex, g["c%d_gt" % i], C.emb_reg_thresh, C.emb_obj_thresh),
                              g["c%d_zoom_of_ex" % i]), i
        t = tr.compute_targets(g["c%d_gt" % i], ex.astype(np.float32), C)
        assert t.shape == g["c%d_targets" % i].shape and np.array_equal(t, g["c%d_targets" % i]), i
        targets.append(t)
    means, stds = tr.target_stats(targets, C)          # per image, as the reference accumulates
    assert np.array_equal(means.ravel(), g["set_means"]) and np.array_equal(stds.ravel(), g["set_stds"])
    assert np.array_equal(np.vstack(targets), g["set_targets"])


def test_goldens_pin_the_quirks(g):
    """The cases reach what the issue asks for: an empty image, a never-embedded object, matches won at overlap 0,
    tied maxima, more objects than sub-regions, clipped-away super-regions."""
    assert g["c3_gt"].shape[0] == 0 and g["c3_ntargets"] == 0 and not g["c3_zoom_gt"].any()
    trace = {}
    for i in (5, 7):
        tr.compute_targets(g["c%d_gt" % i], g["c%d_ex_boxes" % i].astype(np.float32), C, trace)
    assert trace["zero_rounds"] >= 1 and trace["ties"] >= 1
    assert g["c8_gt"].shape[0] >= 12 and g["c9_gt"].shape[0] >= 12
    trace = {}
    tr.compute_targets(g["c9_gt"], g["c9_ex_boxes"].astype(np.float32), C, trace)
    k, n = np.unique(g["c9_targets"][:, 4], return_counts=True)
    assert trace["bound"] >= 1 and n.max() == 11                 # min(11, .) binds
    # thin objects: some of their 11 super-regions fall below MIN_SIDE once clipped to the image
    h, w = (int(v) for v in g["c6_size"])
    dropped = 0
    for ri in g["c6_gt"]:
        rs = tr.super_regions(ri, C.subregion)
        x1, y1 = np.maximum(rs[:, 0], 0), np.maximum(rs[:, 1], 0)
        x2, y2 = np.minimum(rs[:, 2], w - 1), np.minimum(rs[:, 3], h - 1)
        dropped += int((np.minimum(x2 - x1 + 1, y2 - y1 + 1) < C.min_side).sum())
    assert dropped >= 1


def test_image_size_and_flipped_images(tmp_path, g):
    from datasets.synthetic import NpyDirImdb, SyntheticImdb
    imdb = SyntheticImdb(375, 500, 8)
    assert imdb.image_size(3) == (375, 500)
    before = [e["boxes"].copy() for e in imdb.roidb]
    imdb.append_flipped_images()
    assert imdb.num_images == 16 and len(imdb.roidb) == 16 and imdb.image_index == list(range(8)) * 2
    for i in range(8):
        a, b = before[i], imdb.roidb[8 + i]["boxes"]
        assert imdb.roidb[8 + i]["flipped"] and not imdb.roidb[i]["flipped"]
        assert b.dtype == a.dtype and np.array_equal(b, g["syn%d_boxes" % (8 + i)])
        assert np.array_equal(b[:, 0], 500 - a[:, 2].astype(int) - 1) and np.array_equal(b[:, 2], 500 - a[:, 0].astype(int) - 1)
        assert np.array_equal(b[:, [1, 3]], a[:, [1, 3]])
        assert imdb.image_size(8 + i) == (375, 500)
    np.save(str(tmp_path / "a.npy"), np.zeros((33, 57, 3), dtype=np.uint8))
    np.save(str(tmp_path / "a_gt.npy"), np.array([[3., 4., 20., 30., 2.]]))
    d = NpyDirImdb(str(tmp_path))
    assert d.image_size(0) == (33, 57)
    d.append_flipped_images()
    assert d.roidb[1]["boxes"].tolist() == [[57 - 20 - 1, 4, 57 - 3 - 1, 30]]
    from PIL import Image
    Image.new("RGB", (41, 29)).save(str(tmp_path / "p.png"))
    from datasets.imdb import imdb as base

    class One(base):
        def image_path_at(self, i):
            return str(tmp_path / "p.png")
    assert One("one").image_size(0) == (29, 41)
    assert os.path.isdir(One("one").cache_path)


def synthetic_roidb(rdl, seed=3):
    from datasets.synthetic import SyntheticImdb
    from detect.train_az import get_training_roidb
    imdb = SyntheticImdb(375, 500, 8)
    np.random.seed(seed)
    roidb = get_training_roidb(imdb)             # cfg.TRAIN.USE_FLIPPED: appends the flipped entries
    assert roidb is imdb.roidb
    state = np.random.get_state()
    means, stds = rdl.add_adjacent_prediction_targets(imdb)
    return imdb, state, means, stds


def test_prepare_roidb_on_the_restatement(ref_backend, g):
    imdb, state, means, stds = synthetic_roidb(ref_backend)
    # np.random is left where the reference leaves it
    assert np.array_equal(state[1], g["syn_state_keys"]) and int(state[2]) == int(g["syn_state_pos"][0])
    assert len(imdb.roidb) == int(g["syn_n"])
    for i, e in enumerate(imdb.roidb):
        assert e["image"] == "synthetic://%d" % (i % 8)
        for k in ("ex_boxes", "zoom_gt", "gt_boxes"):
            assert e[k].dtype == g["syn%d_%s" % (i, k)].dtype and np.array_equal(e[k], g["syn%d_%s" % (i, k)]), (i, k)
        ref = g["syn%d_bbox_targets" % i]
        assert e["bbox_targets"].dtype == np.float64 and e["bbox_targets"].shape == ref.shape
        assert np.array_equal(e["bbox_targets"][:, 4:], ref[:, 4:])
        # (the restatement's backend sums the set in one pass, the reference image by image: 1e-12)
        assert np.allclose(e["bbox_targets"][:, :4], ref[:, :4], rtol=1e-11, atol=1e-11)
    assert means.shape == (44,) and np.allclose(means, g["syn_means"], rtol=0, atol=1e-12)
    assert np.allclose(stds, g["syn_stds"], rtol=1e-11, atol=1e-12)


def test_noise_block_is_retried(ref_backend, g, monkeypatch):
    """A first block of uniforms that is too small: the chunk runs again with a larger one, same result, same state."""
    monkeypatch.setattr(ref_backend, "NOISE_PER_IMAGE", 16)
    monkeypatch.setattr(ref_backend, "CHUNK", 5)
    imdb, state, _, _ = synthetic_roidb(ref_backend)
    assert np.array_equal(state[1], g["syn_state_keys"]) and int(state[2]) == int(g["syn_state_pos"][0])
    for i, e in enumerate(imdb.roidb):
        assert np.array_equal(e["ex_boxes"], g["syn%d_ex_boxes" % i])


def test_gt_overlaps_select_the_ground_truth(ref_backend):
    import scipy.sparse
    from datasets.synthetic import SyntheticImdb
    imdb = SyntheticImdb(375, 500, 2)
    for e in imdb.roidb:
        ov = np.zeros((e["boxes"].shape[0], 21), dtype=np.float32)
        ov[np.arange(ov.shape[0]), e["gt_classes"]] = 1.0
        ov[0, :] = 0.0
        ov[0, 3] = 0.7                                    # a proposal, not ground truth
        e["gt_overlaps"] = scipy.sparse.csr_matrix(ov)
    np.random.seed(1)
    ref_backend.prepare_roidb(imdb)
    for e in imdb.roidb:
        assert np.array_equal(e["gt_boxes"], e["boxes"][1:].astype(np.float32))


def test_caches_hold_per_image_lists(ref_backend, tmp_path, monkeypatch):
    from datasets.synthetic import SyntheticImdb
    from detect.config import cfg
    monkeypatch.setattr(SyntheticImdb, "cache_path", str(tmp_path))
    monkeypatch.setattr(cfg.TRAIN, "USE_CACHE", True)
    try:
        a = SyntheticImdb(375, 500, 3)
        np.random.seed(5)
        ref_backend.prepare_roidb(a)
        ma, sa = ref_backend.add_adjacent_prediction_targets(a)
        with open(str(tmp_path / (a.name + "_trainable_roidb.pkl")), "rb") as f:
            c1 = pickle.load(f)
        with open(str(tmp_path / (a.name + "_targets_roidb.pkl")), "rb") as f:
            c2 = pickle.load(f)
        assert sorted(c1) == ["ex_boxes", "gt_boxes", "zoom_gt"] and all(len(c1[k]) == 3 for k in c1)
        assert sorted(c2) == ["bbox_targets", "means", "stds"] and len(c2["bbox_targets"]) == 3
        b = SyntheticImdb(375, 500, 3)
        state = np.random.get_state()
        ref_backend.set_backend(None)                      # a cache hit touches neither the device nor np.random
        ref_backend.prepare_roidb(b)
        mb, sb = ref_backend.add_adjacent_prediction_targets(b)
        assert np.array_equal(np.random.get_state()[1], state[1])
        assert np.array_equal(ma, mb) and np.array_equal(sa, sb)
        for x, y in zip(a.roidb, b.roidb):
            for k in ("ex_boxes", "zoom_gt", "gt_boxes", "bbox_targets", "image"):
                assert np.array_equal(x[k], y[k])
    finally:
        cfg.TRAIN.USE_CACHE = False


def golden_roidb(g):
    out = []
    for i in range(int(g["syn_n"])):
        e = {k: g["syn%d_%s" % (i, k)] for k in ("ex_boxes", "zoom_gt", "gt_boxes", "bbox_targets")}
        e.update(flipped=bool(g["syn%d_flipped" % i]), image="synthetic://%d" % (i % 8), height=375, width=500)
        out.append(e)
    return out


def test_minibatch_sampler(g):
    from az_data_layer.minibatch import get_minibatch
    from detect.config import cfg
    roidb = golden_roidb(g)
    for b in range(int(g["n_batches"])):
        cfg.SEAR.SCALE_ADJ_CONF = bool(g["mb%d_conf" % b])
        try:
            np.random.seed(int(g["mb%d_seed" % b]))
            blobs = get_minibatch([roidb[i] for i in g["mb%d_inds" % b]], 11, FakeBlobCtx())
        finally:
            cfg.SEAR.SCALE_ADJ_CONF = False
        st = np.random.get_state()
        assert np.array_equal(st[1], g["mb%d_state_keys" % b]) and int(st[2]) == int(g["mb%d_state_pos" % b][0])
        assert sorted(blobs) == ["adj_labels", "adj_loss_weights", "adj_targets", "data", "rois", "zoom_labels"]
        assert blobs["data"].shape == (len(g["mb%d_inds" % b]), 3, 600, 800)
        for k in ("rois", "adj_labels", "adj_targets", "adj_loss_weights", "zoom_labels"):
            assert np.array_equal(np.asarray(blobs[k]).astype(np.float32), g["mb%d_%s" % (b, k)]), (b, k)
        assert blobs["rois"].shape[0] == blobs["adj_labels"].shape[0] == blobs["zoom_labels"].shape[0] <= cfg.TRAIN.BATCH_SIZE
        if g["mb%d_conf" % b]:
            lab = blobs["adj_labels"]
            assert ((lab > 0) & (lab < 1)).any()


def test_data_layer_index_logic(g):
    from az_data_layer.layer import AZDataLayer, BLOB_NAMES
    from detect.config import cfg
    roidb = golden_roidb(g)[:5]
    layer = AZDataLayer(ctx=FakeBlobCtx())
    np.random.seed(9)
    layer.set_roidb(roidb)
    np.random.seed(9)
    perm = np.random.permutation(np.arange(5))
    assert np.array_equal(layer._perm, perm) and layer._cur == 0
    assert cfg.TRAIN.IMS_PER_BATCH == 2
    assert np.array_equal(layer._get_next_minibatch_inds(), perm[0:2]) and layer._cur == 2
    assert np.array_equal(layer._get_next_minibatch_inds(), perm[2:4]) and layer._cur == 4
    state = np.random.get_state()
    inds = layer._get_next_minibatch_inds()                # 4 + 2 >= 5: reshuffle first (layer.py:34-35)
    np.random.set_state(state)
    assert np.array_equal(inds, np.random.permutation(np.arange(5))[0:2]) and layer._cur == 2
    blobs = layer.forward()
    assert sorted(blobs) == sorted(BLOB_NAMES) and all(v.dtype == np.float32 for v in blobs.values())
    assert blobs["adj_targets"].shape[1] == 44 and blobs["rois"].shape[1] == 5


def test_header_declares_the_training_entries():
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    from aznet_hip import ffi
    for name in ("az_zoom_labels", "az_train_ex_rois", "az_train_adj_targets", "az_train_target_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in ffi.SYMBOLS
    assert "az_train_params" in src
    import ctypes
    assert ctypes.sizeof(ffi.AzTrainParams) == 6 * 8 + 4 * 4 + 2 * ffi.AZ_TRAIN_MAX_REGIONS * 4 * 8    # az_capi.hip asserts the same
    assert int(re.search(r"#define\s+AZ_TRAIN_MAX_REGIONS\s+(\d+)", src).group(1)) == ffi.AZ_TRAIN_MAX_REGIONS
