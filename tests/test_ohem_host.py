"""CPU: online hard-example mining off the device -- the pool builder of roi_data_layer.minibatch on hand-made roidb entries,
what np.random is asked for with the switch on and off, the configuration keys, the tool's flag, the 4096-row refusal, the
two new entries in header / binding / library, and the restatement (tests/ohem_ref.py): its selection against the oracle's nms
and on ties, duplicates, the thresholds and empty images, its float32 row losses against float64, and the planted case that
tests/test_gpu_ohem.py holds the device to."""
import ctypes
import os
import re

import numpy as np
import pytest

import ohem_ref as O
import train_step_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


@pytest.fixture
def ohem_cfg(monkeypatch):
    from detect.config import cfg
    for k, v in dict(OHEM=True, OHEM_NMS=0.7, OHEM_POOL=2000, BATCH_SIZE=8, IMS_PER_BATCH=2, SCALES=(600, 480)).items():
        monkeypatch.setattr(cfg.TRAIN, k, v)
    return cfg


def entry(seed, overlaps, labels=None):
    """A roidb entry with the given max_overlaps: boxes and compact targets by row number, so a gathered row names its source."""
    ov = np.asarray(overlaps, np.float64)
    n = ov.size
    lab = np.where(ov >= 0.5, 1 + np.arange(n) % (K - 1), 0) if labels is None else np.asarray(labels)
    boxes = np.stack([np.arange(n), 2 * np.arange(n), 40 + np.arange(n), 60 + 2 * np.arange(n)], 1).astype(np.float32)
    tgt = np.hstack((lab[:, None], 0.25 * (1 + np.arange(n))[:, None] * np.array([[1, -1, 2, -2]]))).astype(np.float32)
    return {"image": "synthetic://%d" % seed, "height": 120, "width": 160, "flipped": False, "max_overlaps": ov,
            "ex_boxes": boxes, "bbox_targets": tgt}


# ---- the pool builder ----------------------------------------------------------------------------------------------------
def test_pool_bands_order_and_labels(ohem_cfg):
    from roi_data_layer.minibatch import get_ohem_minibatch, ohem_pool_inds
    ov = [0.05, 0.7, 0.1, 0.3, 0.5, 0.0999, 0.49999, 0.9, 0.0]
    e = entry(1, ov)
    keep, n_fg = ohem_pool_inds(e)
    assert keep.tolist() == [1, 4, 7, 2, 3, 6] and n_fg == 3                 # fg in order, then [0.1, 0.5) in order
    want, want_fg = O.pool_inds(ov, 0.5, 0.5, 0.1, 2000)
    assert np.array_equal(keep, want) and n_fg == want_fg
    np.random.seed(4)
    blobs = get_ohem_minibatch([e, entry(2, [0.2, 0.6])], K, R.ShapeOnlyBlobCtx())
    assert sorted(blobs) == ["data", "labels", "rois", "targets"]
    scale = 600.0 / 120 if blobs["data"].shape[2] >= 600 else 480.0 / 120
    assert blobs["rois"].shape == (8, 5) and blobs["rois"][:, 0].tolist() == [0] * 6 + [1] * 2
    assert blobs["labels"].tolist() == [e["bbox_targets"][i, 0] for i in (1, 4, 7)] + [0, 0, 0] + [2, 0]
    assert blobs["targets"].shape == (8, 4) and np.array_equal(blobs["targets"][:6], e["bbox_targets"][keep, 1:])
    im0 = blobs["rois"][:6, 1:] / e["ex_boxes"][keep]
    assert np.ptp(im0[np.isfinite(im0) & (e["ex_boxes"][keep] > 0)]) < 1e-6 and scale in (5.0, 4.0)


def test_pool_empty_band_falls_back_as_sample_rois_does(ohem_cfg):
    from roi_data_layer.minibatch import ohem_pool_inds
    keep, n_fg = ohem_pool_inds(entry(1, [0.05, 0.8, 0.0, 0.09]))            # nothing in [0.1, 0.5): everything below FG_THRESH
    assert keep.tolist() == [1, 0, 2, 3] and n_fg == 1
    keep, n_fg = ohem_pool_inds(entry(1, [0.05, 0.2, 0.0]))                  # an image without foreground
    assert keep.tolist() == [1] and n_fg == 0
    keep, n_fg = ohem_pool_inds(entry(1, [0.9, 0.6]))                        # ... and one without background
    assert keep.tolist() == [0, 1] and n_fg == 2


def test_pool_truncation_keeps_the_foreground(ohem_cfg, monkeypatch):
    from roi_data_layer.minibatch import get_ohem_minibatch, ohem_pool_inds
    ov = [0.2, 0.3, 0.6, 0.2, 0.7, 0.4, 0.8]
    monkeypatch.setattr(ohem_cfg.TRAIN, "OHEM_POOL", 4)
    keep, n_fg = ohem_pool_inds(entry(1, ov))
    assert keep.tolist() == [2, 4, 6, 0] and n_fg == 3
    monkeypatch.setattr(ohem_cfg.TRAIN, "OHEM_POOL", 2)                      # fewer than the foreground: its first rows
    keep, n_fg = ohem_pool_inds(entry(1, ov))
    assert keep.tolist() == [2, 4] and n_fg == 2
    np.random.seed(1)
    blobs = get_ohem_minibatch([entry(1, ov), entry(2, ov)], K, R.ShapeOnlyBlobCtx())
    assert blobs["rois"].shape[0] == 4 and np.all(blobs["labels"] > 0)
    monkeypatch.setattr(ohem_cfg.TRAIN, "FG_FRACTION", 0.0)                  # plays no part
    assert ohem_pool_inds(entry(1, ov))[0].tolist() == [2, 4]


def test_np_random_is_asked_for_the_scales_only(ohem_cfg):
    from roi_data_layer.minibatch import get_ohem_minibatch
    es = [entry(1, [0.2, 0.3, 0.6, 0.2, 0.7]), entry(2, [0.9, 0.1, 0.1])]
    np.random.seed(11)
    get_ohem_minibatch(es, K, R.ShapeOnlyBlobCtx())
    after = np.random.get_state()
    np.random.seed(11)
    np.random.randint(0, high=2, size=2)
    want = np.random.get_state()
    assert bits(after[1]) == bits(want[1]) and after[2] == want[2]
    bad = entry(3, [0.9, 0.2])
    bad["bbox_targets"][0, 2] = np.nan
    with pytest.raises(AssertionError, match="nan or inf"):
        get_ohem_minibatch([bad, es[1]], K, R.ShapeOnlyBlobCtx())


def test_switch_off_the_layer_draws_what_it_drew(monkeypatch):
    """With TRAIN.OHEM off, RoIDataLayer.forward is get_minibatch on the same entries: the blobs and np.random's state after
    one call equal a direct call's."""
    from detect.config import cfg
    from roi_data_layer.layer import RoIDataLayer
    from roi_data_layer.minibatch import get_minibatch
    assert cfg.TRAIN.OHEM is False
    monkeypatch.setattr(cfg.TRAIN, "BATCH_SIZE", 8)
    rng = np.random.Generator(np.random.PCG64(3))
    roidb = [entry(i, rng.uniform(0, 1, 30)) for i in range(6)]
    np.random.seed(21)
    layer = RoIDataLayer(K, ctx=R.ShapeOnlyBlobCtx())
    layer.set_roidb(roidb)
    mid = np.random.get_state()
    got = layer.forward()
    after = np.random.get_state()
    np.random.set_state(mid)
    want = get_minibatch([roidb[i] for i in layer._perm[:2]], K, R.ShapeOnlyBlobCtx())
    direct = np.random.get_state()
    assert bits(after[1]) == bits(direct[1]) and after[2] == direct[2]
    assert sorted(got) == sorted(want) and all(bits(got[k]) == bits(np.asarray(want[k]).astype(np.float32)) for k in want)
    # switched on, the same layer hands over the pool
    monkeypatch.setattr(cfg.TRAIN, "OHEM", True)
    pool = layer.forward()
    assert sorted(pool) == ["data", "labels", "rois", "targets"] and pool["rois"].dtype == np.float32


# ---- configuration, tool, refusal, ABI -------------------------------------------------------------------------------------
def test_cfg_keys_merge_from_yaml(tmp_path, monkeypatch):
    from detect import config
    T = config.cfg.TRAIN
    assert T.OHEM is False and T.OHEM_NMS == 0.7 and T.OHEM_POOL == 2000
    for k in ("OHEM", "OHEM_NMS", "OHEM_POOL"):
        monkeypatch.setattr(T, k, T[k])                                      # (put back afterwards)
    y = tmp_path / "ohem.yml"
    y.write_text("TRAIN:\n  OHEM: True\n  OHEM_NMS: 0.5\n  OHEM_POOL: 300\n")
    config.cfg_from_file(str(y))
    assert T.OHEM is True and T.OHEM_NMS == 0.5 and T.OHEM_POOL == 300
    y.write_text("TRAIN:\n  OHEM_POOL: 0.5\n")
    with pytest.raises(ValueError):
        config.cfg_from_file(str(y))
    text = open(os.path.join(REPO, "az-net_amd", "lib", "detect", "config.py")).read()
    for k in ("OHEM=False", "OHEM_NMS=0.7", "OHEM_POOL=2000"):
        assert re.search(re.escape(k) + r"[,)]\s+# \(not in the reference\)", text), k


def test_ohem_flag_parses_in_the_detection_tool_only(monkeypatch):
    tools = os.path.join(REPO, "az-net_amd", "tools")
    monkeypatch.syspath_prepend(tools)
    import _cli
    import train_az_net
    import train_det_net
    p = _cli.build_parser("t", [train_det_net.COMMON, train_det_net.FLAGS])
    assert p.parse_args(["--iters", "4"]).ohem is False
    a = p.parse_args(["--ohem", "--net", "synthetic:8", "--imdb", "synthetic_375x500_8", "--iters", "4"])
    assert a.ohem is True and a.max_iters == 4
    assert not any(row[0] == "--ohem" for row in _cli.TRAIN_EXT + train_az_net.FLAGS)
    with pytest.raises(SystemExit):
        _cli.build_parser("t", [train_az_net.COMMON, train_az_net.FLAGS]).parse_args(["--ohem"])


def test_more_pool_rows_than_the_trainer_takes_is_refused(ohem_cfg, monkeypatch):
    from aznet_hip import ffi
    from detect.train_det import SolverWrapper

    class Imdb(object):
        num_classes = K
        roidb = []
    assert ffi.DET_MAX_ROIS == 4096
    monkeypatch.setattr(ohem_cfg.TRAIN, "OHEM_POOL", 2049)
    with pytest.raises(ValueError, match="4096"):
        SolverWrapper("no_such_solver.prototxt", Imdb(), "out")
    monkeypatch.setattr(ohem_cfg.TRAIN, "OHEM_POOL", 2048)                    # 4096 rows pass this check (and fail at the file)
    with pytest.raises(Exception) as e:
        SolverWrapper("no_such_solver.prototxt", Imdb(), "out")
    assert "4096" not in str(e.value)
    assert SolverWrapper._max_rois() == 4096
    monkeypatch.setattr(ohem_cfg.TRAIN, "OHEM", False)
    assert SolverWrapper._max_rois() == 8


def test_wrapper_gathers_the_mined_rows_and_names_images_without_a_pool(ohem_cfg):
    """SolverWrapper._mine around a stub of the mining call: the rows it returns are gathered with their targets expanded,
    last_mining is filled, and a batch whose images all have empty pools is a ValueError that names them."""
    from detect.train_det import SolverWrapper
    from roi_data_layer.minibatch import _get_bbox_regression_labels, get_ohem_minibatch

    class Trainer(object):
        def fetch(self, name):
            assert name == "mine_nkeep"
            return np.array([3, 1], np.int32)
    sw = object.__new__(SolverWrapper)
    sw.num_classes, sw.trainer, sw.last_mining, sw.last_sel = K, Trainer(), None, None
    np.random.seed(2)
    pool = get_ohem_minibatch([entry(1, [0.2, 0.3, 0.6, 0.2, 0.7]), entry(2, [0.9, 0.1, 0.1])], K, R.ShapeOnlyBlobCtx())
    pool = {k: np.asarray(v).astype(np.float32) for k, v in pool.items()}
    asked = []

    def mine(rois, labels, targets, thresh, per_image, want):
        asked.append((rois.shape, thresh, per_image, want, targets is not None))
        return np.array([1, 0, 4, 6], np.int32), np.array([3, 1], np.int32), np.arange(8, dtype=np.float32)
    mb = sw._mine(pool, mine)
    assert asked == [((8, 5), 0.7, 4, True, True)]
    sel = [1, 0, 4, 6]
    bt, bw = _get_bbox_regression_labels(np.hstack((pool["labels"][sel, None], pool["targets"][sel])), K)
    assert bits(mb["rois"]) == bits(pool["rois"][sel]) and bits(mb["labels"]) == bits(pool["labels"][sel])
    assert bits(mb["bbox_targets"]) == bits(bt) and bits(mb["bbox_loss_weights"]) == bits(bw) and mb["data"] is pool["data"]
    assert bw[0].sum() == 4 and bw[2].sum() == 0                              # a foreground row, a background row
    assert sw.last_mining == dict(pool=8, kept=[3, 1], selected=[3, 1], fg=2, pool_loss=3.5, mined_loss=2.75)
    assert "pool = 8" in sw._display_extra() and sw.last_sel.tolist() == sel
    empty = dict(pool, rois=pool["rois"][:0], labels=pool["labels"][:0], targets=pool["targets"][:0])
    for fake in (mine, lambda *a: (np.zeros(0, np.int32), np.zeros(2, np.int32), np.zeros(8, np.float32))):
        with pytest.raises(ValueError, match="images 0, 1"):
            sw._mine(empty if fake is mine else pool, fake)
    assert len(asked) == 1                                                    # (an empty pool never reaches the device)


def test_header_binding_and_library_agree_on_the_entries():
    from aznet_hip import ffi
    header = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    L = ffi.load_library()
    for name, nargs in (("az_det_solver_mine", 15), ("az_det_solver_mine_skip", 17)):
        assert name in ffi.SYMBOLS
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and len(m.group(1).split(",")) == nargs
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    for word in ("mine_loss_cls", "mine_loss_bbox", "mine_keep", "mine_nkeep", "FLT_MIN", "must not decrease"):
        assert word in header


# ---- the restatement --------------------------------------------------------------------------------------------------------
def boxes(rng, n, span=200.0):
    x1, y1 = rng.uniform(0, span, n), rng.uniform(0, span, n)
    return np.stack([x1, y1, x1 + rng.uniform(5, span / 2, n), y1 + rng.uniform(5, span / 2, n)], 1).astype(np.float32)


@pytest.mark.parametrize("thresh", [0.0, 0.3, 0.7, 1.0, 1.5])
def test_restatement_nms_equals_the_oracle(thresh):
    import oracle.az_oracle as orc
    rng = np.random.Generator(np.random.PCG64(int(thresh * 10) + 1))
    for n in (1, 2, 17, 300):
        dets = np.hstack((boxes(rng, n), rng.permutation(n)[:, None].astype(np.float32) / n))     # no ties: argsort's order is fixed
        assert O.nms(dets, thresh).tolist() == orc.nms(dets, thresh), (n, thresh)
    assert O.nms(np.zeros((0, 5), np.float32), thresh).size == 0


def test_restatement_ties_duplicates_and_thresholds():
    b = np.array([[0, 0, 9, 9], [0, 0, 9, 9], [100, 100, 120, 120], [0, 0, 9, 9]], np.float32)
    d = np.hstack((b, np.array([[1.0], [1.0], [1.0], [1.0]], np.float32)))
    assert O.nms(d, 0.7).tolist() == [3, 2]                                  # equal scores: the higher index first; duplicates drop
    assert O.nms(d, 1.0).tolist() == [3, 2]                                  # IoU 1 >= 1: an exact duplicate still drops
    assert O.nms(d, 1.5).tolist() == [3, 2, 1, 0]                            # above 1: everything stays, in visiting order
    assert O.nms(d, 0.0).tolist() == [3]                                     # IoU 0 >= 0: one box per image
    d[:, 4] = [0.5, 2.0, 1.0, 2.0]
    assert O.nms(d, 0.7).tolist() == [3, 2]
    rois = np.hstack((np.array([[0], [0], [2], [2]], np.float32), b))        # image 1 owns no row
    sel, n_sel, keeps = O.select(rois, d[:, 4], 3, 0.7, 5)
    assert sel.tolist() == [1, 3, 2] and n_sel.tolist() == [1, 0, 2] and [k.tolist() for k in keeps] == [[1], [], [3, 2]]
    sel, n_sel, _ = O.select(rois, d[:, 4], 3, 0.7, 1)
    assert sel.tolist() == [1, 3] and n_sel.tolist() == [1, 0, 1]
    off = O.image_ranges(rois, 3)
    assert off.tolist() == [0, 2, 2, 4] and O.keep_array(keeps, off, 4).tolist() == [1, -1, 3, 2]
    assert O.image_ranges(rois[2:], 3).tolist() == [0, 0, 0, 2]              # ... nor do images 0 and 1


def test_restatement_row_losses():
    rng = np.random.Generator(np.random.PCG64(8))
    n, ncls = 50, 7
    s, b = rng.standard_normal((n, ncls)) * 3, rng.standard_normal((n, 4 * ncls)) * 2
    lab = rng.integers(0, ncls, n)
    t = rng.standard_normal((n, 4))
    l64, c64, b64 = O.row_losses(s, b, lab, t)
    l32, c32, b32 = O.row_losses(s.astype(np.float32), b.astype(np.float32), lab, t.astype(np.float32), np.float32)
    assert l32.dtype == np.float32 and np.all(b64[lab == 0] == 0) and np.all(b32[lab == 0] == 0)
    assert bits(l32) == bits((c32 + b32).astype(np.float32))
    assert O.rel_err(l32, l64) < 1e-6 and O.rel_err(b32, b64) < 1e-6
    # by hand: one row, label 2, d = (0.5, -2, 1, 0) -> 0.125 + 1.5 + 0.5 + 0
    bp = np.zeros((1, 12), np.float32)
    bp[0, 8:12] = [0.5, -2, 1, 0]
    assert O.bbox_loss32(bp, [2], np.zeros((1, 4), np.float32))[0] == np.float32(2.125)
    assert O.row_losses(np.zeros((1, 3)), bp, [2], None)[2][0] == 0
    assert abs(O.row_losses(np.zeros((1, 3)), bp, [0], None)[0][0] - np.log(3)) < 1e-15
    # the clamp: p[label] underflows
    c = O.cls_loss(np.array([[0.0, 200.0]], np.float32), [0], np.float32)
    assert c[0] == -np.log(np.float32(O.TINY))


def test_planted_case_orders_alike_in_both_precisions():
    """The case the device is held to in float64: the gap between any two row losses of an image is at least 100 x the 8x-rule
    bound x the largest loss, in the float64 and the float32 restatement, and both select the same rows."""
    head, fmap, blobs, info = O.planted_case()
    P = O.PLANT
    counts = [int(np.sum(blobs["rois"][:, 0] == i)) for i in range(2)]
    print("  planted case: %s rows, gap %.3e (bound %.3e), smallest float64 gap %.3e" % (counts, info["gap"], info["bound"], info["smallest"]))
    assert counts[0] >= 257 and 1 <= counts[1] <= 256
    assert np.all(np.diff(blobs["rois"][:, 0]) >= 0)
    for loss in (info["loss64"], info["loss32"].astype(np.float64)):
        for i in range(2):
            v = np.sort(loss[blobs["rois"][:, 0] == i])
            assert np.diff(v).min() >= info["gap"], i
    a = O.select(blobs["rois"], info["loss64"], 2, P["thresh"], P["per_image"])
    b = O.select(blobs["rois"], info["loss32"], 2, P["thresh"], P["per_image"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    assert a[1].tolist() == [P["per_image"]] * 2 and len(a[2][0]) < counts[0]      # NMS does drop rows, the cut does bind
