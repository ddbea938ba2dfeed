"""Transform a roidb into a trainable roidb for the detection net (reference: lib/roi_data_layer/roidb.py).

`prepare_roidb` adds every image's example boxes -- the AZ-net's proposals stacked on the ground truth -- with
'gt_boxes', 'gt_labels' and 'image'; `add_bbox_regression_targets` the compact box-regression targets [E,5] and
'max_overlaps', normalised by per-class means and stds over the whole roidb.  The per-box work of the latter
(roidb.py:104-207) runs on the GPU (az_det_targets, az_det_target_stats; csrc/az_det_train.hip); this module keeps the
reference's roidb keys and dtypes and its proposals cache."""
import os
import pickle

import numpy as np

from detect.config import cfg, get_output_dir

_backend = None          # what answers the device entry points; None: aznet_hip.ffi.default_context()
CHUNK = 256              # images per az_det_targets call


def set_backend(b):
    """Route the device calls to `b` (an object with AzContext's det_targets / det_target_stats); None restores the GPU."""
    global _backend
    _backend = b


def _ctx():
    if _backend is not None:
        return _backend
    from aznet_hip import ffi
    return ffi.default_context()


def _mirror(boxes, im_width):
    """The boxes of the horizontally flipped image."""
    x1, x2 = boxes[:, 0].copy(), boxes[:, 2].copy()
    out = boxes.copy()
    out[:, 0] = im_width - x2 - 1
    out[:, 2] = im_width - x1 - 1
    return out


def _ground_truth(entry):
    """(boxes, labels) of an entry's objects: the rows whose gt_overlaps reach 1 where the entry has gt_overlaps
    (roidb.py:68-76), else every row with its gt_classes (this project's roidbs hold ground truth only)."""
    if "gt_overlaps" in entry:
        ov = entry["gt_overlaps"]
        ov = ov.toarray() if hasattr(ov, "toarray") else np.asarray(ov)
        inds = np.where(ov.max(axis=1) == 1)[0]
        return entry["boxes"][inds, :], ov.argmax(axis=1)[inds]
    return entry["boxes"], np.asarray(entry["gt_classes"])


def _propose(net, entry):
    """The AZ-net's regions for one image (roidb.py:209-216): Train mode, cfg.SEAR.NUM_PROPOSALS = TRAIN.NUM_PROPOSALS."""
    from az_data_layer.minibatch import _image_of
    from detect.test import im_propose
    return np.asarray(im_propose(net, _image_of(entry), num_proposals=cfg.SEAR.NUM_PROPOSALS))


def prepare_roidb(imdb, net):
    """Enrich the imdb's roidb with 'image', 'ex_boxes' [E,4] f32 (proposals, then the objects), 'gt_boxes' [N,4] f32 and
    'gt_labels' [N] (roidb.py:27-102).  The proposals of the unflipped images come from proposals.pkl under
    get_output_dir(imdb, net) when it exists, else from `net` (a HipAZNet or the reference's {'full': net}), and are
    written there; flipped entries mirror their originals."""
    n_all = len(imdb.image_index)
    num_images = n_all // 2 if cfg.TRAIN.USE_FLIPPED else n_all
    full = net["full"] if isinstance(net, dict) else net
    output_dir = get_output_dir(imdb, full)
    cache_file = os.path.join(output_dir, "proposals.pkl")
    prop = [[] for _ in range(num_images)]
    use_loaded = os.path.exists(cache_file)
    if use_loaded:
        with open(cache_file, "rb") as f:
            prop = pickle.load(f)
        print("{} proposals loaded from {}".format(imdb.name, cache_file))
    roidb = imdb.roidb
    for i in range(n_all):
        if i % 20 == 0:
            print("Processing {}/{} ...".format(i, n_all))
        e = roidb[i]
        e["image"] = imdb.image_path_at(i)
        size = imdb.image_size(i)
        e["height"], e["width"] = int(size[0]), int(size[1])          # (for images generated from a seed)
        if e["flipped"]:
            src = roidb[i - num_images]
            e["ex_boxes"] = _mirror(src["ex_boxes"], size[1]).astype(np.float32, copy=False)
            e["gt_boxes"] = _mirror(src["gt_boxes"], size[1]).astype(np.float32, copy=False)
            e["gt_labels"] = src["gt_labels"]
            continue
        gt_rois, labels = _ground_truth(e)
        assert all(labels != 0), "an object of the background class"
        if not use_loaded:
            prop[i] = _propose(net, e)
        regions = np.asarray(prop[i]).reshape(-1, 4)
        prop[i] = regions.astype(np.float32, copy=False)
        e["ex_boxes"] = np.vstack((regions, gt_rois)).astype(np.float32, copy=False)
        e["gt_boxes"] = gt_rois.astype(np.float32, copy=False)
        e["gt_labels"] = labels
        assert e["ex_boxes"].shape[0] > 0, "no example boxes"
    if not use_loaded:
        os.makedirs(output_dir, exist_ok=True)
        with open(cache_file, "wb") as f:
            pickle.dump(prop, f, pickle.HIGHEST_PROTOCOL)
        print("wrote roidb (proposals) to {}".format(cache_file))


def add_bbox_regression_targets(roidb, num_classes=None):
    """Add 'bbox_targets' [E,5] f32 (label, dx, dy, dw, dh; normalised) and 'max_overlaps' [E] to every entry and return
    (means.ravel(), stds.ravel()) of the four deltas per class (roidb.py:104-147).  num_classes: the columns of
    gt_overlaps where the roidb has them, else cfg-independent: the caller's (imdb.num_classes)."""
    assert len(roidb) > 0
    assert "gt_labels" in roidb[0], "Did you call prepare_roidb first?"
    if num_classes is None:
        num_classes = roidb[0]["gt_overlaps"].shape[1]
    ctx = _ctx()
    n = len(roidb)
    parts, overlaps = [], []
    for s in range(0, n, CHUNK):
        idx = range(s, min(n, s + CHUNK))
        off = np.zeros(len(idx) + 1, dtype=np.int32)
        off[1:] = np.cumsum([roidb[i]["ex_boxes"].shape[0] for i in idx])
        ex = np.vstack([roidb[i]["ex_boxes"] for i in idx])
        t, mo = ctx.det_targets(ex, off, [roidb[i]["gt_boxes"] for i in idx], [roidb[i]["gt_labels"] for i in idx],
                                float(cfg.TRAIN.BBOX_THRESH), float(cfg.TRAIN.BG_THRESH_LO), float(cfg.EPS))
        parts.append(t)
        overlaps.append(mo)
    targets = np.ascontiguousarray(np.vstack(parts), dtype=np.float32)
    overlaps = np.concatenate(overlaps)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([e["ex_boxes"].shape[0] for e in roidb])
    _, means, stds = ctx.det_target_stats(targets, off, int(num_classes), float(cfg.EPS), True)
    for i, e in enumerate(roidb):
        e["bbox_targets"] = targets[off[i]:off[i + 1]].copy()
        mo = overlaps[off[i]:off[i + 1]]
        # (the reference's dtypes: float64 IoUs, the float32 constant for an image without objects, roidb.py:160-163)
        e["max_overlaps"] = mo.astype(np.float32) if e["gt_boxes"].shape[0] == 0 else mo.copy()
    return means.ravel(), stds.ravel()
