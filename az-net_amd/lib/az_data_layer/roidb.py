"""Transform a roidb into a trainable roidb (reference: lib/az_data_layer/roidb.py).

`prepare_roidb` adds the example regions of a simulated zoom search with label noise and their zoom labels,
`add_adjacent_prediction_targets` the sub-region / object matches with their box-regression targets, normalised by
per-sub-region means and stds over the whole imdb.  The per-image work of both (roidb.py:146-341) runs on the GPU
(az_train_ex_rois, az_train_adj_targets, az_train_target_stats; csrc/az_train.hip); this module keeps the
reference's roidb keys and dtypes, its use of NumPy's global random stream, and the caches.
"""
import os
import pickle

import numpy as np
import numpy.random as npr

from detect.config import cfg

_backend = None          # what answers the device entry points; None: aznet_hip.ffi.default_context()
CHUNK = 64               # images per device call
NOISE_PER_IMAGE = 8192   # first guess of the uniform doubles an image consumes (measured: 1.2-6.5 k; doubled when short)


def set_backend(b):
    """Route the device calls to `b` (an object with AzContext's train_* methods); None restores the GPU context."""
    global _backend
    _backend = b


def _ctx():
    if _backend is not None:
        return _backend
    from aznet_hip import ffi
    return ffi.default_context()


def train_params():
    """The cfg keys the training kernels read (az_train_params)."""
    return dict(min_side=float(cfg.SEAR.MIN_SIDE), train_rep=int(cfg.SEAR.TRAIN_REP),
                zoom_err_prob=float(cfg.SEAR.ZOOM_ERR_PROB), emb_obj_thresh=float(cfg.SEAR.EMB_OBJ_THRESH),
                emb_reg_thresh=float(cfg.SEAR.EMB_REG_THRESH), adj_thresh=float(cfg.SEAR.ADJ_THRESH),
                eps=float(cfg.EPS), addregions=[list(map(float, r)) for r in cfg.TRAIN.ADDREGIONS],
                subregion=[list(map(float, r)) for r in cfg.SEAR.SUBREGION])


def _gt_boxes(entry):
    """Ground truth of an entry: rows with max_overlaps == 1 (roidb.py:51-57) when it has gt_overlaps, else every row
    (this project's ground-truth roidbs carry no gt_overlaps)."""
    if "gt_overlaps" in entry:
        ov = entry["gt_overlaps"]
        ov = ov.toarray() if hasattr(ov, "toarray") else np.asarray(ov)
        return entry["boxes"][np.where(ov.max(axis=1) == 1)[0], :]
    return entry["boxes"]


def _load(path):
    with open(path, "rb") as f:
        return pickle.load(f)


def _ex_rois_chunk(ctx, tp, sizes, gts):
    """One device call for a run of images, drawing from np.random exactly the doubles the reference's level loops
    draw (roidb.py:259): save the state, draw a generous block, run, rewind, draw the consumed count."""
    n_noise = NOISE_PER_IMAGE * len(sizes)
    while True:
        state = npr.get_state()
        noise = npr.random(size=n_noise)
        npr.set_state(state)
        try:
            ex, zoom, off, used = ctx.train_ex_rois(tp, sizes, gts, noise)
        except Exception as e:                       # AzError(AZ_ERR_CAPACITY) carrying .needed: the block was too small
            needed = getattr(e, "needed", None)
            if needed is None:
                raise
            n_noise = max(2 * n_noise, int(needed))
            continue
        total = int(np.sum(used))
        if total:
            npr.random(size=total)
        return ex, zoom, off


def prepare_roidb(imdb):
    """Enrich the imdb's roidb with 'image', 'ex_boxes' [E,4] f32, 'zoom_gt' [E] bool, 'gt_boxes' [N,4] f32
    (roidb.py:23-77)."""
    cache_file = os.path.join(imdb.cache_path, imdb.name + "_trainable_roidb.pkl") if cfg.TRAIN.USE_CACHE else None
    roidb = imdb.roidb
    n = len(imdb.image_index)
    if cache_file and os.path.exists(cache_file):
        caches = _load(cache_file)
        for i in range(n):
            roidb[i]["image"] = imdb.image_path_at(i)
            for k in ("zoom_gt", "ex_boxes", "gt_boxes"):
                roidb[i][k] = caches[k][i]
        print("{} trainable caches loaded from {}".format(imdb.name, cache_file))
    else:
        ctx, tp = _ctx(), train_params()
        for s in range(0, n, CHUNK):
            idx = range(s, min(n, s + CHUNK))
            gts = [np.asarray(_gt_boxes(roidb[i])) for i in idx]
            sizes = [imdb.image_size(i) for i in idx]
            ex, zoom, off = _ex_rois_chunk(ctx, tp, sizes, [g.astype(np.float64) for g in gts])
            for j, i in enumerate(idx):
                roidb[i]["image"] = imdb.image_path_at(i)
                roidb[i]["zoom_gt"] = zoom[off[j]:off[j + 1]].astype(bool)
                roidb[i]["ex_boxes"] = ex[off[j]:off[j + 1]].copy()
                roidb[i]["gt_boxes"] = gts[j].astype(np.float32)
    for i in range(n):
        e = roidb[i]
        e["height"], e["width"] = (int(v) for v in imdb.image_size(i))     # (for images generated from a seed)
        assert np.all(e["ex_boxes"][:, 0] <= e["ex_boxes"][:, 2]), "error in ex_width id={0}".format(i)
        assert np.all(e["ex_boxes"][:, 1] <= e["ex_boxes"][:, 3]), "error in ex_height id={0}".format(i)
        assert np.all(e["gt_boxes"][:, 0] <= e["gt_boxes"][:, 2]), "error in gt_width id={0}".format(i)
        assert np.all(e["gt_boxes"][:, 1] <= e["gt_boxes"][:, 3]), "error in gt_height id={0}".format(i)
    if cache_file and not os.path.exists(cache_file):
        # (per-image lists: the reference pickles the last image's arrays, roidb.py:73-76)
        caches = {k: [roidb[i][k] for i in range(n)] for k in ("zoom_gt", "ex_boxes", "gt_boxes")}
        with open(cache_file, "wb") as f:
            pickle.dump(caches, f, pickle.HIGHEST_PROTOCOL)
        print("wrote trainable caches to {}".format(cache_file))


def add_adjacent_prediction_targets(imdb):
    """Add 'bbox_targets' [T,7] f64 (dx, dy, dw, dh normalised; example region; sub-region; IoU) to every entry and
    return (means.ravel(), stds.ravel()) of the four deltas per sub-region (roidb.py:79-144)."""
    cache_file = os.path.join(imdb.cache_path, imdb.name + "_targets_roidb.pkl") if cfg.TRAIN.USE_CACHE else None
    roidb = imdb.roidb
    assert len(roidb) > 0
    assert "zoom_gt" in roidb[0], "Did you call prepare_roidb first?"
    n = len(roidb)
    num_classes = cfg.SEAR.NUM_SUBREG
    if cache_file and os.path.exists(cache_file):
        caches = _load(cache_file)
        for i in range(n):
            roidb[i]["bbox_targets"] = caches["bbox_targets"][i]
        print("{} targets cache loaded from {}".format(imdb.name, cache_file))
        return caches["means"].ravel(), caches["stds"].ravel()
    ctx, tp = _ctx(), train_params()
    parts, counts = [], []
    for s in range(0, n, CHUNK):
        idx = range(s, min(n, s + CHUNK))
        off = np.zeros(len(idx) + 1, dtype=np.int32)
        off[1:] = np.cumsum([roidb[i]["ex_boxes"].shape[0] for i in idx])
        ex = np.vstack([roidb[i]["ex_boxes"] for i in idx])
        t, toff = ctx.train_adj_targets(tp, ex, off, [roidb[i]["gt_boxes"] for i in idx])
        parts.append(t)
        counts.extend(np.diff(toff).tolist())
    targets = np.ascontiguousarray(np.vstack(parts))
    means, stds = ctx.train_target_stats(num_classes, float(cfg.EPS), targets, True)
    at = 0
    for i in range(n):
        roidb[i]["bbox_targets"] = targets[at:at + counts[i]].copy()
        at += counts[i]
    if cache_file:
        caches = {"bbox_targets": [roidb[i]["bbox_targets"] for i in range(n)], "means": means, "stds": stds}
        with open(cache_file, "wb") as f:
            pickle.dump(caches, f, pickle.HIGHEST_PROTOCOL)
        print("wrote targets cache to {}".format(cache_file))
    return means.ravel(), stds.ravel()
