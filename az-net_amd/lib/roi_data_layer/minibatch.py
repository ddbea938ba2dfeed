"""Compute minibatch blobs for training the detection net (reference: lib/roi_data_layer/minibatch.py).  Sampling and the
4-of-4K expansion of the compact targets are host NumPy: a gather of 128 rows per batch, interleaved with np.random's
calls, whose order is part of the reference's behaviour (DESIGN §4t argues the same for the AZ layer)."""
import numpy as np
import numpy.random as npr

from az_data_layer.minibatch import _get_image_blob, _project_im_rois
from detect.config import cfg


def get_minibatch(roidb, num_classes, ctx=None):
    """The blobs of one minibatch over the given roidb entries (minibatch.py:16-65): np.random is asked for the scale
    indices first, then per image for its foreground and its background rows."""
    n = len(roidb)
    scale_inds = npr.randint(0, high=len(cfg.TRAIN.SCALES), size=n)
    if cfg.TRAIN.BATCH_SIZE % n != 0:
        raise ValueError("TRAIN.BATCH_SIZE = {} is no multiple of the {} images of a batch".format(cfg.TRAIN.BATCH_SIZE, n))
    per_image = cfg.TRAIN.BATCH_SIZE // n
    fg_per_image = int(np.round(cfg.TRAIN.FG_FRACTION * per_image))
    im_blob, im_scales = _get_image_blob(roidb, scale_inds, ctx)
    rois, labels, targets, weights = [], [], [], []
    for i, entry in enumerate(roidb):
        lab, _, boxes, tgt, wgt = _sample_rois(entry, fg_per_image, per_image, num_classes)
        boxes = _project_im_rois(boxes, im_scales[i])
        rois.append(np.hstack((np.full((boxes.shape[0], 1), float(i)), boxes)))
        labels.append(lab), targets.append(tgt), weights.append(wgt)
    blobs = {"data": im_blob, "rois": np.vstack(rois), "labels": np.hstack(labels).astype(np.float32, copy=False)}
    if cfg.TRAIN.BBOX_REG:
        blobs["bbox_targets"] = np.vstack(targets)
        blobs["bbox_loss_weights"] = np.vstack(weights)
    return blobs


def ohem_pool_inds(entry):
    """The pool rows of one roidb entry under TRAIN.OHEM: (indices, number of foreground rows among them).  The foreground
    (max_overlaps >= FG_THRESH) in roidb order, then the background ([BG_THRESH_LO, BG_THRESH_HI), with _sample_rois'
    fall-back when that band is empty) in roidb order, cut at OHEM_POOL rows: the objects come first, so a long proposal list
    never pushes them out.  FG_FRACTION plays no part, and np.random is not asked."""
    T = cfg.TRAIN
    overlaps = entry["max_overlaps"]
    fg = np.flatnonzero(overlaps >= T.FG_THRESH)
    bg = np.flatnonzero((overlaps < T.BG_THRESH_HI) & (overlaps >= T.BG_THRESH_LO))
    if bg.size == 0:
        bg = np.flatnonzero(overlaps < T.FG_THRESH)
    pool = int(T.OHEM_POOL)
    keep = np.concatenate((fg, bg)).astype(np.int64)[:pool]
    return keep, int(min(fg.size, pool))


def get_ohem_minibatch(roidb, num_classes, ctx=None):
    """The blobs of one minibatch under TRAIN.OHEM: every image's whole pool (ohem_pool_inds) instead of a sample -- data,
    rois (projected, the image index in column 0), labels and the compact targets [R, 4] of each row's own class, which the
    trainer's mining pass reads (detect.train_det).  np.random is asked for the scale indices only."""
    n = len(roidb)
    scale_inds = npr.randint(0, high=len(cfg.TRAIN.SCALES), size=n)
    if cfg.TRAIN.BATCH_SIZE % n != 0:
        raise ValueError("TRAIN.BATCH_SIZE = {} is no multiple of the {} images of a batch".format(cfg.TRAIN.BATCH_SIZE, n))
    im_blob, im_scales = _get_image_blob(roidb, scale_inds, ctx)
    rois, labels, targets = [], [], []
    for i, entry in enumerate(roidb):
        keep, n_fg = ohem_pool_inds(entry)
        compact = entry["bbox_targets"][keep, :]
        lab = compact[:, 0].copy()
        lab[n_fg:] = 0
        boxes = _project_im_rois(entry["ex_boxes"].astype(np.float32, copy=False)[keep], im_scales[i])
        tgt = np.asarray(compact[:, 1:5], dtype=np.float32)
        for a in (boxes, tgt, lab):
            assert np.all(np.isfinite(a)), "nan or inf in a minibatch (a class whose targets have std 0?)"
        rois.append(np.hstack((np.full((boxes.shape[0], 1), float(i)), boxes)))
        labels.append(lab), targets.append(tgt)
    return {"data": im_blob, "rois": np.vstack(rois), "labels": np.hstack(labels).astype(np.float32, copy=False),
            "targets": np.vstack(targets)}


def _sample_rois(roidb, fg_rois_per_image, rois_per_image, num_classes):
    """A random sample of foreground and background example boxes (minibatch.py:67-124).  np.random is asked for a
    choice only when the pool is not empty; an empty [BG_THRESH_LO, BG_THRESH_HI) band falls back to everything below
    FG_THRESH; the labels behind the foreground share are background."""
    T = cfg.TRAIN
    overlaps = roidb["max_overlaps"]
    fg = np.flatnonzero(overlaps >= T.FG_THRESH)
    n_fg = int(min(fg_rois_per_image, fg.size))
    if fg.size > 0:
        fg = npr.choice(fg, size=n_fg, replace=False)
    bg = np.flatnonzero((overlaps < T.BG_THRESH_HI) & (overlaps >= T.BG_THRESH_LO))
    if bg.size == 0:
        bg = np.flatnonzero(overlaps < T.FG_THRESH)
    n_bg = int(min(rois_per_image - n_fg, bg.size))
    if bg.size > 0:
        bg = npr.choice(bg, size=n_bg, replace=False)
    keep = np.concatenate((fg, bg)).astype(np.int64)
    compact = roidb["bbox_targets"][keep, :]
    labels = compact[:, 0].copy()
    labels[n_fg:] = 0
    rois = roidb["ex_boxes"].astype(np.float32, copy=False)[keep]
    bbox_targets, bbox_loss_weights = _get_bbox_regression_labels(compact, num_classes)
    for a in (rois, bbox_targets, bbox_loss_weights, labels):
        assert np.all(np.isfinite(a)), "nan or inf in a minibatch (a class whose targets have std 0?)"
    return labels, overlaps[keep], rois, bbox_targets, bbox_loss_weights


def _get_bbox_regression_labels(bbox_target_data, num_classes):
    """The compact targets [n,5] as the 4-of-4K blobs the net reads: a row's four deltas, and weights of 1, in the columns
    of its class; rows of class 0 stay zero (minibatch.py:153-175)."""
    n = bbox_target_data.shape[0]
    bbox_targets = np.zeros((n, 4 * num_classes), dtype=np.float32)
    bbox_loss_weights = np.zeros((n, 4 * num_classes), dtype=np.float32)
    cls = bbox_target_data[:, 0].astype(np.int64)
    rows = np.where(cls > 0)[0]
    for q in range(4):
        bbox_targets[rows, 4 * cls[rows] + q] = bbox_target_data[rows, 1 + q]
        bbox_loss_weights[rows, 4 * cls[rows] + q] = 1.0
    return bbox_targets, bbox_loss_weights
