"""Compute minibatch blobs for training AZ-Net (reference: lib/az_data_layer/minibatch.py).  The expansion of an
image's compact targets into the dense label / target / weight rows is host NumPy: it is a scatter of a few hundred
rows per image, interleaved with np.random's sampling calls, whose order is part of the reference's behaviour."""
import numpy as np
import numpy.random as npr

from detect.config import cfg


def get_minibatch(roidb, num_classes, ctx=None):
    """Given a roidb, construct a minibatch sampled from it (minibatch.py:20-68)."""
    num_images = len(roidb)
    random_scale_inds = npr.randint(0, high=len(cfg.TRAIN.SCALES), size=num_images)
    assert (cfg.TRAIN.BATCH_SIZE % num_images == 0), \
        "num_images ({}) must divide BATCH_SIZE ({})".format(num_images, cfg.TRAIN.BATCH_SIZE)
    rois_per_image = cfg.TRAIN.BATCH_SIZE // num_images
    fg_rois_per_image = int(np.round(cfg.TRAIN.AZ_POS_FRACTION * rois_per_image))

    im_blob, im_scales = _get_image_blob(roidb, random_scale_inds, ctx)

    rois_blob = np.zeros((0, 5), dtype=np.float32)
    adj_labels_blob = np.zeros((0, num_classes), dtype=np.float32)
    adj_targets_blob = np.zeros((0, 4 * num_classes), dtype=np.float32)
    adj_loss_blob = np.zeros(adj_targets_blob.shape, dtype=np.float32)
    zoom_labels_blob = np.zeros((0), dtype=np.float32)
    for im_i in range(num_images):
        adj_labels, zoom_labels, im_rois, adj_targets, adj_loss = \
            _sample_rois(roidb[im_i], fg_rois_per_image, rois_per_image)
        rois = _project_im_rois(im_rois, im_scales[im_i])
        batch_ind = im_i * np.ones((rois.shape[0], 1))
        rois_blob = np.vstack((rois_blob, np.hstack((batch_ind, rois))))
        adj_labels_blob = np.vstack((adj_labels_blob, adj_labels))
        adj_targets_blob = np.vstack((adj_targets_blob, adj_targets))
        adj_loss_blob = np.vstack((adj_loss_blob, adj_loss))
        zoom_labels_blob = np.hstack((zoom_labels_blob, zoom_labels))

    return {"data": im_blob, "rois": rois_blob, "adj_labels": adj_labels_blob, "adj_targets": adj_targets_blob,
            "adj_loss_weights": adj_loss_blob, "zoom_labels": zoom_labels_blob}


def _adj_labels(entry):
    """adj_labels [E, NUM_SUBREG]: 1 (or the match's IoU with SEAR.SCALE_ADJ_CONF) where a target exists
    (minibatch.py:77-86)."""
    adj_labels = np.zeros((entry["ex_boxes"].shape[0], cfg.SEAR.NUM_SUBREG))
    adj_matching = entry["bbox_targets"][:, 4:6].astype(np.uint32, copy=False)
    iou_target = entry["bbox_targets"][:, -1]
    for cls in range(cfg.SEAR.NUM_SUBREG):
        cls_inds = np.where(adj_matching[:, 1] == cls)[0]
        adj_labels[adj_matching[cls_inds, 0], cls] = iou_target[cls_inds] if cfg.SEAR.SCALE_ADJ_CONF else 1
    return adj_labels


def _sample_rois(roidb, fg_rois_per_image, rois_per_image):
    """A random sample of foreground and background example regions (minibatch.py:70-127); the two sets overlap as
    the reference defines them."""
    zoom_labels = roidb["zoom_gt"]
    rois = roidb["ex_boxes"].astype(np.float32, copy=False)
    adj_labels = _adj_labels(roidb)

    fg_inds = np.where((adj_labels.any(axis=1) == 1) | (zoom_labels == 1))[0]
    fg_rois_per_this_image = int(np.minimum(fg_rois_per_image, fg_inds.size))
    if fg_inds.size > 0:
        fg_inds = npr.choice(fg_inds, size=fg_rois_per_this_image, replace=False)

    bg_inds = np.where((adj_labels.any(axis=1) == 0) | (zoom_labels == 0))[0]
    bg_rois_per_this_image = int(np.minimum(rois_per_image - fg_rois_per_this_image, bg_inds.size))
    if bg_inds.size > 0:
        bg_inds = npr.choice(bg_inds, size=bg_rois_per_this_image, replace=False)

    keep_inds = np.append(fg_inds, bg_inds)
    adj_targets, adj_loss_weights = _get_adjacent_targets(roidb["bbox_targets"], keep_inds,
                                                          roidb["ex_boxes"].shape[0], cfg.SEAR.NUM_SUBREG)
    return adj_labels[keep_inds], zoom_labels[keep_inds], rois[keep_inds], adj_targets, adj_loss_weights


def _image_of(entry):
    """BGR uint8 image of a roidb entry: 'synthetic://<seed>' entries are generated, .npy files loaded, anything
    else decoded with PIL (cv2.imread's channel order)."""
    path = entry["image"]
    if path.startswith("synthetic://"):
        from aznet_hip import synth
        return synth.make_image(int(path[len("synthetic://"):]), int(entry["height"]), int(entry["width"]))
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _get_image_blob(roidb, scale_inds, ctx=None):
    """The images at their sampled TRAIN.SCALES, mean-subtracted and resized by the front-end kernel
    (prep_im_for_blob, lib/utils/blob.py:32-45), zero-padded into one [n, 3, H, W] blob (minibatch.py:129-150)."""
    if ctx is None:
        from aznet_hip import ffi
        ctx = ffi.default_context()
    ims, im_scales = [], []
    for i in range(len(roidb)):
        im = _image_of(roidb[i])
        if roidb[i]["flipped"]:
            im = np.ascontiguousarray(im[:, ::-1, :])
        target_size = cfg.TRAIN.SCALES[scale_inds[i]]
        size_min, size_max = min(im.shape[0:2]), max(im.shape[0:2])
        im_scale = float(target_size) / float(size_min)
        if np.round(im_scale * size_max) > cfg.TRAIN.MAX_SIZE:
            im_scale = float(cfg.TRAIN.MAX_SIZE) / float(size_max)
        ims.append(ctx.image_blob(im, cfg.PIXEL_MEANS, im_scale)[0])
        im_scales.append(im_scale)
    shape = np.array([b.shape for b in ims]).max(axis=0)
    blob = np.zeros((len(ims), 3, shape[1], shape[2]), dtype=np.float32)
    for i, b in enumerate(ims):
        blob[i, :, :b.shape[1], :b.shape[2]] = b
    return blob, im_scales


def _project_im_rois(im_rois, im_scale_factor):
    return im_rois * im_scale_factor


def _get_adjacent_targets(compact_targets, keep_inds, num_regions, num_classes):
    """Dense adj_targets / adj_loss_weights [len(keep_inds), 4 * num_classes] f32 (minibatch.py:157-173)."""
    bbox_targets = np.zeros((num_regions, 4 * num_classes), dtype=np.float32)
    bbox_loss_weights = np.zeros((num_regions, 4 * num_classes), dtype=np.float32)
    reg = compact_targets[:, -3].astype(np.int64)
    cls = compact_targets[:, -2].astype(np.int64)
    for q in range(4):
        bbox_targets[reg, 4 * cls + q] = compact_targets[:, q]
        bbox_loss_weights[reg, 4 * cls + q] = 1.0
    return bbox_targets[keep_inds], bbox_loss_weights[keep_inds]
