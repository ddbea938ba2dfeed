"""NumPy restatement of the reference's image-pyramid test path (lib/detect/test.py:27-97, lib/utils/blob.py:13-30) and
pyramid stand-ins for the oracle's nets, shared by the pyramid tests.

  scales_for(shape, targets, max_size)   _get_image_blob's scale factors (test.py:40-50)
  blob_shape(shape, scales)              the padded blob im_list_to_blob builds: [S, 3, max h, max w]
  rois_blob(boxes, scales)               _get_rois_blob + _project_im_rois (level in column 0)
  dedup(rois, dedup)                     np.unique of the feature-space hash (test.py:210-218)
  chunked(boxes, scales, dedup, batch)   both over BATCH_SIZE chunks, as _az_forward / _frcnn_forward run them
"""
import contextlib

import numpy as np


def scales_for(shape, targets, max_size):
    size_min, size_max = min(shape[0], shape[1]), max(shape[0], shape[1])
    out = []
    for t in targets:
        s = float(t) / float(size_min)
        if np.round(s * size_max) > max_size:
            s = float(max_size) / float(size_max)
        out.append(s)
    return np.array(out)


def blob_shape(shape, scales):
    """cv2.resize's dsize (round half to even of dim * scale), then the per-axis maximum."""
    hs = [int(np.round(shape[0] * s)) for s in scales]
    ws = [int(np.round(shape[1] * s)) for s in scales]
    return (len(scales), 3, max(hs), max(ws))


def rois_blob(im_rois, scales):
    im_rois = np.asarray(im_rois, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64)
    if len(scales) > 1:
        widths = im_rois[:, 2] - im_rois[:, 0] + 1
        heights = im_rois[:, 3] - im_rois[:, 1] + 1
        areas = widths * heights
        scaled_areas = areas[:, np.newaxis] * (scales[np.newaxis, :] ** 2)
        diff_areas = np.abs(scaled_areas - 224 * 224)
        levels = diff_areas.argmin(axis=1)[:, np.newaxis]
    else:
        levels = np.zeros((im_rois.shape[0], 1), dtype=np.int64)
    rois = im_rois * scales[levels]
    return np.hstack((levels, rois)).astype(np.float32, copy=False)


def dedup(rois, dedup_boxes):
    v = np.array([1, 1e3, 1e6, 1e9, 1e12])
    hashes = np.round(rois * dedup_boxes).dot(v)
    _, index, inv = np.unique(hashes, return_index=True, return_inverse=True)
    return index, inv.ravel()


def chunked(boxes, scales, dedup_boxes, batch):
    """(rois [P,5], index [U] and inverse [P] in the device entry's numbering: chunk c's unique rows follow those of the
    chunks before it, indices are global)."""
    rois = rois_blob(boxes, scales) if len(boxes) else np.zeros((0, 5), np.float32)
    index, inv, off = [], [], 0
    for s in range(0, len(boxes), batch):
        i, v = dedup(rois[s:s + batch], dedup_boxes)
        index.append(i + s)
        inv.append(v + off)
        off += len(i)
    cat = lambda a, t: np.concatenate(a).astype(t) if a else np.zeros((0,), t)   # noqa: E731
    return rois, cat(index, np.int64), cat(inv, np.int64)


def pool_pyramid(orc, maps, rois):
    """RoIPool of each roi on the map of its level (column 0), Caffe's [R, C*49] flattening.  maps: [S, C, H, W]."""
    rois = np.asarray(rois, dtype=np.float32)
    out = None
    for lv in range(maps.shape[0]):
        sel = np.where(rois[:, 0] == lv)[0]
        if not len(sel):
            continue
        r = rois[sel].copy()
        r[:, 0] = 0
        p = orc.roi_pool(maps[lv], r)
        if out is None:
            out = np.zeros((rois.shape[0], p.shape[1]), dtype=np.float32)
        out[sel] = p
    if out is None:
        out = np.zeros((rois.shape[0], maps.shape[1] * 49), dtype=np.float32)
    return out


class PyramidNet(object):
    """pycaffe-shaped AZ net over a fixed pyramid of maps [S, C, H, W] for the oracle's level loop: RoIPool on each roi's
    level, then the oracle's fc head (orc.head_forward's layers)."""

    class _Blob(object):
        def reshape(self, *shape):
            self.shape = shape

    def __init__(self, orc, head, maps):
        self.orc, self.head, self.maps = orc, head, maps
        self.blobs = {k: self._Blob() for k in ("data", "rois", "conv5_3")}
        self.rec = []

    def __getitem__(self, k):
        return self

    def __contains__(self, k):
        return k in ("full", "fc")

    def keys(self):
        return ["full", "fc"]

    def forward(self, blobs=None, **kw):
        orc, h = self.orc, self.head
        rois = kw["rois"]
        self.rec.append(np.array(rois, dtype=np.float32))
        pool5 = pool_pyramid(orc, self.maps, rois)
        h6 = orc.fc(pool5, h["W6"], h["b6"], True)
        h71 = orc.fc(h6, h["W71"], h["b71"], True)
        h72 = orc.fc(h6, h["W72"], h["b72"], True)
        out = {"zoom_prob": orc.sigmoid(orc.fc(h72, h["Wz"], h["bz"], False)),
               "adj_prob": orc.sigmoid(orc.fc(h71, h["Was"], h["bas"], False)),
               "adj_bbox": orc.fc(h71, h["Wab"], h["bab"], False)}
        for b in blobs or []:
            out[b] = self.maps
        return out


class PyramidDetNet(object):
    """pycaffe-shaped Fast R-CNN head over a fixed pyramid (the oracle's det head layers)."""

    def __init__(self, orc, head, maps):
        self.orc, self.head, self.maps = orc, head, maps
        self.blobs = {k: PyramidNet._Blob() for k in ("data", "rois", "conv5_3")}

    def __getitem__(self, k):
        return self

    def forward(self, blobs=None, **kw):
        orc, h = self.orc, self.head
        pool5 = pool_pyramid(orc, self.maps, kw["rois"])
        h6 = orc.fc(pool5, h["W6"], h["b6"], True)
        h7 = orc.fc(h6, h["W7"], h["b7"], True)
        return {"cls_prob": orc.softmax(orc.fc(h7, h["Wc"], h["bc"], False)), "bbox_pred": orc.fc(h7, h["Wb"], h["bb"], False)}


@contextlib.contextmanager
def oracle_on_pyramid(orc):
    """The oracle's level loop (orc.im_propose, orc.im_propose_tune, orc.frcnn_forward) with the pyramid projection:
    pass the scale factors array where those functions take `scale`."""
    keep = orc.get_rois_blob
    orc.get_rois_blob = lambda boxes, scales: rois_blob(boxes, np.atleast_1d(np.asarray(scales, dtype=np.float64)))
    try:
        yield
    finally:
        orc.get_rois_blob = keep
