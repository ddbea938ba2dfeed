"""The data layer that feeds detection-net training (reference: lib/roi_data_layer/layer.py), without Caffe: `forward()`
returns the five blobs as float32 arrays instead of copying them into a net's tops."""
import numpy as np

from detect.config import cfg
from roi_data_layer.minibatch import get_minibatch

BLOB_NAMES = ("data", "rois", "labels", "bbox_targets", "bbox_loss_weights")


class RoIDataLayer(object):
    def __init__(self, num_classes, ctx=None):
        self._num_classes = int(num_classes)
        self._ctx = ctx

    def _shuffle_roidb_inds(self):
        """Randomly permute the training roidb (layer.py:23-26)."""
        self._perm = np.random.permutation(np.arange(len(self._roidb)))
        self._cur = 0

    def _get_next_minibatch_inds(self):
        """The roidb indices of the next minibatch (layer.py:28-35)."""
        if self._cur + cfg.TRAIN.IMS_PER_BATCH >= len(self._roidb):
            self._shuffle_roidb_inds()
        db_inds = self._perm[self._cur:self._cur + cfg.TRAIN.IMS_PER_BATCH]
        self._cur += cfg.TRAIN.IMS_PER_BATCH
        return db_inds

    def set_roidb(self, roidb):
        if cfg.TRAIN.USE_PREFETCH:
            raise NotImplementedError("cfg.TRAIN.USE_PREFETCH is not supported: the blobs are made in the training process")
        self._roidb = roidb
        self._shuffle_roidb_inds()

    def forward(self):
        db_inds = self._get_next_minibatch_inds()
        blobs = get_minibatch([self._roidb[i] for i in db_inds], self._num_classes, self._ctx)
        return {k: np.asarray(v).astype(np.float32, copy=False) for k, v in blobs.items()}
