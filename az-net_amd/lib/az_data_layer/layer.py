"""The data layer that feeds AZ-net training (reference: lib/az_data_layer/layer.py), without Caffe: `forward()`
returns the six blobs as float32 arrays instead of copying them into a net's tops."""
import numpy as np

from az_data_layer.minibatch import get_minibatch
from detect.config import cfg

BLOB_NAMES = ("data", "rois", "adj_labels", "adj_targets", "adj_loss_weights", "zoom_labels")


class AZDataLayer(object):
    """The shuffling layer, written once: roi_data_layer.layer.RoIDataLayer is this class with its own get_minibatch."""
    get_minibatch = staticmethod(get_minibatch)

    def __init__(self, num_classes=None, ctx=None):
        self._num_classes = int(num_classes if num_classes is not None else cfg.SEAR.NUM_SUBREG)
        self._ctx = ctx

    def _shuffle_roidb_inds(self):
        """Randomly permute the training roidb (layer.py:27-30)."""
        self._perm = np.random.permutation(np.arange(len(self._roidb)))
        self._cur = 0

    def _get_next_minibatch_inds(self):
        """The roidb indices of the next minibatch (layer.py:32-39)."""
        if self._cur + cfg.TRAIN.IMS_PER_BATCH >= len(self._roidb):
            self._shuffle_roidb_inds()
        db_inds = self._perm[self._cur:self._cur + cfg.TRAIN.IMS_PER_BATCH]
        self._cur += cfg.TRAIN.IMS_PER_BATCH
        return db_inds

    def set_roidb(self, roidb):
        self._roidb = roidb
        self._shuffle_roidb_inds()

    def forward(self):
        db_inds = self._get_next_minibatch_inds()
        blobs = self.get_minibatch([self._roidb[i] for i in db_inds], self._num_classes, self._ctx)
        return {k: np.asarray(v).astype(np.float32, copy=False) for k, v in blobs.items()}
