"""The data layer that feeds detection-net training (reference: lib/roi_data_layer/layer.py), without Caffe: `forward()`
returns the five blobs as float32 arrays instead of copying them into a net's tops."""
import numpy as np

from az_data_layer.layer import AZDataLayer
from detect.config import cfg
from roi_data_layer.minibatch import get_minibatch, get_ohem_minibatch

BLOB_NAMES = ("data", "rois", "labels", "bbox_targets", "bbox_loss_weights")
OHEM_BLOB_NAMES = ("data", "rois", "labels", "targets")      # under TRAIN.OHEM: the whole pool, compact targets


class RoIDataLayer(AZDataLayer):
    get_minibatch = staticmethod(get_minibatch)
    get_ohem_minibatch = staticmethod(get_ohem_minibatch)

    def __init__(self, num_classes, ctx=None):
        super(RoIDataLayer, self).__init__(num_classes, ctx)

    def set_roidb(self, roidb):
        if cfg.TRAIN.USE_PREFETCH:
            raise NotImplementedError("cfg.TRAIN.USE_PREFETCH is not supported: the blobs are made in the training process")
        super(RoIDataLayer, self).set_roidb(roidb)

    def forward(self):
        if not cfg.TRAIN.OHEM:
            return super(RoIDataLayer, self).forward()
        db_inds = self._get_next_minibatch_inds()
        blobs = self.get_ohem_minibatch([self._roidb[i] for i in db_inds], self._num_classes, self._ctx)
        return {k: np.asarray(v).astype(np.float32, copy=False) for k, v in blobs.items()}
