"""The data layer that feeds detection-net training (reference: lib/roi_data_layer/layer.py), without Caffe: `forward()`
returns the five blobs as float32 arrays instead of copying them into a net's tops."""
from az_data_layer.layer import AZDataLayer
from detect.config import cfg
from roi_data_layer.minibatch import get_minibatch

BLOB_NAMES = ("data", "rois", "labels", "bbox_targets", "bbox_loss_weights")


class RoIDataLayer(AZDataLayer):
    get_minibatch = staticmethod(get_minibatch)

    def __init__(self, num_classes, ctx=None):
        super(RoIDataLayer, self).__init__(num_classes, ctx)

    def set_roidb(self, roidb):
        if cfg.TRAIN.USE_PREFETCH:
            raise NotImplementedError("cfg.TRAIN.USE_PREFETCH is not supported: the blobs are made in the training process")
        super(RoIDataLayer, self).set_roidb(roidb)
