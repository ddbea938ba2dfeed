"""Train an AZ-net (reference: lib/detect/train_az.py) without Caffe: PyTorch-ROCm runs the VGG16 convolutions with
autograd, everything from conv5_3 on -- RoIPool, the six InnerProduct layers forward and backward, dropout, the three
losses, the gradient norm and the SGD update -- is the HIP trainer behind az_solver_* (aznet_hip.ffi.AzSolver).
What it shares with detect/train_det.py is in detect/solver.py."""
import az_data_layer.roidb as rdl_roidb
from aznet_hip import ffi
from detect import prototxt, solver
from detect.config import cfg
from detect.solver import clip_scale, learning_rate  # noqa: F401  (detect.train_det and the tests import them from here)

HEAD_OF = {"int6": ("W6", "b6"), "int7_1": ("W71", "b71"), "int7_2": ("W72", "b72"), "adj_score": ("Was", "bas"),
           "adj_bbox": ("Wab", "bab"), "zoom_score": ("Wz", "bz")}


class SolverWrapper(solver.SolverWrapper):
    """What the reference's wrapper around caffe.SGDSolver does (train_az.py:25-116): the adjacency targets and their
    means / stds, the data layer, the TRAIN.UN_NORMALIZE re-initialisation of adj_bbox, the training loop and the
    snapshots with un-normalised adj_bbox weights.
    backbone: a VGG16Conv5 (default: built from pretrained_model, or seeded); trainer: an AzSolver (default: created on
    `ctx` with the head's sizes -- `dims` or the pretrained model's or VGG16's); seed: the dropout / filler seed."""
    HEAD_OF, HEAD_KEYS, DROPOUT_OF, FILLER_STD = HEAD_OF, ffi.HEAD_KEYS, prototxt.DROPOUT_OF, prototxt.FILLER_STD
    BBOX_KEYS = ("Wab", "bab")
    LOSS_NAMES = ("loss_zoom", "loss_adj", "loss_bbox")
    STATE_KIND = "az"

    def __init__(self, solver_prototxt, imdb, output_dir, pretrained_model=None, backbone=None, trainer=None, ctx=None,
                 dims=None, seed=None):
        self.net_param = prototxt.read_train_net(self._read_solver(solver_prototxt))
        print("Computing adjacent prediction targets...")
        self.bbox_means, self.bbox_stds = rdl_roidb.add_adjacent_prediction_targets(imdb)
        print("done")
        super(SolverWrapper, self).__init__(output_dir, pretrained_model, backbone, trainer, ctx, dims, seed)
        if cfg.TRAIN.UN_NORMALIZE:
            self._normalize_bbox_layer()
        from az_data_layer.layer import AZDataLayer
        self.layer = AZDataLayer(ctx=self.ctx)
        self.layer.set_roidb(imdb.roidb)

    def _build(self, layers, dims):
        from aznet_hip import synth, caffemodel as cm
        self._default_device(layers)
        self._refuse_compressed(layers)
        head = cm.az_head_from_layers(layers) if layers and "int6" in layers else None
        if dims is None:
            dims = dict(synth.FULL_DIMS)
            if head is not None:
                dims = dict(n6=head["W6"].shape[0], n71=head["W71"].shape[0], n72=head["W72"].shape[0])
        d = dict(dims, C=self.backbone.out_channels)
        self.trainer = ffi.AzSolver(self.ctx, d["C"], d["n6"], d["n71"], d["n72"], max_rois=int(cfg.TRAIN.BATCH_SIZE),
                                    seed=self.seed, head=head)
        if head is None:
            self._load_fillers()

    @staticmethod
    def _refuse_compressed(layers):
        """The trainers keep full-rank weights: a file whose int6 was compressed (tools/compress_net.py --int6) is refused."""
        if layers and ("int6_L" in layers or "int6_U" in layers):
            raise ValueError("the pretrained model holds int6_L / int6_U, a truncated-SVD int6: train the full-rank net and "
                             "compress its snapshot afterwards (tools/compress_net.py --int6)")

    def _copy_from(self, layers):
        """net.copy_from onto a trainer that was handed in (layers: the pretrained model's, or None)."""
        from aznet_hip import caffemodel as cm
        self._refuse_compressed(layers)
        if layers and "int6" in layers:
            self.trainer.load(cm.az_head_from_layers(layers))

    def _forward_backward(self, blobs, it):
        """One minibatch through the convolutions and the trainer (dropout iteration `it`): (losses, the sum of squares of
        the trainer's gradients, the call that takes d conv5_3 through the trainable convolutions)."""
        import torch
        conv = self.backbone.forward_train(blobs["data"])
        dmap = torch.empty_like(conv) if self.conv_train else None
        losses, sumsq = self.trainer.step(conv.detach(), blobs["rois"], blobs["adj_labels"], blobs["adj_targets"],
                                          blobs["adj_loss_weights"], blobs["zoom_labels"], self.seed, it, dmap=dmap)
        self.last_conv, self.last_blobs = conv.detach(), blobs
        return losses, sumsq, lambda: conv.backward(dmap)


def get_training_roidb(imdb):
    """A roidb for use in training (train_az.py:118-129)."""
    return solver.get_training_roidb(rdl_roidb, imdb)


train_net = SolverWrapper.train_net
