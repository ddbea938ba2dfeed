"""Train the detection net (reference: lib/detect/train_det.py) without Caffe: PyTorch-ROCm runs the VGG16 convolutions with
autograd, everything from conv5_3 on -- RoIPool, fc6 / fc7 / cls_score / bbox_pred forward and backward, dropout, the softmax
and SmoothL1 losses, the gradient norm and the SGD update -- is the HIP trainer behind az_det_solver_*
(aznet_hip.ffi.AzDetSolver).  What it shares with detect/train_az.py is in detect/solver.py.
Under a skip configuration (cfg.SEAR.FRCNN_CONV names several maps: the rule of detect.test) the trainer carries the
skip-connection front -- roi_pool3/4/5, GRN, concat, scale, conv_pool5 -- and autograd starts at the three tapped maps."""
import numpy as np

import roi_data_layer.roidb as rdl_roidb
from aznet_hip import ffi
from detect import prototxt, solver
from detect.config import cfg

HEAD_OF = {"fc6": ("W6", "b6"), "fc7": ("W7", "b7"), "cls_score": ("Wc", "bc"), "bbox_pred": ("Wb", "bb")}


def _fc_blobs(layers, name):
    w, b = layers[name][0], layers[name][1]
    b = np.ascontiguousarray(b.ravel(), dtype=np.float32)
    return np.ascontiguousarray(w.reshape(b.size, -1), dtype=np.float32), b


class SolverWrapper(solver.SolverWrapper):
    """What the reference's wrapper around caffe.SGDSolver does (train_det.py:24-112): the box-regression targets and their
    means / stds, the data layer, the TRAIN.UN_NORMALIZE re-initialisation of bbox_pred, the training loop and the snapshots
    with un-normalised bbox_pred weights.
    backbone: a VGG16Conv5 (default: built from pretrained_model, or seeded); trainer: an AzDetSolver (default: created on
    `ctx` with the head's sizes -- `dims` or the pretrained model's or VGG16's); seed: the dropout / filler seed."""
    HEAD_OF, HEAD_KEYS, DROPOUT_OF = HEAD_OF, ffi.DET_HEAD_KEYS, prototxt.DET_DROPOUT_OF
    FILLER_STD = {k: v or prototxt.DET_FILLER_DEFAULT for k, v in prototxt.DET_FILLER_STD.items()}
    BBOX_KEYS = ("Wb", "bb")
    LOSS_NAMES = ("loss_cls", "loss_bbox")
    STATE_KIND = "det"

    def __init__(self, solver_prototxt, imdb, output_dir, pretrained_model=None, backbone=None, trainer=None, ctx=None,
                 dims=None, seed=None):
        self.num_classes = int(imdb.num_classes)
        self.last_mining = self.last_sel = None          # of the last mining pass (TRAIN.OHEM): its figures, the rows it chose
        if cfg.TRAIN.OHEM and int(cfg.TRAIN.IMS_PER_BATCH) * int(cfg.TRAIN.OHEM_POOL) > ffi.DET_MAX_ROIS:
            raise ValueError("TRAIN.OHEM: IMS_PER_BATCH * OHEM_POOL = %d * %d rows, the trainer takes %d at most"
                             % (cfg.TRAIN.IMS_PER_BATCH, cfg.TRAIN.OHEM_POOL, ffi.DET_MAX_ROIS))
        # the configuration and the train net must name the same model (checked before any device work)
        net_file = self._read_solver(solver_prototxt)
        self.skip = None
        if len(cfg.SEAR.FRCNN_CONV) > 1:
            try:
                self.net_param, self.skip = prototxt.read_skip_train_net(net_file)
            except ValueError as e:
                raise ValueError("cfg.SEAR.FRCNN_CONV = %s names the skip-connection detector's maps, but the train net is "
                                 "not its net: %s" % (list(cfg.SEAR.FRCNN_CONV), e))
            if list(self.skip["sources"]) != list(cfg.SEAR.FRCNN_CONV):
                raise ValueError("the train net pools %s, cfg.SEAR.FRCNN_CONV names %s" % (list(self.skip["sources"]), list(cfg.SEAR.FRCNN_CONV)))
        else:
            try:
                self.net_param = prototxt.read_det_train_net(net_file)
            except ValueError as e:
                if "conv_pool5" in str(e):
                    raise ValueError("the train net has the skip front (conv_pool5), but cfg.SEAR.FRCNN_CONV = %s names one map: "
                                     "use the skip configuration (voc_skip.yml): %s" % (list(cfg.SEAR.FRCNN_CONV), e))
                raise
        print("Computing bounding-box regression targets...")
        self.bbox_means, self.bbox_stds = rdl_roidb.add_bbox_regression_targets(imdb.roidb, self.num_classes)
        print("done")
        super(SolverWrapper, self).__init__(output_dir, pretrained_model, backbone, trainer, ctx, dims, seed)
        if cfg.TRAIN.BBOX_REG and cfg.TRAIN.UN_NORMALIZE:
            self._normalize_bbox_layer()
        from roi_data_layer.layer import RoIDataLayer
        self.layer = RoIDataLayer(self.num_classes, ctx=self.ctx)
        self.layer.set_roidb(imdb.roidb)

    def _build(self, layers, dims):
        from aznet_hip import synth
        self._default_device(layers)
        if dims is None:
            dims = {k: v for k, v in synth.FULL_DET_DIMS.items() if k in ("n6", "n7")}
            if layers and "fc6" in layers and "fc7" in layers:
                dims = dict(n6=layers["fc6"][1].size, n7=layers["fc7"][1].size)
        self.trainer = ffi.AzDetSolver(self.ctx, self.backbone.out_channels, dims["n6"], dims["n7"], self.num_classes,
                                       max_rois=self._max_rois(), seed=self.seed)
        self._load_fillers()
        self._copy_from(layers)

    @staticmethod
    def _max_rois():
        """Rows of the largest pass: a minibatch, or under TRAIN.OHEM the pools of a batch's images."""
        if cfg.TRAIN.OHEM:
            return max(int(cfg.TRAIN.BATCH_SIZE), int(cfg.TRAIN.IMS_PER_BATCH) * int(cfg.TRAIN.OHEM_POOL))
        return int(cfg.TRAIN.BATCH_SIZE)

    def _attach_skip(self):
        """The front of the train net on the trainer: scales and gain as the file states them, eps the library's."""
        if self.skip is None or getattr(self.trainer, "skip", None) is not None:
            return
        conv = {layer[0]: layer[1] for layer in self.backbone.layers if layer is not None}
        missing = [n for n in self.skip["sources"] if n not in conv]
        if missing:
            raise ValueError("the train net pools %s, which the backbone does not have" % ", ".join(missing))
        self.trainer.attach_skip([int(conv[n].shape[0]) for n in self.skip["sources"]], self.skip["scales"],
                                 gain=self.skip["gain"], eps=1e-10, seed=self.seed)

    def _copy_from(self, layers):
        """The skip front onto the trainer, then net.copy_from: the head layers the pretrained model (layers, or None) has, by
        name (an ImageNet VGG16 brings fc6 and fc7 only)."""
        self._attach_skip()
        if not layers:
            return
        head = {}
        for lname, (wk, bk) in HEAD_OF.items():
            if lname in layers:
                head[wk], head[bk] = _fc_blobs(layers, lname)
        shp = self.trainer._shapes()
        bad = [k for k, v in head.items() if v.shape != shp[k]]
        if bad:
            raise ValueError("pretrained model: %s of shape %s, the trainer holds %s" % (bad[0], head[bad[0]].shape, shp[bad[0]]))
        if head:
            self.trainer.load(head)
        if self.skip is not None and "conv_pool5" in layers:          # (a model without it keeps the xavier fill)
            from aznet_hip import caffemodel as cm
            front = cm.skip_front_from_layers(layers, Cs=self.trainer.skip["Cs"])
            if front["Wp"].shape != shp["Wp"]:
                raise ValueError("pretrained model: conv_pool5 of shape %s, the trainer holds %s" % (front["Wp"].shape, shp["Wp"]))
            self.trainer.load_skip(front)

    def _configure(self):
        super(SolverWrapper, self)._configure()
        if self.skip is not None:
            self.trainer.set_skip_hyper(self.net_param["conv_pool5"]["lr_mult"], self.net_param["conv_pool5"]["decay_mult"])

    def _state_kind(self):
        return "det_skip" if self.skip is not None else "det"

    def _forward_backward(self, blobs, it):
        """One minibatch through the convolutions and the trainer (dropout iteration `it`): (losses, the sum of squares of
        the trainer's gradients, the call that takes the map gradients through the trainable convolutions)."""
        import torch
        if self.skip is not None:
            conv, taps = self.backbone.forward_train(blobs["data"], taps=tuple(self.skip["sources"]))
            maps = [t.detach() for t in taps]
            if cfg.TRAIN.OHEM:
                blobs = self._mine(blobs, lambda *a: self.trainer.mine_skip(maps, *a))
            # (a tap in front of the first trainable convolution takes no gradient: no buffer, no gather)
            dmaps = [torch.empty_like(m) if t.requires_grad else None for m, t in zip(maps, taps)] if self.conv_train else None
            if dmaps is not None and all(d is None for d in dmaps):
                dmaps = None
            losses, sumsq = self.trainer.step_skip(maps, blobs["rois"], blobs["labels"], blobs["bbox_targets"],
                                                   blobs["bbox_loss_weights"], self.seed, it, dmaps=dmaps)
            self.last_maps, self.last_dmaps = maps, dmaps

            def backward():
                if dmaps is not None:
                    torch.autograd.backward([t for t, d in zip(taps, dmaps) if d is not None], [d for d in dmaps if d is not None])
        else:
            conv = self.backbone.forward_train(blobs["data"])
            if cfg.TRAIN.OHEM:
                blobs = self._mine(blobs, lambda *a: self.trainer.mine(conv.detach(), *a))
            dmap = torch.empty_like(conv) if self.conv_train else None
            losses, sumsq = self.trainer.step(conv.detach(), blobs["rois"], blobs["labels"], blobs["bbox_targets"],
                                              blobs["bbox_loss_weights"], self.seed, it, dmap=dmap)

            def backward():
                conv.backward(dmap)
        self.last_conv, self.last_blobs = conv.detach(), blobs
        return losses, sumsq, backward

    def _mine(self, pool, mine):
        """TRAIN.OHEM: the minibatch that the trainer's mining pass picks from the pool blobs (roi_data_layer.minibatch.
        get_ohem_minibatch) on the maps of this iteration -- the BATCH_SIZE // IMS_PER_BATCH rows of highest loss per image
        that survive NMS at OHEM_NMS --, gathered on the host with the targets expanded; notes the pass in last_mining."""
        from roi_data_layer.minibatch import _get_bbox_regression_labels
        n_im = int(pool["data"].shape[0])
        per_image = int(cfg.TRAIN.BATCH_SIZE) // n_im
        rois, labels, targets = pool["rois"], pool["labels"], pool["targets"]
        sel = np.zeros(0, np.int32)
        if rois.shape[0] > 0:
            sel, n_sel, loss = mine(rois, labels, targets if cfg.TRAIN.BBOX_REG else None, float(cfg.TRAIN.OHEM_NMS), per_image, True)
        if sel.size == 0:
            raise ValueError("TRAIN.OHEM: no row selected in any of the batch's images %s (their pools are empty: no proposal "
                             "at or above FG_THRESH or below it)" % ", ".join(str(i) for i in range(n_im)))
        lab = labels[sel]
        bbox_targets, bbox_loss_weights = _get_bbox_regression_labels(np.hstack((lab[:, np.newaxis], targets[sel])), self.num_classes)
        self.last_mining = dict(pool=int(rois.shape[0]), kept=[int(k) for k in self.trainer.fetch("mine_nkeep")],
                                selected=[int(k) for k in n_sel], fg=int(np.count_nonzero(lab > 0)),
                                pool_loss=float(np.mean(loss, dtype=np.float64)), mined_loss=float(np.mean(loss[sel], dtype=np.float64)))
        self.last_sel = sel
        return {"data": pool["data"], "rois": np.ascontiguousarray(rois[sel]), "labels": np.ascontiguousarray(lab),
                "bbox_targets": bbox_targets, "bbox_loss_weights": bbox_loss_weights}

    def _display_extra(self):
        m = self.last_mining
        if not cfg.TRAIN.OHEM or m is None:
            return None
        return ("mining: pool = {:d}, kept = {}, selected = {} ({:d} fg), pool loss = {:.6g}, mined loss = {:.6g}"
                .format(m["pool"], m["kept"], m["selected"], m["fg"], m["pool_loss"], m["mined_loss"]))

    def _snapshot_extra(self):
        if self.skip is None:
            return {}
        f = self.trainer.read_skip()
        return {"conv_pool5": [f["Wp"].reshape(f["Wp"].shape[0], f["Wp"].shape[1], 1, 1), f["bp"]]}


def get_training_roidb(imdb, net=None):
    """A roidb for use in training (train_det.py:118-129); `net` makes the proposals where no proposals.pkl exists."""
    return solver.get_training_roidb(rdl_roidb, imdb, net)


train_net = SolverWrapper.train_net
