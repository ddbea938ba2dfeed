"""Train the detection net (reference: lib/detect/train_det.py) without Caffe: PyTorch-ROCm runs the VGG16 convolutions with
autograd, everything from conv5_3 on -- RoIPool, fc6 / fc7 / cls_score / bbox_pred forward and backward, dropout, the softmax
and SmoothL1 losses, the gradient norm and the SGD update -- is the HIP trainer behind az_det_solver_*
(aznet_hip.ffi.AzDetSolver).  Shaped like detect/train_az.py, whose learning-rate and clipping rules it shares.
Under a skip configuration (cfg.SEAR.FRCNN_CONV names several maps: the rule of detect.test) the trainer carries the
skip-connection front -- roi_pool3/4/5, GRN, concat, scale, conv_pool5 -- and autograd starts at the three tapped maps."""
import os

import numpy as np

import roi_data_layer.roidb as rdl_roidb
from detect import prototxt
from detect.config import cfg
from detect.train_az import clip_scale, learning_rate
from utils.timer import Timer

HEAD_OF = {"fc6": ("W6", "b6"), "fc7": ("W7", "b7"), "cls_score": ("Wc", "bc"), "bbox_pred": ("Wb", "bb")}


def _fc_blobs(layers, name):
    w, b = layers[name][0], layers[name][1]
    b = np.ascontiguousarray(b.ravel(), dtype=np.float32)
    return np.ascontiguousarray(w.reshape(b.size, -1), dtype=np.float32), b


class SolverWrapper(object):
    """What the reference's wrapper around caffe.SGDSolver does (train_det.py:24-112): the box-regression targets and their
    means / stds, the data layer, the TRAIN.UN_NORMALIZE re-initialisation of bbox_pred, the training loop and the snapshots
    with un-normalised bbox_pred weights.
    backbone: a VGG16Conv5 (default: built from pretrained_model, or seeded); trainer: an AzDetSolver (default: created on
    `ctx` with the head's sizes -- `dims` or the pretrained model's or VGG16's); seed: the dropout / filler seed."""

    def __init__(self, solver_prototxt, imdb, output_dir, pretrained_model=None, backbone=None, trainer=None, ctx=None,
                 dims=None, seed=None):
        self.output_dir = output_dir
        self.num_classes = int(imdb.num_classes)
        # the configuration and the train net must name the same model (checked before any device work)
        self.solver_param = prototxt.read_solver(solver_prototxt)
        net_file = prototxt.resolve_train_net(solver_prototxt, self.solver_param["train_net"])
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
        self.seed = int(cfg.RNG_SEED if seed is None else seed)
        self.iter = 0
        self.losses = []                       # (loss_cls, loss_bbox) of every iteration
        layers = None
        if pretrained_model is not None:
            print("Loading pretrained model weights from {:s}".format(pretrained_model))
            from aznet_hip import caffemodel as cm
            layers = cm.load_caffemodel(pretrained_model)
        self.ctx = ctx
        self.backbone = backbone
        self.trainer = trainer
        if self.trainer is None:
            self._build(layers, dims)
        else:
            self._attach_skip()
            if layers is not None:
                self._copy_from(layers)
        self._configure()
        if cfg.TRAIN.BBOX_REG and cfg.TRAIN.UN_NORMALIZE:
            # scale and shift bbox_pred into the normalised targets' units (train_det.py:46-54)
            p = self.trainer.read()
            self.trainer.load({"Wb": p["Wb"] / (self.bbox_stds[:, np.newaxis] + cfg.EPS),
                               "bb": (p["bb"] - self.bbox_means) / (self.bbox_stds + cfg.EPS)})
        from roi_data_layer.layer import RoIDataLayer
        self.layer = RoIDataLayer(self.num_classes, ctx=self.ctx)
        self.layer.set_roidb(imdb.roidb)

    # ---- set-up ----------------------------------------------------------------------------------------------------
    def _build(self, layers, dims):
        from aznet_hip import ffi, synth, caffemodel as cm
        from aznet_hip.backbone import VGG16Conv5
        if self.ctx is None:
            self.ctx = ffi.default_context()
        if self.backbone is None:
            self.backbone = VGG16Conv5(device="cuda:%d" % self.ctx.device, seed=self.seed + 1,
                                       weights=cm.backbone_from_layers(layers) if layers else None)
        if dims is None:
            dims = {k: v for k, v in synth.FULL_DET_DIMS.items() if k in ("n6", "n7")}
            if layers and "fc6" in layers and "fc7" in layers:
                dims = dict(n6=layers["fc6"][1].size, n7=layers["fc7"][1].size)
        self.trainer = ffi.AzDetSolver(self.ctx, self.backbone.out_channels, dims["n6"], dims["n7"], self.num_classes,
                                       max_rois=int(cfg.TRAIN.BATCH_SIZE), seed=self.seed)
        # fillers whose std differs from the library's table (Caffe's gaussian filler, mean 0)
        rng = np.random.RandomState(self.seed)
        shp = self.trainer._shapes()
        for lname, (wk, _) in HEAD_OF.items():
            std = self.net_param[lname]["std"]
            lib_std = prototxt.DET_FILLER_STD[lname] or prototxt.DET_FILLER_DEFAULT
            if std is not None and abs(std - lib_std) > 1e-12 * std:
                self.trainer.load({wk: rng.normal(0.0, std, shp[wk]).astype(np.float32)})
        self._attach_skip()
        if layers:
            self._copy_from(layers)

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
        """net.copy_from: the head layers the model has, by name (an ImageNet VGG16 brings fc6 and fc7 only)."""
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
        """lr_mult / decay_mult / dropout of the prototxt -> the trainer; the trainable convolutions and their history."""
        from aznet_hip.ffi import DET_HEAD_KEYS
        from detect.config import train_precision
        lr, dc, drop = {}, {}, [0.0, 0.0]
        for lname, (wk, bk) in HEAD_OF.items():
            n = self.net_param[lname]
            lr[wk], lr[bk] = n["lr_mult"]
            dc[wk], dc[bk] = n["decay_mult"]
            if lname in prototxt.DET_DROPOUT_OF and n["dropout_ratio"] is not None:
                drop[prototxt.DET_DROPOUT_OF[lname]] = n["dropout_ratio"]
        self.trainer.set_hyper([lr[k] for k in DET_HEAD_KEYS], [dc[k] for k in DET_HEAD_KEYS], drop)
        prec = train_precision()                 # (ValueError on anything but 'fp32' / 'bf16')
        if prec or hasattr(self.trainer, "set_precision"):
            self.trainer.set_precision(prec)
        if self.skip is not None:
            self.trainer.set_skip_hyper(self.net_param["conv_pool5"]["lr_mult"], self.net_param["conv_pool5"]["decay_mult"])
        self.conv_train = []
        if self.backbone is not None:
            import torch
            names = [n for n in prototxt.CONV_LAYERS if max(self.net_param[n]["lr_mult"]) > 0]
            for name, w, b in self.backbone.set_trainable(names):
                n = self.net_param[name]
                self.conv_train.append((name, w, b, torch.zeros_like(w), torch.zeros_like(b), n["lr_mult"], n["decay_mult"]))

    # ---- one iteration (Caffe Solver::Step(1)) -------------------------------------------------------------------------
    def step(self, blobs=None):
        sp = self.solver_param
        if blobs is None:
            blobs = self.layer.forward()
        import torch
        from aznet_hip import ffi
        if self.skip is not None:
            conv, taps = self.backbone.forward_train(blobs["data"], taps=tuple(self.skip["sources"]))
            maps = [t.detach() for t in taps]
            # (a tap in front of the first trainable convolution takes no gradient: no buffer, no gather)
            dmaps = [torch.empty_like(m) if t.requires_grad else None for m, t in zip(maps, taps)] if self.conv_train else None
            if dmaps is not None and all(d is None for d in dmaps):
                dmaps = None
            losses, sumsq = self.trainer.step_skip(maps, blobs["rois"], blobs["labels"], blobs["bbox_targets"],
                                                   blobs["bbox_loss_weights"], self.seed, self.iter, dmaps=dmaps)
            self.last_maps, self.last_dmaps = maps, dmaps
        else:
            conv = self.backbone.forward_train(blobs["data"])
            dmap = torch.empty_like(conv) if self.conv_train else None
            losses, sumsq = self.trainer.step(conv.detach(), blobs["rois"], blobs["labels"], blobs["bbox_targets"],
                                              blobs["bbox_loss_weights"], self.seed, self.iter, dmap=dmap)
        self.last_conv, self.last_blobs, self.last_head_sumsq = conv.detach(), blobs, sumsq
        if self.conv_train:
            for _, w, b, _, _, _, _ in self.conv_train:
                w.grad = None
                b.grad = None
            if self.skip is not None:
                if dmaps is not None:
                    torch.autograd.backward([t for t, d in zip(taps, dmaps) if d is not None], [d for d in dmaps if d is not None])
            else:
                conv.backward(dmap)
            sumsq += float(sum((p.grad.double() ** 2).sum() for _, w, b, _, _, _, _ in self.conv_train for p in (w, b)))
        rate = learning_rate(sp, self.iter)
        clip = clip_scale(sumsq, sp["clip_gradients"])
        self.last_rate, self.last_clip, self.last_sumsq = rate, clip, sumsq
        self.trainer.update(rate, sp["momentum"], sp["weight_decay"], clip)
        for _, w, b, hw, hb, lr, dc in self.conv_train:
            for p, h, q in ((w, hw, 0), (b, hb, 1)):
                g = p.grad if p.grad.stride() == p.stride() else torch.empty_like(p).copy_(p.grad)
                ffi.sgd_update(self.ctx, p.detach(), g, h, rate * lr[q], sp["momentum"], sp["weight_decay"] * dc[q], clip)
        self.iter += 1
        self.losses.append(np.asarray(losses, dtype=np.float32))
        return losses

    def snapshot(self):
        """The network with bbox_pred un-normalised (weights * stds, bias * stds + means: usable at test time as it is),
        every backbone and head layer under its Caffe name; the trainer keeps its normalised weights."""
        from aznet_hip.caffemodel import write_caffemodel
        p = self.trainer.read()
        orig_w, orig_b = p["Wb"].copy(), p["bb"].copy()
        if cfg.TRAIN.BBOX_REG:
            p["Wb"] = (p["Wb"] * self.bbox_stds[:, np.newaxis]).astype(np.float32)
            p["bb"] = (p["bb"] * self.bbox_stds + self.bbox_means).astype(np.float32)
        if not os.path.exists(self.output_dir):
            os.makedirs(self.output_dir)
        infix = ("_" + cfg.TRAIN.SNAPSHOT_INFIX if cfg.TRAIN.SNAPSHOT_INFIX != "" else "")
        filename = os.path.join(self.output_dir, self.solver_param["snapshot_prefix"] + infix +
                                "_iter_{:d}".format(self.iter) + ".caffemodel")
        layers = {}
        if self.backbone is not None:
            for layer in self.backbone.layers:
                if layer is not None:
                    layers[layer[0]] = [layer[1].detach().contiguous().cpu().numpy(), layer[2].detach().cpu().numpy()]
        for lname, (wk, bk) in HEAD_OF.items():
            layers[lname] = [p[wk], p[bk]]
        if self.skip is not None:
            f = self.trainer.read_skip()
            layers["conv_pool5"] = [f["Wp"].reshape(f["Wp"].shape[0], f["Wp"].shape[1], 1, 1), f["bp"]]
        write_caffemodel(filename, layers)
        print("Wrote snapshot to: {:s}".format(filename))
        # the trainer's own bbox_pred must be what it was (train_det.py:93-96)
        now = self.trainer.read()
        if not (np.array_equal(now["Wb"], orig_w) and np.array_equal(now["bb"], orig_b)):
            self.trainer.load({"Wb": orig_w, "bb": orig_b})
        return filename

    def train_model(self, max_iters):
        """Network training loop (train_det.py:98-116)."""
        sp = self.solver_param
        last_snapshot_iter = -1
        timer = Timer()
        display, avg = int(sp["display"]), max(1, int(sp["average_loss"]))
        while self.iter < max_iters:
            timer.tic()
            self.step()
            timer.toc()
            if display > 0 and (self.iter - 1) % display == 0:
                recent = np.sum(np.asarray(self.losses[-avg:], dtype=np.float64), axis=1)
                lc, lb = self.losses[-1]
                print("Iteration {:d}, loss = {:.6g} (loss_cls = {:.6g}, loss_bbox = {:.6g}), lr = {:g}"
                      .format(self.iter - 1, float(recent.mean()), float(lc), float(lb), self.last_rate))
            if display > 0 and self.iter % (10 * display) == 0:
                print("speed: {:.3f}s / iter".format(timer.average_time))
            if self.iter % cfg.TRAIN.SNAPSHOT_ITERS == 0:
                last_snapshot_iter = self.iter
                self.snapshot()
        if last_snapshot_iter != self.iter:
            self.snapshot()


def get_training_roidb(imdb, net=None):
    """A roidb for use in training (train_det.py:118-129); `net` makes the proposals where no proposals.pkl exists."""
    if cfg.TRAIN.USE_FLIPPED:
        print("Appending horizontally-flipped training examples...")
        imdb.append_flipped_images()
        print("done")
    print("Preparing training data...")
    rdl_roidb.prepare_roidb(imdb, net)
    print("done")
    return imdb.roidb


def train_net(solver_prototxt, imdb, output_dir, pretrained_model=None, max_iters=40000, **kw):
    """Train a detection net (train_det.py:131-139); returns the SolverWrapper."""
    sw = SolverWrapper(solver_prototxt, imdb, output_dir, pretrained_model=pretrained_model, **kw)
    print("Solving...")
    sw.train_model(max_iters)
    print("done solving")
    return sw
