"""Train an AZ-net (reference: lib/detect/train_az.py) without Caffe: PyTorch-ROCm runs the VGG16 convolutions with
autograd, everything from conv5_3 on -- RoIPool, the six InnerProduct layers forward and backward, dropout, the three
losses, the gradient norm and the SGD update -- is the HIP trainer behind az_solver_* (aznet_hip.ffi.AzSolver)."""
import os

import numpy as np

import az_data_layer.roidb as rdl_roidb
from detect import prototxt
from detect.config import cfg
from utils.timer import Timer

HEAD_OF = {"int6": ("W6", "b6"), "int7_1": ("W71", "b71"), "int7_2": ("W72", "b72"), "adj_score": ("Was", "bas"),
           "adj_bbox": ("Wab", "bab"), "zoom_score": ("Wz", "bz")}


def learning_rate(sp, it):
    """Caffe SGDSolver::GetLearningRate for lr_policy "fixed" and "step"."""
    if sp["lr_policy"] == "fixed":
        return float(sp["base_lr"])
    return float(sp["base_lr"]) * float(sp["gamma"]) ** (int(it) // int(sp["stepsize"]))


def clip_scale(sumsq, clip_gradients):
    """SGDSolver::ClipGradients: clip / ||g|| when the L2 norm of ALL learnable gradients exceeds clip_gradients."""
    norm = float(np.sqrt(sumsq))
    if clip_gradients is not None and clip_gradients > 0 and norm > clip_gradients:
        return float(clip_gradients) / norm
    return 1.0


class SolverWrapper(object):
    """What the reference's wrapper around caffe.SGDSolver does (train_az.py:25-116): the adjacency targets and their
    means / stds, the data layer, the TRAIN.UN_NORMALIZE re-initialisation of adj_bbox, the training loop and the
    snapshots with un-normalised adj_bbox weights.
    backbone: a VGG16Conv5 (default: built from pretrained_model, or seeded); trainer: an AzSolver (default: created on
    `ctx` with the head's sizes -- `dims` or the pretrained model's or VGG16's); seed: the dropout / filler seed."""

    def __init__(self, solver_prototxt, imdb, output_dir, pretrained_model=None, backbone=None, trainer=None, ctx=None,
                 dims=None, seed=None):
        self.output_dir = output_dir
        print("Computing adjacent prediction targets...")
        self.bbox_means, self.bbox_stds = rdl_roidb.add_adjacent_prediction_targets(imdb)
        print("done")
        self.solver_param = prototxt.read_solver(solver_prototxt)
        self.net_param = prototxt.read_train_net(prototxt.resolve_train_net(solver_prototxt, self.solver_param["train_net"]))
        self.seed = int(cfg.RNG_SEED if seed is None else seed)
        self.iter = 0
        self.losses = []                       # (loss_zoom, loss_adj, loss_bbox) of every iteration
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
        elif layers is not None:
            self._copy_from(layers)
        self._configure()
        from az_data_layer.layer import AZDataLayer
        self.layer = AZDataLayer(ctx=self.ctx)
        self.layer.set_roidb(imdb.roidb)
        if cfg.TRAIN.UN_NORMALIZE:
            # re-initialize the bounding-box regression layer (train_az.py:53-61)
            p = self.trainer.read()
            self.trainer.load({"Wab": p["Wab"] / (self.bbox_stds[:, np.newaxis] + cfg.EPS),
                               "bab": (p["bab"] - self.bbox_means) / (self.bbox_stds + cfg.EPS)})

    # ---- set-up ----------------------------------------------------------------------------------------------------
    def _build(self, layers, dims):
        from aznet_hip import ffi, synth, caffemodel as cm
        from aznet_hip.backbone import VGG16Conv5
        if self.ctx is None:
            self.ctx = ffi.default_context()
        if self.backbone is None:
            self.backbone = VGG16Conv5(device="cuda:%d" % self.ctx.device, seed=self.seed + 1,
                                       weights=cm.backbone_from_layers(layers) if layers else None)
        head = cm.az_head_from_layers(layers) if layers and "int6" in layers else None
        if dims is None:
            dims = dict(synth.FULL_DIMS)
            if head is not None:
                dims = dict(n6=head["W6"].shape[0], n71=head["W71"].shape[0], n72=head["W72"].shape[0])
        d = dict(dims, C=self.backbone.out_channels)
        self.trainer = ffi.AzSolver(self.ctx, d["C"], d["n6"], d["n71"], d["n72"], max_rois=int(cfg.TRAIN.BATCH_SIZE),
                                    seed=self.seed, head=head)
        if head is None:
            # fillers whose std differs from the library's table (Caffe's gaussian filler, mean 0)
            rng = np.random.RandomState(self.seed)
            shp = self.trainer._shapes()
            for lname, (wk, _) in HEAD_OF.items():
                std = self.net_param[lname]["std"]
                if std is not None and abs(std - prototxt.FILLER_STD[lname]) > 1e-12 * std:
                    self.trainer.load({wk: rng.normal(0.0, std, shp[wk]).astype(np.float32)})

    def _copy_from(self, layers):
        from aznet_hip import caffemodel as cm
        if "int6" in layers:
            self.trainer.load(cm.az_head_from_layers(layers))

    def _configure(self):
        """lr_mult / decay_mult / dropout of the prototxt -> the trainer; the trainable convolutions and their history."""
        from aznet_hip.ffi import HEAD_KEYS
        from detect.config import train_precision
        lr, dc, drop = {}, {}, [0.0, 0.0, 0.0]
        for lname, (wk, bk) in HEAD_OF.items():
            n = self.net_param[lname]
            lr[wk], lr[bk] = n["lr_mult"]
            dc[wk], dc[bk] = n["decay_mult"]
            if lname in prototxt.DROPOUT_OF and n["dropout_ratio"] is not None:
                drop[prototxt.DROPOUT_OF[lname]] = n["dropout_ratio"]
        self.trainer.set_hyper([lr[k] for k in HEAD_KEYS], [dc[k] for k in HEAD_KEYS], drop)
        prec = train_precision()                 # (ValueError on anything but 'fp32' / 'bf16')
        if prec or hasattr(self.trainer, "set_precision"):
            self.trainer.set_precision(prec)
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
        conv = self.backbone.forward_train(blobs["data"])
        dmap = torch.empty_like(conv) if self.conv_train else None
        losses, sumsq = self.trainer.step(conv.detach(), blobs["rois"], blobs["adj_labels"], blobs["adj_targets"],
                                          blobs["adj_loss_weights"], blobs["zoom_labels"], self.seed, self.iter, dmap=dmap)
        self.last_conv, self.last_blobs, self.last_head_sumsq = conv.detach(), blobs, sumsq
        if self.conv_train:
            for _, w, b, _, _, _, _ in self.conv_train:
                w.grad = None
                b.grad = None
            conv.backward(dmap)
            # (plumbing: the convolutions' share of the gradient norm, 14.7 M values, is taken with torch)
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
        """The network with adj_bbox un-normalised (weights * stds, bias * stds + means: usable at test time as it is),
        every backbone and head layer under its Caffe name; the trainer keeps its normalised weights."""
        from aznet_hip.caffemodel import write_caffemodel
        p = self.trainer.read()
        orig_w, orig_b = p["Wab"].copy(), p["bab"].copy()
        if cfg.TRAIN.BBOX_REG:
            p["Wab"] = (p["Wab"] * self.bbox_stds[:, np.newaxis]).astype(np.float32)
            p["bab"] = (p["bab"] * self.bbox_stds + self.bbox_means).astype(np.float32)
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
        write_caffemodel(filename, layers)
        print("Wrote snapshot to: {:s}".format(filename))
        # the trainer's own adj_bbox must be what it was (train_az.py:94-97)
        now = self.trainer.read()
        if not (np.array_equal(now["Wab"], orig_w) and np.array_equal(now["bab"], orig_b)):
            self.trainer.load({"Wab": orig_w, "bab": orig_b})
        return filename

    def train_model(self, max_iters):
        """Network training loop (train_az.py:99-116)."""
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
                z, a, b = self.losses[-1]
                print("Iteration {:d}, loss = {:.6g} (loss_zoom = {:.6g}, loss_adj = {:.6g}, loss_bbox = {:.6g}), lr = {:g}"
                      .format(self.iter - 1, float(recent.mean()), float(z), float(a), float(b), self.last_rate))
            if display > 0 and self.iter % (10 * display) == 0:
                print("speed: {:.3f}s / iter".format(timer.average_time))
            if self.iter % cfg.TRAIN.SNAPSHOT_ITERS == 0:
                last_snapshot_iter = self.iter
                self.snapshot()
        if last_snapshot_iter != self.iter:
            self.snapshot()


def get_training_roidb(imdb):
    """A roidb for use in training (train_az.py:118-129)."""
    if cfg.TRAIN.USE_FLIPPED:
        print("Appending horizontally-flipped training examples...")
        imdb.append_flipped_images()
        print("done")
    print("Preparing training data...")
    rdl_roidb.prepare_roidb(imdb)
    print("done")
    return imdb.roidb


def train_net(solver_prototxt, imdb, output_dir, pretrained_model=None, max_iters=40000, **kw):
    """Train an AZ-net (train_az.py:131-139); returns the SolverWrapper."""
    sw = SolverWrapper(solver_prototxt, imdb, output_dir, pretrained_model=pretrained_model, **kw)
    print("Solving...")
    sw.train_model(max_iters)
    print("done solving")
    return sw
