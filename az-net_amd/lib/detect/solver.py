"""What detect/train_az.py and detect/train_det.py share: the base of their two SolverWrapper classes -- set-up around a HIP
trainer (aznet_hip.ffi.AzSolver / AzDetSolver) and a VGG16Conv5 backbone, the second half of an iteration (backward through
the convolutions, gradient norm, rate, clip, update), snapshots and the training loop -- and Caffe's learning-rate and
clipping rules.  A subclass names its head (the class attributes below), computes its targets, builds its trainer and runs the
forward half of a step."""
import os

import numpy as np

from aznet_hip import ffi
from detect import prototxt
from detect.config import cfg, train_precision
from utils.timer import Timer


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
    """A subclass sets `solver_param`, `net_param`, `bbox_means` and `bbox_stds`, then calls this __init__, then makes its
    data layer `layer`; it gives `_build`, `_copy_from` and the forward half of `step`."""
    HEAD_OF = None         # {layer name: (weight key, bias key)} of the head's InnerProduct layers
    HEAD_KEYS = None       # the keys in the trainer's order (ffi.HEAD_KEYS / ffi.DET_HEAD_KEYS)
    DROPOUT_OF = None      # {layer name: index of its dropout ratio} (prototxt.DROPOUT_OF / DET_DROPOUT_OF)
    FILLER_STD = None      # {layer name: std of the library's gaussian filler}
    BBOX_KEYS = None       # the box-regression layer's (weight key, bias key)
    LOSS_NAMES = None      # the names of trainer.step's losses, as train_model prints them

    def __init__(self, output_dir, pretrained_model=None, backbone=None, trainer=None, ctx=None, dims=None, seed=None):
        self.output_dir = output_dir
        self.seed = int(cfg.RNG_SEED if seed is None else seed)
        self.iter = 0
        self.losses = []                       # LOSS_NAMES' values of every iteration
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
            self._copy_from(layers)
        self._configure()

    # ---- set-up ----------------------------------------------------------------------------------------------------
    def _read_solver(self, solver_prototxt):
        """The solver file into `solver_param`; returns the path of the train net it names."""
        self.solver_param = prototxt.read_solver(solver_prototxt)
        return prototxt.resolve_train_net(solver_prototxt, self.solver_param["train_net"])

    def _default_device(self, layers):
        """_build without a context or a backbone: the default context, a VGG16Conv5 from the pretrained model or seeded."""
        from aznet_hip import caffemodel as cm
        from aznet_hip.backbone import VGG16Conv5
        if self.ctx is None:
            self.ctx = ffi.default_context()
        if self.backbone is None:
            self.backbone = VGG16Conv5(device="cuda:%d" % self.ctx.device, seed=self.seed + 1,
                                       weights=cm.backbone_from_layers(layers) if layers else None)

    def _load_fillers(self):
        """Fillers whose std differs from the library's table (Caffe's gaussian filler, mean 0)."""
        rng = np.random.RandomState(self.seed)
        shp = self.trainer._shapes()
        for lname, (wk, _) in self.HEAD_OF.items():
            std = self.net_param[lname]["std"]
            if std is not None and abs(std - self.FILLER_STD[lname]) > 1e-12 * std:
                self.trainer.load({wk: rng.normal(0.0, std, shp[wk]).astype(np.float32)})

    def _configure(self):
        """lr_mult / decay_mult / dropout of the prototxt -> the trainer; the trainable convolutions and their history."""
        lr, dc, drop = {}, {}, [0.0] * len(self.DROPOUT_OF)
        for lname, (wk, bk) in self.HEAD_OF.items():
            n = self.net_param[lname]
            lr[wk], lr[bk] = n["lr_mult"]
            dc[wk], dc[bk] = n["decay_mult"]
            if lname in self.DROPOUT_OF and n["dropout_ratio"] is not None:
                drop[self.DROPOUT_OF[lname]] = n["dropout_ratio"]
        self.trainer.set_hyper([lr[k] for k in self.HEAD_KEYS], [dc[k] for k in self.HEAD_KEYS], drop)
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

    def _normalize_bbox_layer(self):
        """TRAIN.UN_NORMALIZE: scale and shift the box-regression layer of an un-normalised pretrained model into the
        normalised targets' units (train_az.py:53-61, train_det.py:46-54)."""
        wk, bk = self.BBOX_KEYS
        p = self.trainer.read()
        self.trainer.load({wk: p[wk] / (self.bbox_stds[:, np.newaxis] + cfg.EPS),
                           bk: (p[bk] - self.bbox_means) / (self.bbox_stds + cfg.EPS)})

    # ---- one iteration (Caffe Solver::Step(1)) -------------------------------------------------------------------------
    @property
    def iter_size(self):
        return int(self.solver_param.get("iter_size", 1))

    def _minibatches(self, blobs, n):
        """The n minibatches of one iteration: drawn from the data layer, or the caller's (a dict when n == 1, else a list
        of n dicts)."""
        if blobs is None:
            return [self.layer.forward() for _ in range(n)]
        if isinstance(blobs, dict):
            if n != 1:
                raise ValueError("step: iter_size = %d takes a list of %d minibatches, not one" % (n, n))
            return [blobs]
        blobs = list(blobs)
        if len(blobs) != n or not all(isinstance(b, dict) for b in blobs):
            raise ValueError("step: iter_size = %d takes a list of %d minibatches" % (n, n))
        return blobs

    def step(self, blobs=None):
        """Caffe Solver::Step(1) + SGDSolver::ApplyUpdate with n = iter_size: n minibatches' gradients summed (the trainer
        accumulates from the second on, autograd in the convolutions' .grad), the losses averaged; the norm and the clip
        on the sum, the update with clip / n.  The dropout iteration of sub-step k is iter * n + k."""
        n = self.iter_size
        subs = self._minibatches(blobs, n)
        for _, w, b, _, _, _, _ in self.conv_train:
            w.grad = None
            b.grad = None
        mean = None
        for k, mb in enumerate(subs):
            if n > 1:
                self.trainer.set_accumulate(1 if k else 0)
            losses, sumsq, backward = self._forward_backward(mb, self.iter * n + k)
            if self.conv_train:
                backward()
            if n > 1:
                row = np.asarray(losses, dtype=np.float32)
                mean = row.copy() if mean is None else mean + row
        if n > 1:
            losses = mean / np.float32(n)
        return self._apply_update(losses, sumsq, n)

    def _apply_update(self, losses, sumsq, n=1):
        """The end of step(): the norm of all accumulated gradients (sumsq: the head's share), rate, clip and the update."""
        import torch
        sp = self.solver_param
        self.last_head_sumsq = sumsq
        if self.conv_train:
            # (plumbing: the convolutions' share of the gradient norm, 14.7 M values, is taken with torch)
            sumsq += float(sum((p.grad.double() ** 2).sum() for _, w, b, _, _, _, _ in self.conv_train for p in (w, b)))
        rate = learning_rate(sp, self.iter)
        clip = clip_scale(sumsq, sp["clip_gradients"])            # on the un-normalised sum: Caffe clips before Normalize
        scale = clip if n == 1 else clip / n
        self.last_rate, self.last_clip, self.last_sumsq, self.last_scale = rate, clip, sumsq, scale
        self.trainer.update(rate, sp["momentum"], sp["weight_decay"], scale)
        for _, w, b, hw, hb, lr, dc in self.conv_train:
            for p, h, q in ((w, hw, 0), (b, hb, 1)):
                g = p.grad if p.grad.stride() == p.stride() else torch.empty_like(p).copy_(p.grad)
                ffi.sgd_update(self.ctx, p.detach(), g, h, rate * lr[q], sp["momentum"], sp["weight_decay"] * dc[q], scale)
        self.iter += 1
        self.losses.append(np.asarray(losses, dtype=np.float32))
        return losses

    def _display_extra(self):
        """One more line for train_model's display iterations, or None."""
        return None

    def _snapshot_extra(self):
        """Layers of the snapshot beside the backbone's and HEAD_OF's: {Caffe name: [blobs]}."""
        return {}

    def snapshot(self):
        """The network with the box-regression layer un-normalised (weights * stds, bias * stds + means: usable at test time
        as it is), every backbone and head layer under its Caffe name; the trainer keeps its normalised weights."""
        from aznet_hip.caffemodel import write_caffemodel
        wk, bk = self.BBOX_KEYS
        p = self.trainer.read()
        orig_w, orig_b = p[wk].copy(), p[bk].copy()
        if cfg.TRAIN.BBOX_REG:
            p[wk] = (p[wk] * self.bbox_stds[:, np.newaxis]).astype(np.float32)
            p[bk] = (p[bk] * self.bbox_stds + self.bbox_means).astype(np.float32)
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
        for lname, (k_w, k_b) in self.HEAD_OF.items():
            layers[lname] = [p[k_w], p[k_b]]
        layers.update(self._snapshot_extra())
        write_caffemodel(filename, layers)
        print("Wrote snapshot to: {:s}".format(filename))
        # the trainer's own box-regression layer must be what it was (train_az.py:94-97, train_det.py:93-96)
        now = self.trainer.read()
        if not (np.array_equal(now[wk], orig_w) and np.array_equal(now[bk], orig_b)):
            self.trainer.load({wk: orig_w, bk: orig_b})
        if getattr(cfg.TRAIN, "SNAPSHOT_STATE", False):
            self.save_state()
        return filename

    # ---- the solver's state between two iterations (Caffe's .solverstate; here a NumPy .npz) ------------------------------
    STATE_FORMAT = 1
    STATE_KIND = None      # "az" / "det" ("det_skip" with the front)

    def _state_kind(self):
        return self.STATE_KIND

    def _trainer_state(self):
        """(weights, history) as the trainer holds them: the box-regression layer normalised, the skip front included."""
        w, h = dict(self.trainer.read()), dict(self.trainer.read_history())
        if getattr(self, "skip", None) is not None:
            w.update(self.trainer.read_skip())
            h.update(self.trainer.read_skip_history())
        return w, h

    def _state_arrays(self):
        avg = max(1, int(self.solver_param["average_loss"]))
        nloss = len(self.LOSS_NAMES)
        rng = np.random.get_state()
        st = dict(format=np.int64(self.STATE_FORMAT), kind=np.array(self._state_kind()), iter=np.int64(self.iter),
                  iter_size=np.int64(self.iter_size), seed=np.uint64(self.seed & ((1 << 64) - 1)),
                  bbox_means=np.asarray(self.bbox_means), bbox_stds=np.asarray(self.bbox_stds),
                  rng_name=np.array(rng[0]), rng_keys=np.asarray(rng[1], dtype=np.uint32), rng_pos=np.int64(rng[2]),
                  rng_has_gauss=np.int64(rng[3]), rng_cached_gaussian=np.float64(rng[4]),
                  layer_perm=np.asarray(self.layer._perm, dtype=np.int64), layer_cur=np.int64(self.layer._cur),
                  roidb_len=np.int64(len(self.layer._roidb)),
                  losses=np.asarray(self.losses[-avg:], dtype=np.float32).reshape(-1, nloss))
        w, h = self._trainer_state()
        for k in w:
            st["w_" + k], st["h_" + k] = np.asarray(w[k], dtype=np.float32), np.asarray(h[k], dtype=np.float32)
        if self.backbone is not None:
            for layer in self.backbone.layers:
                if layer is not None:
                    st["conv_w_" + layer[0]] = layer[1].detach().contiguous().cpu().numpy()
                    st["conv_b_" + layer[0]] = layer[2].detach().contiguous().cpu().numpy()
            for name, _, _, hw, hb, _, _ in self.conv_train:
                st["conv_hw_" + name], st["conv_hb_" + name] = hw.contiguous().cpu().numpy(), hb.contiguous().cpu().numpy()
        return st

    def state_path(self):
        infix = ("_" + cfg.TRAIN.SNAPSHOT_INFIX if cfg.TRAIN.SNAPSHOT_INFIX != "" else "")
        return os.path.join(self.output_dir, self.solver_param["snapshot_prefix"] + infix + "_iter_{:d}".format(self.iter) + ".solverstate")

    def save_state(self, path=None):
        """Everything the next iteration depends on, into `path` (default: beside the snapshot, .solverstate): weights and
        momentum history of the trainer (as it holds them) and of the convolutions, iter, seed, the np.random stream, the
        data layer's permutation and cursor, the recent losses.  Only ever between two iterations."""
        path = self.state_path() if path is None else path
        d = os.path.dirname(path)
        if d and not os.path.exists(d):
            os.makedirs(d)
        with open(path, "wb") as f:                  # (a file object: np.savez would append ".npz" to a name)
            np.savez(f, **self._state_arrays())
        print("Wrote solver state to: {:s}".format(path))
        return path

    def restore(self, path):
        """Install a save_state file.  Everything is checked first -- format, kind, iter_size, the key set, every shape, the
        roidb length, bbox_means / bbox_stds bit for bit (the weights are in those units) -- and a mismatch is a ValueError
        that names what differs and leaves the wrapper as it was."""
        try:
            with np.load(path, allow_pickle=False) as z:
                st = {k: z[k] for k in z.files}
        except Exception as e:                       # (a truncated archive: zipfile.BadZipFile, EOFError, ValueError ...)
            raise ValueError("solver state %s cannot be read: %s: %s" % (path, type(e).__name__, e))
        for k in ("format", "kind"):
            if k not in st:
                raise ValueError("solver state %s: no '%s' entry" % (path, k))
        if int(st["format"]) != self.STATE_FORMAT:
            raise ValueError("solver state %s: format %d, this wrapper reads %d" % (path, int(st["format"]), self.STATE_FORMAT))
        if str(st["kind"]) != self._state_kind():
            raise ValueError("solver state %s: kind '%s', this wrapper is '%s'" % (path, str(st["kind"]), self._state_kind()))
        mine = self._state_arrays()
        if set(st) != set(mine):
            diff = sorted(set(st) ^ set(mine))
            raise ValueError("solver state %s: entries differ: %s" % (path, ", ".join(diff)))
        if int(st["roidb_len"]) != int(mine["roidb_len"]) or st["layer_perm"].shape != mine["layer_perm"].shape:
            raise ValueError("solver state %s: roidb of %d entries, this wrapper's has %d" % (path, int(st["roidb_len"]), int(mine["roidb_len"])))
        if int(st["iter_size"]) != self.iter_size:
            raise ValueError("solver state %s: iter_size %d, the solver file says %d" % (path, int(st["iter_size"]), self.iter_size))
        for k in sorted(mine):
            a, b = st[k], mine[k]
            same = (a.ndim == 2 and a.shape[1] == b.shape[1]) if k == "losses" else a.shape == b.shape
            if not same or (a.dtype != b.dtype and k not in ("kind", "rng_name")):
                raise ValueError("solver state %s: %s is %s %s, this wrapper holds %s %s" % (path, k, a.dtype, a.shape, b.dtype, b.shape))
        for k in ("bbox_means", "bbox_stds"):
            if st[k].tobytes() != mine[k].tobytes():
                raise ValueError("solver state %s: %s differs from this wrapper's (other data or another roidb: the weights are "
                                 "in those units)" % (path, k))
        cur = int(st["layer_cur"])
        if not 0 <= cur <= int(st["roidb_len"]) or int(st["iter"]) < 0:
            raise ValueError("solver state %s: iter or cursor out of range" % path)
        # ---- nothing below fails on a checked file
        import torch
        keys = list(self.HEAD_KEYS)
        self.trainer.load({k: st["w_" + k] for k in keys})
        self.trainer.load_history({k: st["h_" + k] for k in keys})
        if getattr(self, "skip", None) is not None:
            self.trainer.load_skip({k: st["w_" + k] for k in ffi.SKIP_KEYS})
            self.trainer.load_skip_history({k: st["h_" + k] for k in ffi.SKIP_KEYS})
        if self.backbone is not None:
            with torch.no_grad():
                for layer in self.backbone.layers:
                    if layer is not None:
                        layer[1].copy_(torch.from_numpy(st["conv_w_" + layer[0]]))
                        layer[2].copy_(torch.from_numpy(st["conv_b_" + layer[0]]))
                for name, _, _, hw, hb, _, _ in self.conv_train:
                    hw.copy_(torch.from_numpy(st["conv_hw_" + name]))
                    hb.copy_(torch.from_numpy(st["conv_hb_" + name]))
        self.iter, self.seed = int(st["iter"]), int(st["seed"])
        np.random.set_state((str(st["rng_name"]), st["rng_keys"], int(st["rng_pos"]), int(st["rng_has_gauss"]),
                             float(st["rng_cached_gaussian"])))
        self.layer._perm, self.layer._cur = st["layer_perm"].copy(), cur
        self.losses = [row.copy() for row in st["losses"]]
        print("Restored solver state from {:s}: iteration {:d}".format(path, self.iter))
        return self.iter

    def train_model(self, max_iters):
        """Network training loop (train_az.py:99-116, train_det.py:98-116)."""
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
                each = ", ".join("{:s} = {:.6g}".format(n, float(v)) for n, v in zip(self.LOSS_NAMES, self.losses[-1]))
                print("Iteration {:d}, loss = {:.6g} ({:s}), lr = {:g}".format(self.iter - 1, float(recent.mean()), each, self.last_rate))
                extra = self._display_extra()
                if extra:
                    print("    " + extra)
            if display > 0 and self.iter % (10 * display) == 0:
                print("speed: {:.3f}s / iter".format(timer.average_time))
            if self.iter % cfg.TRAIN.SNAPSHOT_ITERS == 0:
                last_snapshot_iter = self.iter
                self.snapshot()
        if last_snapshot_iter != self.iter:
            self.snapshot()

    @classmethod
    def train_net(cls, solver_prototxt, imdb, output_dir, pretrained_model=None, max_iters=40000, restore=None, **kw):
        """Train a network (train_az.py:131-139, train_det.py:131-139); returns the SolverWrapper.  restore: a save_state
        file to continue from (max_iters stays the total)."""
        sw = cls(solver_prototxt, imdb, output_dir, pretrained_model=pretrained_model, **kw)
        if restore is not None:
            print("Resuming from iteration {:d} of {:d}".format(sw.restore(restore), max_iters))
        print("Solving...")
        sw.train_model(max_iters)
        print("done solving")
        return sw


def get_training_roidb(rdl_roidb, imdb, *args):
    """A roidb for use in training (train_az.py:118-129, train_det.py:118-129), prepared by the data layer's roidb module."""
    if cfg.TRAIN.USE_FLIPPED:
        print("Appending horizontally-flipped training examples...")
        imdb.append_flipped_images()
        print("done")
    print("Preparing training data...")
    rdl_roidb.prepare_roidb(imdb, *args)
    print("done")
    return imdb.roidb
