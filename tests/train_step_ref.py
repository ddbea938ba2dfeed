"""A CPU restatement of ONE AZ-net training step from conv5_3 on (test infrastructure; the yardstick of
tests/test_train_step_host.py and tests/test_gpu_train_step.py).  Written from the layer table of the training issue and
include/aznet_hip.h, not from the HIP code: explicit RoIPool with first-maximum arg-max, InnerProduct / ReLU / Dropout,
SigmoidCrossEntropyLoss, SmoothL1Loss, the hand-written backward, the gradient norm and Caffe's SGD step.  The dropout masks
and (optionally) the ReLU gates are INPUTS; `dtype` is float64 (the reference) or float32 (what sets the tolerance)."""
import os

import numpy as np

KEYS = ("W6", "b6", "W71", "b71", "W72", "b72", "Was", "bas", "Wab", "bab", "Wz", "bz")
LR_MULT = {k: (2.0 if k.startswith("b") else 1.0) for k in KEYS}
DECAY_MULT = {k: (0.0 if k.startswith("b") else 1.0) for k in KEYS}


def _roundf(x):
    """C roundf on float32: half away from zero."""
    x = np.float32(x)
    return int(np.sign(x) * np.floor(np.abs(x) + np.float32(0.5)))


def roi_pool(fmap, rois, spatial_scale=0.0625, pooled=7):
    """Caffe ROIPooling: fmap [N,C,H,W] f32, rois [R,5] f32 -> (pool5 [R, C*49] f32 flattened c*49 + ph*7 + pw,
    argmax [R, C*49] int32 = h*W + w of the FIRST maximum in (h, w) scan order, -1 for an empty bin)."""
    f32 = np.float32
    N, C, H, W = fmap.shape
    R = rois.shape[0]
    pool = np.zeros((R, C, pooled, pooled), dtype=np.float32)
    arg = np.full((R, C, pooled, pooled), -1, dtype=np.int32)
    ss = f32(spatial_scale)
    for r in range(R):
        n = int(rois[r, 0])
        rsw, rsh, rew, reh = (_roundf(f32(rois[r, q]) * ss) for q in (1, 2, 3, 4))
        rh, rw = max(reh - rsh + 1, 1), max(rew - rsw + 1, 1)
        bh, bw = f32(rh) / f32(pooled), f32(rw) / f32(pooled)
        for ph in range(pooled):
            hs = min(max(int(np.floor(f32(ph) * bh)) + rsh, 0), H)
            he = min(max(int(np.ceil(f32(ph + 1) * bh)) + rsh, 0), H)
            for pw in range(pooled):
                ws = min(max(int(np.floor(f32(pw) * bw)) + rsw, 0), W)
                we = min(max(int(np.ceil(f32(pw + 1) * bw)) + rsw, 0), W)
                if he <= hs or we <= ws:
                    continue
                win = fmap[n, :, hs:he, ws:we].reshape(C, -1)
                k = win.argmax(axis=1)                  # first maximum in row-major (h, w) order
                pool[r, :, ph, pw] = win[np.arange(C), k]
                arg[r, :, ph, pw] = (hs + k // (we - ws)) * W + (ws + k % (we - ws))
    return pool.reshape(R, -1), arg.reshape(R, -1)


def roi_pool_backward(dpool, argmax, rois, shape):
    """Each pooled gradient to its arg-max cell; -> [N,C,H,W]."""
    N, C, H, W = shape
    R = rois.shape[0]
    d = np.zeros((N, C, H * W), dtype=dpool.dtype)
    dp = dpool.reshape(R, C, 49)
    am = argmax.reshape(R, C, 49)
    cc = np.repeat(np.arange(C), 49).reshape(C, 49)
    for r in range(R):
        n = int(rois[r, 0])
        ok = am[r] >= 0
        np.add.at(d[n], (cc[ok], am[r][ok]), dp[r][ok])
    return d.reshape(N, C, H, W)


def sigmoid_ce(x, t, num):
    """(loss, dx) of SigmoidCrossEntropyLoss with loss_weight 1, normalised by `num`."""
    ge = (x >= 0).astype(x.dtype)
    ex = np.exp(x - 2 * x * ge)
    loss = -np.sum(x * (t - ge) - np.log1p(ex)) / num
    sg = np.where(x >= 0, 1 / (1 + ex), ex / (1 + ex))
    return loss, ((sg - t) / num).astype(x.dtype)


def smooth_l1(x, t, w, num):
    d = w * (x - t)
    ad = np.abs(d)
    loss = np.sum(np.where(ad < 1, 0.5 * d * d, ad - 0.5)) / num
    g = np.where(ad < 1, d, np.sign(d))
    return loss, (w * g / num).astype(x.dtype)


def step(params, pool5, blobs, masks, gates=None, dtype=np.float64, ratios=(0.5, 0.5, 0.5), want_dpool=True):
    """Forward + backward of the head on pooled rows.  params: the twelve Caffe-layout arrays; pool5 [R, C*49];
    blobs: adj_labels [R,11], adj_targets [R,44], adj_loss_weights [R,44], zoom_labels [R]; masks: {6, 71, 72: keep
    flags [R, n]} (None: no dropout); gates: {6, 71, 72: bool [R, n]} to impose on the ReLUs (None: pre > 0); ratios: the
    dropout ratios of int6 / int7_1 / int7_2, rounded to float32 first in BOTH dtypes (the trainer holds them as float32, so
    that is the ratio the step is run at); a layer whose ratio is 0 has no dropout and its mask is not looked at.
    Returns a dict of every tensor by the names az_solver_fetch uses."""
    dt = dtype
    P = {k: np.asarray(params[k], dtype=dt) for k in KEYS}
    R = pool5.shape[0]
    ratios = [float(np.float32(r)) for r in ratios]
    out = {}

    def hidden(x, W, b, tag, ratio):
        pre = x @ W.T + b
        gate = (pre > 0) if gates is None else gates[tag].astype(bool)
        a = np.where(gate, pre, 0).astype(dt)
        sc = dt(1)
        if masks is not None and ratio > 0:
            sc = dt(1) / (dt(1) - dt(ratio))
            a = np.where(masks[tag].astype(bool), a * sc, 0).astype(dt)
        out["pre%d" % tag], out["a%d" % tag] = pre, a
        return a, gate, sc

    x = np.asarray(pool5, dtype=dt)
    a6, g6, s6 = hidden(x, P["W6"], P["b6"], 6, ratios[0])
    a71, g71, s71 = hidden(a6, P["W71"], P["b71"], 71, ratios[1])
    a72, g72, s72 = hidden(a6, P["W72"], P["b72"], 72, ratios[2])
    s_as = a71 @ P["Was"].T + P["bas"]
    s_ab = a71 @ P["Wab"].T + P["bab"]
    s_z = (a72 @ P["Wz"].T + P["bz"]).reshape(R)
    out.update(adj_score=s_as, adj_bbox=s_ab, zoom_score=s_z)
    lz, d_z = sigmoid_ce(s_z, np.asarray(blobs["zoom_labels"], dt).reshape(R), dt(R))
    la, d_as = sigmoid_ce(s_as, np.asarray(blobs["adj_labels"], dt), dt(R))
    lb, d_ab = smooth_l1(s_ab, np.asarray(blobs["adj_targets"], dt), np.asarray(blobs["adj_loss_weights"], dt), dt(R))
    out["losses"] = np.array([lz, la, lb], dtype=dt)
    out.update(d_zoom_score=d_z, d_adj_score=d_as, d_adj_bbox=d_ab)
    g = {}
    d_z2 = d_z.reshape(R, 1)
    g["Was"], g["bas"] = d_as.T @ a71, d_as.sum(0)
    g["Wab"], g["bab"] = d_ab.T @ a71, d_ab.sum(0)
    g["Wz"], g["bz"] = d_z2.T @ a72, d_z2.sum(0)

    def back(d, gate, tag, sc, ratio):
        if masks is not None and ratio > 0:
            d = np.where(masks[tag].astype(bool), d * sc, 0)
        return np.where(gate, d, 0).astype(dt)

    d71 = back(d_as @ P["Was"] + d_ab @ P["Wab"], g71, 71, s71, ratios[1])
    d72 = back(d_z2 @ P["Wz"], g72, 72, s72, ratios[2])
    g["W71"], g["b71"] = d71.T @ a6, d71.sum(0)
    g["W72"], g["b72"] = d72.T @ a6, d72.sum(0)
    d6 = back(d71 @ P["W71"] + d72 @ P["W72"], g6, 6, s6, ratios[0])
    g["W6"], g["b6"] = d6.T @ x, d6.sum(0)
    out.update(d_pre71=d71, d_pre72=d72, d_pre6=d6)
    if want_dpool:
        out["d_pool5"] = d6 @ P["W6"]
    out["grads"] = g
    out["sumsq"] = float(sum(np.sum(np.asarray(v, np.float64) ** 2) for v in g.values()))
    out["gates"] = {6: g6, 71: g71, 72: g72}
    return out


def learning_rate(policy, base_lr, it, gamma=0.1, stepsize=1):
    """Caffe SGDSolver::GetLearningRate for lr_policy "fixed" and "step"."""
    if policy == "fixed":
        return float(base_lr)
    if policy == "step":
        return float(base_lr) * float(gamma) ** (int(it) // int(stepsize))
    raise ValueError("lr_policy %r" % (policy,))


def clip_scale(sumsq, clip_gradients):
    """clip_gradients / ||g|| when the norm of ALL learnable gradients exceeds clip_gradients (> 0), else 1."""
    norm = float(np.sqrt(sumsq))
    if clip_gradients is not None and clip_gradients > 0 and norm > clip_gradients:
        return float(clip_gradients) / norm
    return 1.0


def sgd(params, grads, hist, rate, momentum, weight_decay, clip, dtype=np.float64, lr_mult=LR_MULT, decay_mult=DECAY_MULT):
    """Caffe's SGD step on every blob: g = clip g + (wd decay_mult) w; h = momentum h + (rate lr_mult) g; w -= h."""
    dt = dtype
    new_p, new_h = {}, {}
    for k in params:
        w, g, h = (np.asarray(a, dtype=dt) for a in (params[k], grads[k], hist[k]))
        gg = g * dt(clip)
        gg = gg + dt(weight_decay * decay_mult[k]) * w
        hh = dt(momentum) * h + dt(rate * lr_mult[k]) * gg
        new_h[k], new_p[k] = hh, w - hh
    return new_p, new_h


def rel_err(got, ref64):
    """max |got - ref| / max |ref| (the per-tensor error of the issue); 0 for two all-zero tensors."""
    ref = np.asarray(ref64, dtype=np.float64)
    d = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref))) if ref.size else 0.0
    m = float(np.max(np.abs(ref))) if ref.size else 0.0
    return d / m if m > 0 else d


def bound(err32):
    """The tolerance of the issue: 8 x the float32-CPU restatement's own error against float64, floor 1e-6."""
    return max(8.0 * float(err32), 1e-6)


# ---- seeded cases shared by the host and the GPU tests ---------------------------------------------------------------------
def filler_head(seed, C, n6, n71, n72, gain=1.0):
    """Caffe-layout weights at a scale that keeps every layer alive (He-like), biases small."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def w(no, ni, s):
        return (rng.standard_normal((no, ni)) * s * gain / np.sqrt(ni)).astype(np.float32)
    return {"W6": w(n6, C * 49, 1.4), "b6": (0.05 * rng.standard_normal(n6)).astype(np.float32),
            "W71": w(n71, n6, 1.4), "b71": (0.05 * rng.standard_normal(n71)).astype(np.float32),
            "W72": w(n72, n6, 1.4), "b72": (0.05 * rng.standard_normal(n72)).astype(np.float32),
            "Was": w(11, n71, 1.0), "bas": np.zeros(11, np.float32), "Wab": w(44, n71, 0.5), "bab": np.zeros(44, np.float32),
            "Wz": w(1, n72, 1.0), "bz": np.zeros(1, np.float32)}


def random_blobs(seed, R, N, H, W):
    """rois inside N maps of H x W cells (network-input pixels = 16 x cells) and labels / targets shaped like the data
    layer's: binary zoom labels, adjacency labels in [0, 1] (some fractional, SEAR.SCALE_ADJ_CONF), targets where the
    weights are 1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x1 = rng.uniform(0, 16 * W - 40, R)
    y1 = rng.uniform(0, 16 * H - 40, R)
    x2 = np.minimum(x1 + rng.uniform(20, 16 * W * 0.7, R), 16 * W - 1)
    y2 = np.minimum(y1 + rng.uniform(20, 16 * H * 0.7, R), 16 * H - 1)
    rois = np.stack([np.sort(rng.integers(0, N, R)).astype(np.float64), x1, y1, x2, y2], 1).astype(np.float32)
    lab = (rng.random((R, 11)) < 0.2).astype(np.float32) * np.where(rng.random((R, 11)) < 0.5, 1.0, rng.random((R, 11))).astype(np.float32)
    wgt = np.repeat((lab > 0).astype(np.float32), 4, axis=1)
    tgt = (rng.standard_normal((R, 44)) * 1.5).astype(np.float32) * wgt
    return {"rois": rois, "adj_labels": lab.astype(np.float32), "adj_targets": tgt, "adj_loss_weights": wgt,
            "zoom_labels": (rng.random(R) < 0.4).astype(np.float32)}


class ShapeOnlyBlobCtx(object):
    """The image front-end's shape arithmetic without the GPU (zeros of cv2's dsize): for cases whose conv5_3 maps do not
    come from the images."""

    def image_blob(self, im, means, scale):
        return np.zeros((1, 3, int(np.round(im.shape[0] * scale)), int(np.round(im.shape[1] * scale))), np.float32)


def data_layer_blobs(height, width, n_images, seed, blob_ctx=None, n_batches=1):
    """Minibatches of AZDataLayer over SyntheticImdb(height, width, n_images) with the data layer's entry points answered
    by the NumPy restatement (train_ref.RefBackend), so that the CPU and the GPU tests see the SAME rows.  Returns
    (list of blob dicts, imdb, means, stds)."""
    import train_ref
    from az_data_layer import roidb as rdl
    from az_data_layer.layer import AZDataLayer
    from datasets.synthetic import SyntheticImdb
    from detect.train_az import get_training_roidb
    rdl.set_backend(train_ref.RefBackend())
    try:
        imdb = SyntheticImdb(height, width, n_images)
        np.random.seed(seed)
        get_training_roidb(imdb)
        means, stds = rdl.add_adjacent_prediction_targets(imdb)
        layer = AZDataLayer(ctx=blob_ctx or ShapeOnlyBlobCtx())
        layer.set_roidb(imdb.roidb)
        return [layer.forward() for _ in range(n_batches)], imdb, means, stds
    finally:
        rdl.set_backend(None)


FULL = dict(C=512, n6=4096, n71=1024, n72=256)


def full_size_case():
    """The full-size step of the issue: C = 512, n6 = 4096, R = 128 rows over N = 2 maps of 38 x 63 cells
    (synth.make_feature_map), the other five blobs from AZDataLayer on a 600 x 1000 synthetic imdb."""
    from aznet_hip import synth
    blobs = data_layer_blobs(600, 1000, 2, seed=11)[0][0]
    fmap = np.concatenate([synth.make_feature_map(s, 512, 38, 63) for s in (31, 32)], axis=0)
    assert blobs["rois"].shape == (128, 5) and int(blobs["rois"][:, 0].max()) == 1
    return filler_head(5, **FULL), fmap, blobs


def small_case(R=128, seed=7, dims=None):
    """dims: (C, n6, n71, n72), default synth.SMALL_DIMS."""
    from aznet_hip import synth
    d = synth.SMALL_DIMS if dims is None else dict(zip(("C", "n6", "n71", "n72"), dims))
    fmap = np.concatenate([synth.make_feature_map(s, d["C"], 24, 32) for s in (seed, seed + 1)], axis=0)
    return filler_head(seed, **d), fmap, random_blobs(seed, R, 2, 24, 32)


def gate_mismatch(pre_a, pre_ref):
    """Fraction of units whose ReLU gate differs between two evaluations of a layer's pre-activations."""
    return float(np.mean((np.asarray(pre_a) > 0) != (np.asarray(pre_ref) > 0)))


# ---- the 20-step runs through SolverWrapper (reduced head, width_div backbone, two-image synthetic imdb) -------------------
TRAJ = dict(height=375, width=500, n_images=2, roidb_seed=5, width_div=32, backbone_seed=21, solver_seed=3, steps=20,
            solver=dict(base_lr=0.01, lr_policy="step", gamma=0.5, stepsize=10, momentum=0.9, weight_decay=0.0005,
                        clip_gradients=20.0, display=5, average_loss=5, snapshot_prefix="az_small"))


class TorchBlobCtx(object):
    """The image front-end on the CPU (mean subtraction, bilinear resize with half-pixel centres): close to the device's,
    for the CPU check of the frozen run."""

    def image_blob(self, im, means, scale):
        import torch
        x = torch.from_numpy(np.ascontiguousarray((im.astype(np.float32) - np.asarray(means, np.float32)).transpose(2, 0, 1)))[None]
        oh, ow = int(np.round(im.shape[0] * scale)), int(np.round(im.shape[1] * scale))
        return torch.nn.functional.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False).numpy()


def traj_backbone(device):
    from aznet_hip.backbone import VGG16Conv5
    bb = VGG16Conv5(device=device, seed=TRAJ["backbone_seed"], width_div=TRAJ["width_div"])
    bb.fused_epilogue = False
    # (unit RMS of conv5_3 on a blob with the range of a mean-subtracted image)
    bb.normalize_output(np.random.RandomState(0).uniform(-120, 140, (1, 3, TRAJ["height"], TRAJ["width"])).astype(np.float32))
    return bb


def traj_solver_files(dirname, frozen_all, edit_rows=None):
    """edit_rows: a function on the rows of prototxt.layer_table, applied before the train net is written."""
    from detect import prototxt as P
    net = os.path.join(dirname, "train_%s.prototxt" % ("shared" if frozen_all else "az"))
    rows = P.layer_table(frozen=P.CONV_LAYERS if frozen_all else P.CONV_LAYERS[:4])
    P.write_train_prototxt(net, rows if edit_rows is None else edit_rows(rows))
    sol = os.path.join(dirname, "solver_%s.prototxt" % ("shared" if frozen_all else "az"))
    P.write_solver_prototxt(sol, net, **TRAJ["solver"])
    return sol


class RefTrajectory(object):
    """The restatement stepping beside a device run: same start, same minibatches, same conv5_3 maps, same masks (drawn at
    `ratios`; none for a layer whose ratio is 0), the update with `lr_mult` / `decay_mult`."""

    def __init__(self, params, dtype, solver=None, ratios=(0.5, 0.5, 0.5), lr_mult=LR_MULT, decay_mult=DECAY_MULT):
        self.dt = dtype
        self.p = {k: np.asarray(v, dtype) for k, v in params.items()}
        self.h = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.sp = dict(TRAJ["solver"] if solver is None else solver)
        self.it = 0
        self.ratios, self.lr_mult, self.decay_mult = tuple(ratios), lr_mult, decay_mult

    def step(self, conv, blobs, seed, gates=None):
        from aznet_hip import ffi
        pool, _ = roi_pool(conv, blobs["rois"])
        n = pool.shape[0]
        masks = {t: ffi.dropout_mask(seed, self.it, l, n * self.p[k].shape[0], ratio=self.ratios[l]).reshape(n, -1)
                 for t, l, k in ((6, 0, "b6"), (71, 1, "b71"), (72, 2, "b72")) if self.ratios[l] > 0}
        r = step(self.p, pool, blobs, masks, gates=gates, dtype=self.dt, ratios=self.ratios, want_dpool=False)
        rate = learning_rate(self.sp["lr_policy"], self.sp["base_lr"], self.it, self.sp["gamma"], self.sp["stepsize"])
        self.p, self.h = sgd(self.p, r["grads"], self.h, rate, self.sp["momentum"], self.sp["weight_decay"],
                             clip_scale(r["sumsq"], self.sp["clip_gradients"]), dtype=self.dt, lr_mult=self.lr_mult,
                             decay_mult=self.decay_mult)
        self.it += 1
        return r
