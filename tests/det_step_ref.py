"""A CPU restatement of ONE detection-net (Fast R-CNN) training step from conv5_3 on (test infrastructure; the yardstick of
tests/test_det_train_host.py and tests/test_gpu_det_train.py).  Written from the layer graph of frcnn/train.prototxt and
include/aznet_hip.h, not from the HIP code: RoIPool (train_step_ref.roi_pool) -> fc6 -> fc7 -> {cls_score, bbox_pred},
SoftmaxWithLoss and SmoothL1Loss normalised by the rows, the hand-written backward, the gradient norm and Caffe's SGD step
(train_step_ref.sgd).  The dropout masks and (optionally) the ReLU gates are INPUTS; `dtype` is float64 (the reference) or
float32 (what sets the tolerance)."""
import numpy as np

import train_step_ref as R
from train_step_ref import bound, clip_scale, learning_rate, rel_err, roi_pool, roi_pool_backward, sgd, smooth_l1  # noqa: F401

KEYS = ("W6", "b6", "W7", "b7", "Wc", "bc", "Wb", "bb")
LR_MULT = {k: (2.0 if k.startswith("b") else 1.0) for k in KEYS}
DECAY_MULT = {k: (0.0 if k.startswith("b") else 1.0) for k in KEYS}
LAYERS = ((6, 0, "b6"), (7, 1, "b7"))          # (tag, dropout layer id, bias key)


def softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(x.dtype)


def softmax_loss(x, labels, num):
    """(loss, dx, p) of SoftmaxWithLoss with loss_weight 1, normalised by `num`."""
    p = softmax(x)
    lab = np.asarray(labels).astype(np.int64)
    rows = np.arange(x.shape[0])
    tiny = np.finfo(np.float32).tiny
    loss = -np.sum(np.log(np.maximum(p[rows, lab], x.dtype.type(tiny)))) / num
    d = p.copy()
    d[rows, lab] -= 1
    return loss, (d / num).astype(x.dtype), p


def step(params, pool5, blobs, masks, gates=None, dtype=np.float64, ratios=(0.5, 0.5), want_dpool=True):
    """Forward + backward of the head on pooled rows.  params: the eight Caffe-layout arrays; pool5 [R, C*49]; blobs: labels
    [R], bbox_targets / bbox_loss_weights [R, 4 ncls]; masks: {6, 7: keep flags [R, n]} (None: no dropout); gates: {6, 7: bool
    [R, n]} to impose on the ReLUs (None: pre > 0); ratios rounded to float32 first in both dtypes.  Returns a dict of every
    tensor by the names az_det_solver_fetch uses."""
    dt = dtype
    P = {k: np.asarray(params[k], dtype=dt) for k in KEYS}
    n = pool5.shape[0]
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
    a7, g7, s7 = hidden(a6, P["W7"], P["b7"], 7, ratios[1])
    s_c = a7 @ P["Wc"].T + P["bc"]
    s_b = a7 @ P["Wb"].T + P["bb"]
    lc, d_c, prob = softmax_loss(s_c, blobs["labels"], dt(n))
    lb, d_b = smooth_l1(s_b, np.asarray(blobs["bbox_targets"], dt), np.asarray(blobs["bbox_loss_weights"], dt), dt(n))
    out.update(cls_score=s_c, cls_prob=prob, bbox_pred=s_b, d_cls_score=d_c, d_bbox_pred=d_b)
    out["losses"] = np.array([lc, lb], dtype=dt)
    g = {}
    g["Wc"], g["bc"] = d_c.T @ a7, d_c.sum(0)
    g["Wb"], g["bb"] = d_b.T @ a7, d_b.sum(0)

    def back(d, gate, tag, sc, ratio):
        if masks is not None and ratio > 0:
            d = np.where(masks[tag].astype(bool), d * sc, 0)
        return np.where(gate, d, 0).astype(dt)

    d7 = back(d_c @ P["Wc"] + d_b @ P["Wb"], g7, 7, s7, ratios[1])
    g["W7"], g["b7"] = d7.T @ a6, d7.sum(0)
    d6 = back(d7 @ P["W7"], g6, 6, s6, ratios[0])
    g["W6"], g["b6"] = d6.T @ x, d6.sum(0)
    out.update(d_pre7=d7, d_pre6=d6)
    if want_dpool:
        out["d_pool5"] = d6 @ P["W6"]
    out["grads"] = g
    out["sumsq"] = float(sum(np.sum(np.asarray(v, np.float64) ** 2) for v in g.values()))
    out["gates"] = {6: g6, 7: g7}
    return out


def forward_test(params, pool5, dtype=np.float64):
    """TEST phase: (cls_prob, bbox_pred)."""
    r = step(params, pool5, {"labels": np.zeros(pool5.shape[0]), "bbox_targets": np.zeros((pool5.shape[0], params["bb"].size)),
                             "bbox_loss_weights": np.zeros((pool5.shape[0], params["bb"].size))}, None, dtype=dtype, want_dpool=False)
    return r["cls_prob"], r["bbox_pred"]


# ---- seeded cases shared by the host and the GPU tests ---------------------------------------------------------------------
HEADS = {"small": dict(C=4, n6=4, n7=4, ncls=2, R=1),
         "voc": dict(C=12, n6=132, n7=100, ncls=21, R=37),
         "coco": dict(C=44, n6=260, n7=516, ncls=81, R=130)}
MAP_H, MAP_W = 12, 16                            # two maps of 12 x 16 cells


def filler_head(seed, C, n6, n7, ncls, gain=1.0):
    """Caffe-layout weights at a scale that keeps every layer alive (He-like), biases small."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def w(no, ni, s):
        return (rng.standard_normal((no, ni)) * s * gain / np.sqrt(ni)).astype(np.float32)
    return {"W6": w(n6, C * 49, 1.4), "b6": (0.05 * rng.standard_normal(n6)).astype(np.float32),
            "W7": w(n7, n6, 1.4), "b7": (0.05 * rng.standard_normal(n7)).astype(np.float32),
            "Wc": w(ncls, n7, 1.0), "bc": (0.1 * rng.standard_normal(ncls)).astype(np.float32),
            "Wb": w(4 * ncls, n7, 0.5), "bb": (0.1 * rng.standard_normal(4 * ncls)).astype(np.float32)}


def random_blobs(seed, R, N, H, W, ncls):
    """rois inside N maps of H x W cells and the data layer's shapes: a quarter of the rows foreground (label > 0) with targets
    and weights in their class's four columns, the rest background."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x1 = rng.uniform(0, 16 * W - 40, R)
    y1 = rng.uniform(0, 16 * H - 40, R)
    x2 = np.minimum(x1 + rng.uniform(20, 16 * W * 0.7, R), 16 * W - 1)
    y2 = np.minimum(y1 + rng.uniform(20, 16 * H * 0.7, R), 16 * H - 1)
    rois = np.stack([np.sort(rng.integers(0, N, R)).astype(np.float64), x1, y1, x2, y2], 1).astype(np.float32)
    labels = np.where(rng.random(R) < 0.25, rng.integers(1, ncls, R), 0).astype(np.float32)
    if R > 1:
        labels[0], labels[-1] = ncls - 1, 0
    tgt = np.zeros((R, 4 * ncls), np.float32)
    wgt = np.zeros((R, 4 * ncls), np.float32)
    for r in np.where(labels > 0)[0]:
        c = int(labels[r])
        tgt[r, 4 * c:4 * c + 4] = (rng.standard_normal(4) * 1.5).astype(np.float32)
        wgt[r, 4 * c:4 * c + 4] = 1.0
    return {"rois": rois, "labels": labels, "bbox_targets": tgt, "bbox_loss_weights": wgt}


def case(name, seed=7):
    """(head, fmap [2, C, 12, 16], blobs) of one of HEADS."""
    from aznet_hip import synth
    d = HEADS[name]
    fmap = np.concatenate([synth.make_feature_map(s, d["C"], MAP_H, MAP_W) for s in (seed, seed + 1)], axis=0)
    head = filler_head(seed, d["C"], d["n6"], d["n7"], d["ncls"])
    return head, fmap, random_blobs(seed, d["R"], 2, MAP_H, MAP_W, d["ncls"])


def step_masks(seed, it, n, head, ratios=(0.5, 0.5)):
    from aznet_hip import ffi
    return {t: ffi.dropout_mask(seed, it, l, n * head[k].shape[0], ratio=ratios[l]).reshape(n, -1)
            for t, l, k in LAYERS if ratios[l] > 0}


def gate_mismatch(pre_a, pre_ref):
    return float(np.mean((np.asarray(pre_a) > 0) != (np.asarray(pre_ref) > 0)))


# ---- the 20-step run through detect.train_det.SolverWrapper (reduced head, width_div backbone, synthetic_375x500_8) ---------
# base_lr: found on the CPU (tests/test_det_train_host.py::test_frozen_run_restatement_lowers_the_loss prints the float64
# restatement's summed loss of the first and the last five steps at this value)
TRAJ = dict(n6=128, n7=96, solver_seed=3, steps=20, np_seed=5,
            solver=dict(base_lr=0.02, lr_policy="step", gamma=0.5, stepsize=10, momentum=0.9, weight_decay=0.0005,
                        clip_gradients=20.0, display=5, average_loss=5, snapshot_prefix="frcnn_small"))
traj_backbone = R.traj_backbone                  # (the AZ trajectory's frozen width_div = 32 backbone: C = 16)
TorchBlobCtx = R.TorchBlobCtx


def traj_solver_files(dirname, frozen_all=True, edit_rows=None):
    """edit_rows: a function on the rows of prototxt.det_layer_table, applied before the train net is written."""
    import os
    from detect import prototxt as P
    net = os.path.join(dirname, "train_det.prototxt")
    rows = P.det_layer_table(frozen=P.CONV_LAYERS if frozen_all else P.CONV_LAYERS[:4])
    P.write_train_prototxt(net, rows if edit_rows is None else edit_rows(rows), name="frcnn_train")
    sol = os.path.join(dirname, "solver_det.prototxt")
    P.write_solver_prototxt(sol, net, **TRAJ["solver"])
    return sol


class RefTrajectory(object):
    """The restatement stepping beside a device run: same start, same minibatches, same conv5_3 maps, same masks."""

    def __init__(self, params, dtype, solver, ratios=(0.5, 0.5), lr_mult=LR_MULT, decay_mult=DECAY_MULT):
        self.dt = dtype
        self.p = {k: np.asarray(v, dtype) for k, v in params.items()}
        self.h = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.sp = dict(solver)
        self.it = 0
        self.ratios, self.lr_mult, self.decay_mult = tuple(ratios), lr_mult, decay_mult

    def step(self, conv, blobs, seed, gates=None):
        pool, _ = roi_pool(conv, blobs["rois"])
        masks = step_masks(seed, self.it, pool.shape[0], self.p, self.ratios)
        r = step(self.p, pool, blobs, masks, gates=gates, dtype=self.dt, ratios=self.ratios, want_dpool=False)
        rate = learning_rate(self.sp["lr_policy"], self.sp["base_lr"], self.it, self.sp["gamma"], self.sp["stepsize"])
        self.p, self.h = sgd(self.p, r["grads"], self.h, rate, self.sp["momentum"], self.sp["weight_decay"],
                             clip_scale(r["sumsq"], self.sp["clip_gradients"]), dtype=self.dt, lr_mult=self.lr_mult,
                             decay_mult=self.decay_mult)
        self.it += 1
        return r
