"""CPU restatements of the three training steps with bf16 OPERANDS (test infrastructure; the yardstick of
tests/test_bf16_host.py and tests/test_gpu_train_bf16.py).  The model of AZ_TRAIN_BF16 (include/aznet_hip.h): both operands
of EVERY matrix product -- forward, dx and dW of every layer, conv_pool5's three included -- are rounded to bfloat16 (nearest,
ties to even; ffi.bf16_round on the float32 value) and the products are summed exactly (`dtype` float64, the reference) or in
float32 (what sets the tolerance: train_step_ref.bound).  Everything that is no matrix product -- pooling, bias, ReLU,
dropout, column sums, losses, GRN, the norm and the update -- is the unchanged piece of det_step_ref / train_step_ref /
skip_train_ref.  The graphs are those restatements' own; only `mm` is new."""
import numpy as np

import det_step_ref as D
import skip_train_ref as K
import solver_edges_ref as E
import train_step_ref as R
from det_step_ref import gate_mismatch, softmax_loss  # noqa: F401
from solver_edges_ref import gemm_abs_sum, gemm_operands  # noqa: F401
from train_step_ref import bound, rel_err, sigmoid_ce, smooth_l1  # noqa: F401


def q(x):
    """x with every element rounded to bfloat16 (through float32, as the device holds it), in x's dtype."""
    from aznet_hip import ffi
    x = np.asarray(x)
    return ffi.bf16_round(x.astype(np.float32)).astype(x.dtype)


def mm(a, b):
    """The product the device forms in bf16 mode, summed in the operands' dtype."""
    return q(a) @ q(b)


def _hidden_fns(dt, masks, gates, out):
    def hidden(x, W, b, tag, ratio):
        pre = mm(x, W.T) + b
        gate = (pre > 0) if gates is None else gates[tag].astype(bool)
        a = np.where(gate, pre, 0).astype(dt)
        sc = dt(1)
        if masks is not None and ratio > 0:
            sc = dt(1) / (dt(1) - dt(ratio))
            a = np.where(masks[tag].astype(bool), a * sc, 0).astype(dt)
        out["pre%d" % tag], out["a%d" % tag] = pre, a
        return a, gate, sc

    def back(d, gate, tag, sc, ratio):
        if masks is not None and ratio > 0:
            d = np.where(masks[tag].astype(bool), d * sc, 0)
        return np.where(gate, d, 0).astype(dt)
    return hidden, back


def det_step(params, pool5, blobs, masks, gates=None, dtype=np.float64, ratios=(0.5, 0.5), want_dpool=True):
    """det_step_ref.step with bf16 operands (same arguments, same names in the result)."""
    dt = dtype
    P = {k: np.asarray(params[k], dtype=dt) for k in D.KEYS}
    n = pool5.shape[0]
    ratios = [float(np.float32(r)) for r in ratios]
    out = {}
    hidden, back = _hidden_fns(dt, masks, gates, out)
    x = np.asarray(pool5, dtype=dt)
    a6, g6, s6 = hidden(x, P["W6"], P["b6"], 6, ratios[0])
    a7, g7, s7 = hidden(a6, P["W7"], P["b7"], 7, ratios[1])
    s_c = mm(a7, P["Wc"].T) + P["bc"]
    s_b = mm(a7, P["Wb"].T) + P["bb"]
    lc, d_c, prob = softmax_loss(s_c, blobs["labels"], dt(n))
    lb, d_b = smooth_l1(s_b, np.asarray(blobs["bbox_targets"], dt), np.asarray(blobs["bbox_loss_weights"], dt), dt(n))
    out.update(cls_score=s_c, cls_prob=prob, bbox_pred=s_b, d_cls_score=d_c, d_bbox_pred=d_b)
    out["losses"] = np.array([lc, lb], dtype=dt)
    g = {}
    g["Wc"], g["bc"] = mm(d_c.T, a7), d_c.sum(0)
    g["Wb"], g["bb"] = mm(d_b.T, a7), d_b.sum(0)
    d7 = back(mm(d_c, P["Wc"]) + mm(d_b, P["Wb"]), g7, 7, s7, ratios[1])
    g["W7"], g["b7"] = mm(d7.T, a6), d7.sum(0)
    d6 = back(mm(d7, P["W7"]), g6, 6, s6, ratios[0])
    g["W6"], g["b6"] = mm(d6.T, x), d6.sum(0)
    out.update(d_pre7=d7, d_pre6=d6)
    if want_dpool:
        out["d_pool5"] = mm(d6, P["W6"])
    out["grads"] = g
    out["sumsq"] = float(sum(np.sum(np.asarray(v, np.float64) ** 2) for v in g.values()))
    out["gates"] = {6: g6, 7: g7}
    return out


def det_forward_test(params, pool5, dtype=np.float64):
    z = np.zeros((pool5.shape[0], params["bb"].size))
    r = det_step(params, pool5, {"labels": np.zeros(pool5.shape[0]), "bbox_targets": z, "bbox_loss_weights": z}, None, dtype=dtype,
                 want_dpool=False)
    return r["cls_prob"], r["bbox_pred"]


def az_step(params, pool5, blobs, masks, gates=None, dtype=np.float64, ratios=(0.5, 0.5, 0.5), want_dpool=True):
    """train_step_ref.step with bf16 operands."""
    dt = dtype
    P = {k: np.asarray(params[k], dtype=dt) for k in R.KEYS}
    n = pool5.shape[0]
    ratios = [float(np.float32(r)) for r in ratios]
    out = {}
    hidden, back = _hidden_fns(dt, masks, gates, out)
    x = np.asarray(pool5, dtype=dt)
    a6, g6, s6 = hidden(x, P["W6"], P["b6"], 6, ratios[0])
    a71, g71, s71 = hidden(a6, P["W71"], P["b71"], 71, ratios[1])
    a72, g72, s72 = hidden(a6, P["W72"], P["b72"], 72, ratios[2])
    s_as = mm(a71, P["Was"].T) + P["bas"]
    s_ab = mm(a71, P["Wab"].T) + P["bab"]
    s_z = (mm(a72, P["Wz"].T) + P["bz"]).reshape(n)
    out.update(adj_score=s_as, adj_bbox=s_ab, zoom_score=s_z)
    lz, d_z = sigmoid_ce(s_z, np.asarray(blobs["zoom_labels"], dt).reshape(n), dt(n))
    la, d_as = sigmoid_ce(s_as, np.asarray(blobs["adj_labels"], dt), dt(n))
    lb, d_ab = smooth_l1(s_ab, np.asarray(blobs["adj_targets"], dt), np.asarray(blobs["adj_loss_weights"], dt), dt(n))
    out["losses"] = np.array([lz, la, lb], dtype=dt)
    out.update(d_zoom_score=d_z, d_adj_score=d_as, d_adj_bbox=d_ab)
    g = {}
    d_z2 = d_z.reshape(n, 1)
    g["Was"], g["bas"] = mm(d_as.T, a71), d_as.sum(0)
    g["Wab"], g["bab"] = mm(d_ab.T, a71), d_ab.sum(0)
    g["Wz"], g["bz"] = mm(d_z2.T, a72), d_z2.sum(0)
    d71 = back(mm(d_as, P["Was"]) + mm(d_ab, P["Wab"]), g71, 71, s71, ratios[1])
    d72 = back(mm(d_z2, P["Wz"]), g72, 72, s72, ratios[2])
    g["W71"], g["b71"] = mm(d71.T, a6), d71.sum(0)
    g["W72"], g["b72"] = mm(d72.T, a6), d72.sum(0)
    d6 = back(mm(d71, P["W71"]) + mm(d72, P["W72"]), g6, 6, s6, ratios[0])
    g["W6"], g["b6"] = mm(d6.T, x), d6.sum(0)
    out.update(d_pre71=d71, d_pre72=d72, d_pre6=d6)
    if want_dpool:
        out["d_pool5"] = mm(d6, P["W6"])
    out["grads"] = g
    out["sumsq"] = float(sum(np.sum(np.asarray(v, np.float64) ** 2) for v in g.values()))
    out["gates"] = {6: g6, 71: g71, 72: g72}
    return out


def front_forward(front, raw, Cs, dtype=np.float64, gate=None):
    """skip_train_ref.front_forward with conv_pool5's product in bf16 operands (GRN and scale unchanged)."""
    dt = dtype
    gain, eps = dt(front.get("gain", 1000.0)), dt(front.get("eps", 1e-10))
    off = K.offsets(Cs)
    x = np.asarray(raw, dt)
    cat, fac, tot = np.zeros_like(x), np.zeros((x.shape[0], len(Cs)), dt), np.zeros((x.shape[0], len(Cs)), dt)
    for i in range(len(Cs)):
        xi = x[:, off[i]:off[i + 1]]
        t = (xi * xi).sum(axis=1, dtype=dt) + eps
        f = np.where(t > 0, gain / np.sqrt(np.where(t > 0, t, 1)), 0).astype(dt)
        cat[:, off[i]:off[i + 1]] = xi * f[:, None]
        fac[:, i], tot[:, i] = f, t
    Wp = np.asarray(front["Wp"], dt).reshape(np.asarray(front["bp"]).size, -1)
    pre = mm(cat, Wp.T) + np.asarray(front["bp"], dt)
    g = (pre > 0) if gate is None else np.asarray(gate, bool)
    y = np.where(g, pre, 0).astype(dt)
    return dict(x=x, cat=cat, fac=fac, tot=tot, pre_pool=pre, gate_pool=g, y=y, pool5=K.flatten_caffe(y, x.shape[0] // 49), Wp=Wp)


def front_backward(fw, d_pool5, Cs, arg, rois, shapes, dtype=np.float64, want=None):
    """skip_train_ref.front_backward with g_Wp and d_cat in bf16 operands."""
    dt = dtype
    off = K.offsets(Cs)
    d_y = np.where(fw["gate_pool"], K.unflatten_caffe(np.asarray(d_pool5, dt), rois.shape[0]), 0).astype(dt)
    out = dict(d_y=d_y, g_Wp=mm(d_y.T, fw["cat"]), g_bp=d_y.sum(0))
    d_cat = mm(d_y, fw["Wp"])
    d_raw = np.zeros_like(d_cat)
    for i in range(len(Cs)):
        sl = slice(off[i], off[i + 1])
        x, dy, f, t = fw["x"][:, sl], d_cat[:, sl], fw["fac"][:, i], fw["tot"][:, i]
        s = (x * dy).sum(axis=1, dtype=dt)
        k = np.where(t > 0, s / np.where(t > 0, t, 1), 0).astype(dt)
        d_raw[:, sl] = f[:, None] * (dy - x * k[:, None])
    out.update(d_cat=d_cat, d_raw=d_raw)
    out["dmaps"] = K.scatter(d_raw, arg, Cs, rois, shapes, want)
    return out


def skip_step(params, front, maps, blobs, masks, gates=None, dtype=np.float64, ratios=(0.5, 0.5), pooled=None):
    """skip_train_ref.step with bf16 operands."""
    Cs = tuple(int(m.shape[1]) for m in maps)
    raw, arg = K.pool_argmax(maps, blobs["rois"]) if pooled is None else pooled
    fw = front_forward(front, raw, Cs, dtype, None if gates is None else gates["pool"])
    r = det_step(params, fw["pool5"], blobs, masks, gates=gates, dtype=dtype, ratios=ratios, want_dpool=True)
    bw = front_backward(fw, r["d_pool5"], Cs, arg, blobs["rois"], [m.shape for m in maps], dtype)
    r.update(raw=raw, skip_argmax=arg, cat=fw["cat"], pre_pool=fw["pre_pool"], pool5=fw["pool5"], d_y=bw["d_y"], d_cat=bw["d_cat"],
             d_raw=bw["d_raw"], dmaps=bw["dmaps"])
    r["grads"]["Wp"], r["grads"]["bp"] = bw["g_Wp"], bw["g_bp"]
    r["sumsq"] = float(sum(np.sum(np.asarray(v, np.float64) ** 2) for v in r["grads"].values()))
    r["gates"]["pool"] = fw["gate_pool"]
    return r


class DetTrajectory(D.RefTrajectory):
    """det_step_ref.RefTrajectory on the bf16 model."""

    def step(self, conv, blobs, seed, gates=None):
        pool, _ = R.roi_pool(conv, blobs["rois"])
        masks = D.step_masks(seed, self.it, pool.shape[0], self.p, self.ratios)
        r = det_step(self.p, pool, blobs, masks, gates=gates, dtype=self.dt, ratios=self.ratios, want_dpool=False)
        rate = R.learning_rate(self.sp["lr_policy"], self.sp["base_lr"], self.it, self.sp["gamma"], self.sp["stepsize"])
        self.p, self.h = R.sgd(self.p, r["grads"], self.h, rate, self.sp["momentum"], self.sp["weight_decay"],
                               R.clip_scale(r["sumsq"], self.sp["clip_gradients"]), dtype=self.dt, lr_mult=self.lr_mult,
                               decay_mult=self.decay_mult)
        self.it += 1
        return r


class AzTrajectory(R.RefTrajectory):
    """train_step_ref.RefTrajectory on the bf16 model."""

    def step(self, conv, blobs, seed, gates=None):
        from aznet_hip import ffi
        pool, _ = R.roi_pool(conv, blobs["rois"])
        n = pool.shape[0]
        masks = {t: ffi.dropout_mask(seed, self.it, l, n * self.p[k].shape[0], ratio=self.ratios[l]).reshape(n, -1)
                 for t, l, k in ((6, 0, "b6"), (71, 1, "b71"), (72, 2, "b72")) if self.ratios[l] > 0}
        r = az_step(self.p, pool, blobs, masks, gates=gates, dtype=self.dt, ratios=self.ratios, want_dpool=False)
        rate = R.learning_rate(self.sp["lr_policy"], self.sp["base_lr"], self.it, self.sp["gamma"], self.sp["stepsize"])
        self.p, self.h = R.sgd(self.p, r["grads"], self.h, rate, self.sp["momentum"], self.sp["weight_decay"],
                               R.clip_scale(r["sumsq"], self.sp["clip_gradients"]), dtype=self.dt, lr_mult=self.lr_mult,
                               decay_mult=self.decay_mult)
        self.it += 1
        return r


def az_forward_test(params, pool5, dtype=np.float64):
    n = pool5.shape[0]
    r = az_step(params, pool5, {"zoom_labels": np.zeros(n), "adj_labels": np.zeros((n, 11)), "adj_targets": np.zeros((n, 44)),
                                "adj_loss_weights": np.zeros((n, 44))}, None, dtype=dtype, want_dpool=False)
    return r["zoom_score"], r["adj_score"], r["adj_bbox"]


# ---- the cases --------------------------------------------------------------------------------------------------------------
# 1. integer operands in -8..8: exact in bf16, every partial sum below 2^24 (asserted in test_bf16_host.py)
INT_MN = ((1, 1), (127, 129), (128, 128), (129, 257), (130, 84), (37, 324))
INT_K = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 512, 513)    # edges of the fragment (8), the instruction (16), the
INT_BIG = E.GEMM_BIG                                                   # stage (32) and Kc; 2049 x 2049 x 5: 289 tiles, forms 0, 1
integer_draw = E.integer_draw

# 2. rounding: integers in 257..511 need 9 bits, bf16 keeps 8.  Odd values are ties: 257 -> 256 (down to even), 259 -> 260
# (up to even); both signs.  K <= 16 and |product| < 2^18: sums exact in float32.
ROUND_SHAPES = ((33, 40, 16), (5, 7, 3), (128, 130, 9))


def tie_draw(rng):
    return lambda s: (rng.integers(257, 512, s) * rng.choice((-1, 1), s)).astype(np.float32)


def mixed_draw(rng):
    """First call (a): bf16 values (integers in -8..8); second call (b): integers that need rounding."""
    calls = []

    def draw(s):
        calls.append(1)
        return E.integer_draw(rng)(s) if len(calls) == 1 else tie_draw(rng)(s)
    return draw


# 3. random operands
RANDOM_SHAPES = (E.GEMM_RANDOM, (128, 4096 // 32, 1568))


def normal_draw(rng):
    return lambda s: rng.standard_normal(s).astype(np.float32)


def rounded_product(form, a, b, dtype=np.float64):
    """The product of the form on bf16-rounded operands, summed in dtype."""
    a, b = q(a).astype(dtype), q(b).astype(dtype)
    return {0: lambda: a @ b.T, 1: lambda: a @ b, 2: lambda: a.T @ b}[form]()


# 4. step cases.  Seeds: the first of each list at which the float32 and the float64 restatement of the bf16 model agree on
# every ReLU gate (asserted in test_bf16_host.py).
DET_SEEDS = {"small": 7, "voc": 7, "coco": 7}
AZ_CASES = {"R5": dict(R=5, dims=None), "R130": dict(R=130, dims=None), "R37-odd": dict(R=37, dims=(12, 132, 68, 36))}
AZ_SEEDS = {"R5": 7, "R130": 7, "R37-odd": 7}
SKIP_SEED = 7


def det_case(name):
    return D.case(name, DET_SEEDS[name])


def az_case(name):
    c = AZ_CASES[name]
    return R.small_case(R=c["R"], seed=AZ_SEEDS[name], dims=c["dims"])


def skip_case():
    return K.case("small", SKIP_SEED)


def integer_det_head(seed, C, n6, n7, ncls):
    """A head of integers in -1..1 (biases 0) for pooled rows of integers in -2..2 with few non-zeros: every operand of the
    forward is exact in bf16 and every partial sum stays far below 2^24."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def w(no, ni):
        return rng.integers(-1, 2, (no, ni)).astype(np.float32)
    return {"W6": w(n6, C * 49), "b6": np.zeros(n6, np.float32), "W7": w(n7, n6), "b7": np.zeros(n7, np.float32),
            "Wc": w(ncls, n7), "bc": np.zeros(ncls, np.float32), "Wb": w(4 * ncls, n7), "bb": np.zeros(4 * ncls, np.float32)}
