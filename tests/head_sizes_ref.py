"""Cases for the two inference heads at layer sizes other than the reduced and the full one (test infrastructure, plain
NumPy; the yardstick of tests/test_head_sizes_host.py and tests/test_gpu_head_sizes.py).

Two kinds of head per size set, on conv maps of 24 x 32 cells with 300 rois of a 384 x 512 image:

  * integer-exact: the map holds integers 0..3 (about half zeros), W6 / W71 / W72 / Wab (detection: W6 / W7 / Wb) are
    ternary {-1, 0, 1} at density 0.25, the biases small integers, and the score layers (Was, Wz; detection: Wc) ternary
    times ONE power of two 2^-k per case, their biases integers times 2^-k.  Every product and every partial sum, in any
    order, is an integer below 2^24 (asserted: `abs_sum`), hence exact in fp32, in two fp16 terms and in three bf16 terms:
    no summation order, K split, kernel or GEMM mode can change a bit of a pre-activation.  The reference is a float64
    evaluation (exact: integers below 2^53) cast to float32.  k is the smallest for which max |pre-sigmoid| (|pre-softmax|)
    is at most 4.  The score rows are as dense as the sensitivity condition allows: starting from density 0.25 (zoom_score,
    the only reader of int7_2: every column) the non-zeros per row of the layer that sets k are halved until one unit 2^-k
    at the largest |pre-activation| of each layer moves the float64 probability by more than 4 x the tolerance of the
    probability check (`unit_move` > 4 `tol`); the choice reads the reference only.
  * random: synth.make_head / make_det_head weights on a synth.make_feature_map map, with the float64 evaluation
    (f64_head, f64_det_head) that the tolerance rule of tests/test_gpu_train_step.py needs.

Tolerances are train_step_ref.bound: 8 x the error of the float32 restatement against float64, floor 1e-6."""
import numpy as np

import train_step_ref as R

MAP_H, MAP_W = 24, 32
IM_H, IM_W = 384, 512
ROWS = (1, 8, 16, 33, 40, 48, 130, 161, 300)

# (C, n6, n71, n72): what each is for is in tests/test_gpu_head_sizes.py
AZ_SIZES = ((4, 4, 4, 4), (12, 132, 68, 36), (44, 260, 132, 4), (336, 36, 8, 8), (4, 516, 3000, 72), (4, 2052, 8, 4),
            (4, 16388, 4, 4), (44, 8324, 8, 4), (256, 4096, 1024, 256))
AZ_LARGEST = (256, 4096, 1024, 256)
# (C, n6, n7, ncls)
DET_SIZES = ((4, 4, 4, 2), (12, 132, 100, 21), (44, 260, 516, 81), (4, 2052, 2052, 256))
AZ_REFUSED_LDS = (4, 516, 3004, 72)


def fc_split(K):
    """The number of K chunks of a layer (include/aznet_hip.h: part of a row's bits)."""
    return 16 if K >= 16384 else 8 if K >= 2048 else 2 if K >= 512 else 1


def rois300(seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = 300
    x1 = rng.uniform(0, IM_W - 40, n)
    y1 = rng.uniform(0, IM_H - 40, n)
    x2 = np.minimum(x1 + rng.uniform(16, 0.8 * IM_W, n), IM_W - 1)
    y2 = np.minimum(y1 + rng.uniform(16, 0.8 * IM_H, n), IM_H - 1)
    return np.stack([np.zeros(n), x1, y1, x2, y2], 1).astype(np.float32)


def int_map(seed, C):
    """[1, C, 24, 32] float32 of integers 0..3, about half zeros."""
    rng = np.random.Generator(np.random.PCG64(20_000 + seed))
    a = rng.integers(1, 4, (1, C, MAP_H, MAP_W), dtype=np.int8)
    a[rng.random(a.shape, dtype=np.float32) < 0.5] = 0
    return a.astype(np.float32)


def ternary(rng, n_out, n_in, density=0.25):
    """{-1, 0, 1}, a quarter of the entries non-zero (or the share `density` = 2 / an integer)."""
    t = rng.integers(0, int(round(2.0 / density)), (n_out, n_in), dtype=np.int8)
    return (t == 0).astype(np.float32) - (t == 1).astype(np.float32)


def sparse_rows(rng, n_out, n_in, nnz):
    """{-1, 0, 1} with exactly `nnz` non-zeros in every row."""
    w = np.zeros((n_out, n_in), np.float32)
    for o in range(n_out):
        w[o, rng.choice(n_in, size=nnz, replace=False)] = rng.choice(np.float32([-1, 1]), size=nnz)
    return w


def small_ints(rng, n, lim=4):
    return rng.integers(-lim, lim + 1, n).astype(np.float32)


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def softmax64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def sigmoid32(x):
    """Caffe's Sigmoid in float32: f32 exp, f64 divide, f32 store."""
    e = np.exp(-np.asarray(x, np.float32))
    return (1.0 / (1.0 + e.astype(np.float64))).astype(np.float32)


def softmax32(x):
    """Caffe's Softmax in float32."""
    x = np.asarray(x, np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def _layer(x, W, b, relu, abs_sum, name):
    """Exact integer InnerProduct in float64, recording max sum |w||x| + |b| (the bound on every partial sum)."""
    W64 = W.astype(np.float64)
    abs_sum[name] = max(abs_sum.get(name, 0.0), float((np.abs(x) @ np.abs(W64).T + np.abs(b.astype(np.float64))).max()))
    y = x @ W64.T + b.astype(np.float64)
    assert np.array_equal(y, np.rint(y))
    return np.maximum(y, 0) if relu else y


def _score_layers(rng, feats, shapes, prob64, prob32):
    """The score layers of a case.  feats: {name: exact activations [R, n_in]}; shapes: ((name, n_out, feat name, starting
    density), ...); prob64 / prob32: {name: pre -> probabilities}.  While the sensitivity condition fails, the layer with the
    largest |integer pre-activation| (the one that sets k) gets half the non-zeros per row.  Returns the first choice that
    meets the condition, or the sparsest one tried (the host test asserts the condition)."""
    nnz = {name: max(1, int(round(dens * feats[f].shape[1]))) for name, _, f, dens in shapes}
    while True:
        sub = np.random.Generator(np.random.PCG64(int(rng.integers(1 << 62))))
        Wi = {name: sparse_rows(sub, n_out, feats[f].shape[1], nnz[name]) for name, n_out, f, _ in shapes}
        bi = {name: small_ints(sub, n_out, 2) for name, n_out, f, _ in shapes}
        ints = {name: feats[f] @ Wi[name].astype(np.float64).T + bi[name] for name, _, f, _ in shapes}
        asum = {name: float((np.abs(feats[f]) @ np.abs(Wi[name]).astype(np.float64).T + np.abs(bi[name])).max()) for name, _, f, _ in shapes}
        tops = {name: float(np.abs(v).max()) for name, v in ints.items()}
        k = max(0, int(np.ceil(np.log2(max(max(tops.values()), 1.0) / 4.0))))
        unit = 2.0 ** -k
        out = {"k": k, "nnz": dict(nnz), "W": {}, "b": {}, "pre": {}, "p64": {}, "tol": {}, "unit_move": {}, "abs_sum": asum}
        ok = True
        for name in ints:
            pre = ints[name] * unit
            p64 = prob64[name](pre)
            tol = R.bound(R.rel_err(prob32[name](pre.astype(np.float32)), p64))
            r, c = np.unravel_index(int(np.abs(pre).argmax()), pre.shape)
            move = np.inf
            for step in (unit, -unit):                                 # (the smaller of the two directions)
                moved = pre[r:r + 1].copy()
                moved[0, c] += step
                move = min(move, float(np.abs(prob64[name](moved) - p64[r:r + 1]).max() / np.abs(p64).max()))
            out["W"][name], out["b"][name] = Wi[name] * np.float32(unit), bi[name] * np.float32(unit)
            out["pre"][name], out["p64"][name], out["tol"][name], out["unit_move"][name] = pre, p64, tol, move
            ok &= move > 4.0 * tol
        dense = [name for name in nnz if nnz[name] > 1]
        if ok or not dense:
            return out
        worst = max(dense, key=lambda name: tops[name])
        nnz[worst] //= 2


def int_az_case(dims, seed=0, pool=None):
    """The integer-exact AZ head of one size set on the 300 rois.  `pool`: RoIPool, (fmap [1,C,H,W], rois) -> [R, C*49]
    (default: the NumPy restatement of train_step_ref)."""
    C, n6, n71, n72 = dims
    rng = np.random.Generator(np.random.PCG64(1000 * C + n6 + seed))
    fmap, rois = int_map(seed + C, C), rois300()
    p5 = (pool or (lambda f, r: R.roi_pool(f, r)[0]))(fmap, rois)
    head = {"W6": ternary(rng, n6, C * 49), "b6": small_ints(rng, n6), "W71": ternary(rng, n71, n6), "b71": small_ints(rng, n71),
            "W72": ternary(rng, n72, n6), "b72": small_ints(rng, n72), "Wab": ternary(rng, 44, n71), "bab": small_ints(rng, 44)}
    asum = {}
    h6 = _layer(p5.astype(np.float64), head["W6"], head["b6"], True, asum, "int6")
    h71 = _layer(h6, head["W71"], head["b71"], True, asum, "int7")
    h72 = _layer(h6, head["W72"], head["b72"], True, asum, "int7")
    bbox = _layer(h71, head["Wab"], head["bab"], False, asum, "tail")
    s = _score_layers(rng, {"h71": h71, "h72": h72}, (("adj", 11, "h71", 0.25), ("zoom", 1, "h72", 1.0)),
                      {"adj": sigmoid64, "zoom": sigmoid64}, {"adj": sigmoid32, "zoom": sigmoid32})
    head.update(Was=s["W"]["adj"], bas=s["b"]["adj"], Wz=s["W"]["zoom"], bz=s["b"]["zoom"])
    asum["tail"] = max(asum["tail"], s["abs_sum"]["adj"], s["abs_sum"]["zoom"])
    return {"dims": dims, "head": {k: np.ascontiguousarray(v, np.float32) for k, v in head.items()}, "fmap": fmap, "rois": rois,
            "pool5": p5, "k": s["k"], "nnz": s["nnz"], "abs_sum": asum, "bbox": bbox.astype(np.float32),
            "pre": s["pre"], "p64": s["p64"], "tol": s["tol"], "unit_move": s["unit_move"]}


def int_det_case(dims, seed=0, pool=None, rois=None, density=0.25):
    """The integer-exact detection head of one size set on the 300 rois (or on `rois`, with W6 / W7 / Wb at `density`:
    tests/det_rows_ref.py)."""
    C, n6, n7, ncls = dims
    rng = np.random.Generator(np.random.PCG64(1000 * C + n6 + 7 * ncls + seed))
    fmap, rois = int_map(seed + C, C), rois300() if rois is None else rois
    p5 = (pool or (lambda f, r: R.roi_pool(f, r)[0]))(fmap, rois)
    head = {"W6": ternary(rng, n6, C * 49, density), "b6": small_ints(rng, n6), "W7": ternary(rng, n7, n6, density),
            "b7": small_ints(rng, n7), "Wb": ternary(rng, 4 * ncls, n7, density), "bb": small_ints(rng, 4 * ncls)}
    asum = {}
    h6 = _layer(p5.astype(np.float64), head["W6"], head["b6"], True, asum, "fc6")
    h7 = _layer(h6, head["W7"], head["b7"], True, asum, "fc7")
    bbox = _layer(h7, head["Wb"], head["bb"], False, asum, "tail")
    s = _score_layers(rng, {"h7": h7}, (("cls", ncls, "h7", 0.25),), {"cls": softmax64}, {"cls": softmax32})
    head.update(Wc=s["W"]["cls"], bc=s["b"]["cls"])
    asum["tail"] = max(asum["tail"], s["abs_sum"]["cls"])
    return {"dims": dims, "head": {k: np.ascontiguousarray(v, np.float32) for k, v in head.items()}, "fmap": fmap, "rois": rois,
            "pool5": p5, "k": s["k"], "nnz": s["nnz"], "abs_sum": asum, "bbox": bbox.astype(np.float32),
            "pre": s["pre"], "p64": s["p64"], "tol": s["tol"], "unit_move": s["unit_move"]}


# ---- random cases ---------------------------------------------------------------------------------------------------------
def random_az_case(dims, seed=0):
    from aznet_hip import synth
    C, n6, n71, n72 = dims
    return {"dims": dims, "head": synth.make_head(seed=300 + seed + C + n6, C=C, n6=n6, n71=n71, n72=n72),
            "fmap": synth.make_feature_map(40 + seed + C, C, MAP_H, MAP_W), "rois": rois300()}


def random_det_case(dims, seed=0):
    from aznet_hip import synth
    C, n6, n7, ncls = dims
    return {"dims": dims, "head": synth.make_det_head(seed=500 + seed + C + n6, C=C, n6=n6, n7=n7, ncls=ncls),
            "fmap": synth.make_feature_map(40 + seed + C, C, MAP_H, MAP_W), "rois": rois300()}


def _fc64(x, W, b, relu):
    y = x @ W.astype(np.float64).T + b.astype(np.float64)
    return np.maximum(y, 0) if relu else y


def f64_head_on_pool5(head, pool5):
    """(zoom_prob, adj_prob, adj_bbox) of the AZ head in float64 from pooled rows [R, C*49]."""
    h6 = _fc64(np.asarray(pool5, np.float64), head["W6"], head["b6"], True)
    h71 = _fc64(h6, head["W71"], head["b71"], True)
    h72 = _fc64(h6, head["W72"], head["b72"], True)
    return sigmoid64(_fc64(h72, head["Wz"], head["bz"], False)), sigmoid64(_fc64(h71, head["Was"], head["bas"], False)), \
        _fc64(h71, head["Wab"], head["bab"], False)


def f64_head(orc, head, fmap, rois):
    """The AZ head in float64 on the oracle's RoIPool."""
    return f64_head_on_pool5(head, orc.roi_pool(fmap[0], rois).reshape(rois.shape[0], -1))


def f64_det_head(orc, head, fmap, rois):
    """(cls_prob, bbox_pred) of the detection head in float64 on the oracle's RoIPool."""
    p5 = orc.roi_pool(fmap[0], rois).reshape(rois.shape[0], -1).astype(np.float64)
    h7 = _fc64(_fc64(p5, head["W6"], head["b6"], True), head["W7"], head["b7"], True)
    return softmax64(_fc64(h7, head["Wc"], head["bc"], False)), _fc64(h7, head["Wb"], head["bb"], False)
