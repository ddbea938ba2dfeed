"""References and cases for the truncated-SVD detection head (test infrastructure, plain NumPy; the yardstick of
tests/test_lowrank_host.py and tests/test_gpu_lowrank.py; the sizes other than DIMS, SIZES below: tests/test_lowrank_sizes_host.py
and tests/test_gpu_lowrank_sizes.py).

  * compress_layer restated: U, s, Vt = svd(W) in float64, L = diag(s[:r]) Vt[:r], U = U[:, :r], cast to float32 once.
  * the two-stage head on pooled rows in float64 and in float32: a layer given as (L, U, b) is t = L x (no bias, no
    ReLU), y = relu(U t + b); a layer given as (W, b) is y = relu(W x + b); cls_score + Softmax and bbox_pred as ever.
    RoIPool, decode and the dedup come from what the suite already has (the oracle, det_infer_ref, pyramid_ref, skip_ref).
  * integer cases: operands for the U-stage kernel alone, and heads whose factors are small integers, so that
    W = U L and every intermediate of either evaluation is an integer below 2^24 -- exact in float32 in any order.

Tolerances are train_step_ref.bound: 8 x the float32 restatement's own error against float64, floor 1e-6."""
import numpy as np

import head_sizes_ref as H

DIMS = (44, 260, 516)                    # C, n6, n7 of the reduced head these tests use (K6 = 2156: 8 chunks at full rank)
RANKS = (4, 36, 128)
EXACT = float(1 << 24)

# the U-stage kernel alone: tiles of 64 x 64, K steps of 32
UNIT_M = (1, 31, 32, 33, 63, 65, 257)    # + max_rois of the small context
UNIT_N = (4, 36, 132, 260, 516)
UNIT_K = (4, 36, 64, 100, 256, 260, 1024, 2048)
UNIT_CAP = 320                           # max_regions of the small context
UNIT_GUARD = 64                          # rows behind row M that az_lowrank_gemm_unit checks: its launch is sized for M + 64
LR_TILE, LR_GRID = 64, 1024              # k_lowrank_gemm's tile edge and the launcher's cap on the grid

# ---- off the one size (tests/test_lowrank_sizes_host.py, tests/test_gpu_lowrank_sizes.py) ------------------------------------
# name: ((C, n6, n7), max_regions, ((ncls, r6, r7), ...)); what each reaches is in tests/test_gpu_lowrank_sizes.py
SIZES = {
    "WIDE": ((4, 2116, 8), 2304, ((21, 36, 0), (21, 4, 4))),
    "DEEP": ((160, 260, 516), 512, ((21, 36, 0), (81, 132, 132), (21, 260, 256))),
    "TINY": ((4, 8, 8), 64, ((2, 4, 4), (21, 8, 0), (21, 0, 8))),
    "LONG": ((672, 132, 8), 64, ((21, 132, 0), (21, 128, 0))),
    "DIMS": (DIMS, 512, ((21, 132, 0), (81, 260, 260), (21, 0, 256), (21, 256, 132))),
}
WIDE_ROWS = (1, 64, 65, 300, 1024, 1025, 1984, 2047, 2048)        # rois[:n] and rois[2048 - n:]
TINY_ROWS = (1, 31, 64)                 # TINY and LONG
SECOND_TURN = slice(1920, 2048)          # WIDE at 2048 rows: m-tiles 30 and 31 are the 64 workgroups' second items
# the U-stage kernel alone on a context of 2304 regions: (M, N, K), then (M of the operands, the row counts M' <= M run on them)
UNIT_BIG_CAP = 2304
UNIT_BIG = ((2112, 2116, 4), (2112, 2116, 36), (2112, 2116, 100), (2240, 2052, 36))
UNIT_BIG_MASKED = ((2112, 2116, 36), (2049, 1985))
# random heads: (size, r6, r7)
RANDOM_SIZES = (("DEEP", 132, 132), ("DIMS", 260, 260))
RANDOM_WIDE = (36, 0)
CHUNK = 160                              # the reference launches of the WIDE random head: 3 m-tiles x 34 n-tiles, one turn
FEW = ((2000, 1), (2000, 161), (2000, 2000))
BATCHES = ((1000, 1000), (300, 700, 1048))
# the loads of part 5, in order: (r6, r7) or None for the full head
LOAD_ORDER = ((260, 260), (4, 0), None, (0, 256))


def tiles(M, N, capM):
    """The launcher's arithmetic restated: (n-tiles, m-tiles of the M rows the device finds, workgroups launched)."""
    nt, mt = -(-N // LR_TILE), -(-M // LR_TILE)
    return nt, mt, max(1, min(-(-capM // LR_TILE) * nt, LR_GRID))


def fc_chunk(K, S):
    """azk_fc_chunk: ceil(K / S) rounded up to the GEMM's K step."""
    return (-(-K // S) + 31) // 32 * 32


def split_ref(K, r):
    """azk_lowrank_split restated: 512 // (n-tiles of 128) chunks at most, counted with chunks of at least 128."""
    S = max(512 // (-(-r // 128)), 1)
    return -(-K // max(fc_chunk(K, S), 128))


def size_rois(name):
    """The roi set of a size: WIDE all of det_rows_ref.rois2048; DEEP and DIMS rois300 followed by the first 512 of
    rois2048 (two launches on a context of 512 regions); TINY and LONG the first 64 of rois300."""
    import det_rows_ref as DR
    if name == "WIDE":
        return DR.rois2048()
    if name in ("TINY", "LONG"):
        return H.rois300()[:64]
    return np.concatenate([H.rois300(), DR.rois2048()[:512]], 0)


def layer_shapes(name, r6, r7):
    """((K, r) of each L stage, (N, K) of each U stage) of a head of that size."""
    C, n6, n7 = SIZES[name][0]
    Ls = [(K, r) for K, r in ((49 * C, r6), (n6, r7)) if r]
    Us = [(N, r) for N, r in ((n6, r6), (n7, r7)) if r]
    return Ls, Us


def compress_layer(W, r):
    """(L [r, in], U [out, r]) float32: the definition, in NumPy's float64 SVD."""
    U, s, Vt = np.linalg.svd(np.asarray(W, np.float64), full_matrices=False)
    return np.ascontiguousarray(s[:r, None] * Vt[:r], np.float32), np.ascontiguousarray(U[:, :r], np.float32)


def planted_spectrum(n_out, n_in, s, seed):
    """W [out, in] float64 with singular values exactly s (descending, len = min(out, in)): Q1 diag(s) Q2^T."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = min(n_out, n_in)
    q1 = np.linalg.qr(rng.standard_normal((n_out, k)))[0]
    q2 = np.linalg.qr(rng.standard_normal((n_in, k)))[0]
    return (q1 * np.asarray(s, np.float64)[None, :]) @ q2.T


def _layer(x, head, i, dtype):
    b = np.asarray(head["b%d" % i], dtype)
    if "L%d" % i in head:
        t = x @ np.asarray(head["L%d" % i], dtype).T
        y = t @ np.asarray(head["U%d" % i], dtype).T + b
    else:
        y = x @ np.asarray(head["W%d" % i], dtype).T + b
    return np.maximum(y, 0).astype(dtype)


def head_on_pool5(head, p5, dtype):
    """(cls_prob, bbox_pred) of the (possibly compressed) detection head on pooled rows [R, C*49], every operation in
    `dtype` (float32: Caffe's Softmax as the oracle states it)."""
    h7 = _layer(_layer(np.asarray(p5, dtype), head, 6, dtype), head, 7, dtype)
    s = h7 @ np.asarray(head["Wc"], dtype).T + np.asarray(head["bc"], dtype)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True, dtype=dtype)).astype(dtype)
    return p, (h7 @ np.asarray(head["Wb"], dtype).T + np.asarray(head["bb"], dtype)).astype(dtype)


def product_head(head):
    """The full-rank head whose weights are the products U L of a compressed head's factors (float64 product, cast)."""
    out = {k: v for k, v in head.items() if k[0] not in "LU"}
    for i in (6, 7):
        if "L%d" % i in head:
            out["W%d" % i] = (head["U%d" % i].astype(np.float64) @ head["L%d" % i].astype(np.float64)).astype(np.float32)
    return out


# ---- the U-stage kernel alone ---------------------------------------------------------------------------------------------
def unit_case(M, N, K, seed=0):
    """Integer X [M, K] in 0..3, ternary W [N, K] with 16 non-zeros per row (or K), integer bias: every partial sum an
    integer of magnitude <= 3 * 16 + 8.  -> X, W, b, Y64 (pre-activation, exact)."""
    rng = np.random.Generator(np.random.PCG64(977 * M + 31 * N + K + seed))
    X = rng.integers(0, 4, (M, K)).astype(np.float32)
    W = H.sparse_rows(rng, N, K, min(K, 16))
    b = H.small_ints(rng, N, 8)
    Y = X.astype(np.float64) @ W.astype(np.float64).T + b
    assert float((np.abs(X) @ np.abs(W).T).max()) + 8 < EXACT
    return X, W, b, Y


# ---- planted exact factorisations -----------------------------------------------------------------------------------------
def planted_head(ncls, r6, r7, seed=0, pool=None, dims=None, rois=None):
    """A reduced head (DIMS, or `dims` = (C, n6, n7), on rois300 or on `rois`) whose compressed layers have small-integer factors: L rows with 64 (fc6) / 8 (fc7) entries
    +-1, U rows with min(r, 8) entries +-1, integer biases; a layer of rank 0 is a sparse integer W.  bbox_pred is sparse
    integer, cls_score sparse integer times 2^-k with max |logit| <= 4.  Returns the case: head (factors), full (the
    product head), fmap, rois, pool5, bbox (exact, float32), p64 (float64 softmax of the exact logits), abs_sum (the bound
    on every partial sum of either evaluation, asserted below 2^24)."""
    C, n6, n7 = dims or DIMS
    rng = np.random.Generator(np.random.PCG64(5000 + 100 * r6 + r7 + 7 * ncls + seed + (0 if (dims or DIMS) == DIMS else 1000 * C + n6)))
    fmap, rois = H.int_map(seed + C, C), H.rois300() if rois is None else rois
    p5 = (pool or (lambda f, r: __import__("train_step_ref").roi_pool(f, r)[0]))(fmap, rois).astype(np.float64)
    p5 = p5.reshape(rois.shape[0], -1)
    head, asum = {}, 0.0

    def stage(x, W, b=None):
        nonlocal asum
        W64 = W.astype(np.float64)
        asum = max(asum, float((np.abs(x) @ np.abs(W64).T).max()) + (0.0 if b is None else float(np.abs(b).max())))
        y = x @ W64.T + (0.0 if b is None else b.astype(np.float64))
        assert np.array_equal(y, np.rint(y))
        return y

    x = p5
    for i, r, n_out, nnz_in in ((6, r6, n6, 64), (7, r7, n7, 8)):
        b = H.small_ints(rng, n_out)
        n_in = x.shape[1]
        if r:
            Lf, U = H.sparse_rows(rng, r, n_in, nnz_in), H.sparse_rows(rng, n_out, r, min(r, 8))
            head["L%d" % i], head["U%d" % i] = Lf, U
            # (the full head sums |W||x| with W = U L, which |U| (|L| |x|) bounds)
            asum = max(asum, float(((np.abs(x) @ np.abs(Lf).astype(np.float64).T) @ np.abs(U).astype(np.float64).T).max())
                       + float(np.abs(b).max()))
            y = stage(stage(x, Lf), U, b)
        else:
            W = H.sparse_rows(rng, n_out, n_in, nnz_in)
            head["W%d" % i] = W
            y = stage(x, W, b)
        head["b%d" % i] = b
        x = np.maximum(y, 0)
    Wb, bb = H.sparse_rows(rng, 4 * ncls, n7, 8), H.small_ints(rng, 4 * ncls)
    bbox = stage(x, Wb, bb)
    Wc, bc = H.sparse_rows(rng, ncls, n7, 2), H.small_ints(rng, ncls, 2)
    logit = stage(x, Wc, bc)
    k = max(0, int(np.ceil(np.log2(max(float(np.abs(logit).max()), 1.0) / 4.0))))
    unit = np.float32(2.0 ** -k)
    head.update(Wb=Wb, bb=bb, Wc=Wc * unit, bc=bc * unit)
    assert asum < EXACT, asum
    head = {key: np.ascontiguousarray(v, np.float32) for key, v in head.items()}
    return {"head": head, "full": product_head(head), "fmap": fmap, "rois": rois, "pool5": p5.astype(np.float32),
            "bbox": bbox.astype(np.float32), "p64": H.softmax64(logit * float(unit)), "abs_sum": asum, "k": k}


# ---- random heads -----------------------------------------------------------------------------------------------------------
def random_case(r6, r7, ncls=21, seed=0, dims=None, rois=None):
    """synth.make_det_head at DIMS (or `dims`) compressed by the restated compress_layer, on a synth.make_feature_map map
    with rois300 (or `rois`)."""
    from aznet_hip import synth
    C, n6, n7 = dims or DIMS
    full = synth.make_det_head(seed=600 + seed, C=C, n6=n6, n7=n7, ncls=ncls)
    head = {k: v for k, v in full.items() if k not in ("W6", "W7")}
    for i, r in ((6, r6), (7, r7)):
        if r:
            head["L%d" % i], head["U%d" % i] = compress_layer(full["W%d" % i], r)
        else:
            head["W%d" % i] = full["W%d" % i]
    return {"head": head, "uncompressed": full, "fmap": synth.make_feature_map(40 + seed + C, C, H.MAP_H, H.MAP_W),
            "rois": H.rois300() if rois is None else rois}


def sized_planted(name, ncls, r6, r7, pool=None):
    """The planted head of a size of SIZES on that size's rois."""
    return planted_head(ncls, r6, r7, pool=pool, dims=SIZES[name][0], rois=size_rois(name))


def sized_random(name, r6, r7):
    return random_case(r6, r7, dims=SIZES[name][0], rois=size_rois(name))
