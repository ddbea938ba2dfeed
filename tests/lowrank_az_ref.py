"""References and cases for the truncated-SVD int6 of the AZ head (test infrastructure, plain NumPy; the yardstick of
tests/test_lowrank_az_host.py and tests/test_gpu_lowrank_az.py; the detection head's twin is tests/lowrank_ref.py).

  * the AZ L stage's split restated (az_az_lowrank_split): the cheapest split that keeps the many-row GEMM eligible, else
    the detection head's rule (lowrank_ref.split_ref).
  * the two-stage head on pooled rows in float64 and in float32: int6 given as (L6, U6, b6) is t = L6 x (no bias, no ReLU),
    h6 = relu(U6 t + b6); the rest is the AZ head as tests/head_sizes_ref.py states it.
  * planted integer factors: L6 / U6 small integers, so that W6 = U6 L6 and every partial sum of either evaluation is an
    integer below 2^24 -- exact in float32 in any order; the layers behind int6 as head_sizes_ref.int_az_case makes them.
  * the zoom-exact factorisation of a search_limits_ref head: the planted zoom path of synth.make_object_head kept exact in
    the factors, the rest of W6 at rank r - 1, so that the planted tree of a frozen search case is the compressed head's too.

Tolerances are train_step_ref.bound: 8 x the float32 restatement's own error against float64, floor 1e-6."""
import numpy as np

import head_sizes_ref as H
import lowrank_ref as LR

EXACT = float(1 << 24)
SMALL = (16, 128, 64, 32)                # synth.SMALL_DIMS as (C, n6, n71, n72): K6 = 784
ODD = (44, 260, 132, 4)                  # of tests/test_gpu_head_sizes.py: K6 = 2156 (no multiple of 128), n6 no multiple of 64
RANKS = {SMALL: (4, 36, 128), ODD: (4, 36, 128, 132, 256)}
CAP = 2304                               # max_regions of the head tests' context
# the smallest int6 whose L stage the many-row GEMM takes at rank 128 (one n-tile: 256 chunks at least, of 64 at least, that
# divide K6 = 18816 = 32 x 588 -> 294 chunks of 64), on a head too narrow for its own int6 to take it (n6 = 132)
MANY = (384, 132, 8, 4)
MANY_RANK, MANY_ROWS = 128, (1, 160, 161, 300)
# both sides of gemm12_min_rows (161), and, at CAP rows and n6 = 260, 36 x 5 tiles of the U stage
ROWS = (1, 31, 32, 33, 64, 65, 160, 161, 300, 688, CAP)


def fc_chunk(K, S):
    """azk_fc_chunk: ceil(K / S) rounded up to the GEMM's K step."""
    return (-(-K // S) + 31) // 32 * 32


def fits12(N, K, S):
    """azk_fc_gemm12_fits (az_head12.hip): whole n-tiles of 128, at least 256 (n-tile, chunk) groups, whole K steps, whole
    chunks of at least two K steps."""
    Kc = fc_chunk(K, S)
    return N % 128 == 0 and (N // 128) * S >= 256 and K % 32 == 0 and Kc * S == K and Kc >= 64


def az_split_ref(K, r):
    """azk_az_lowrank_split restated: among the S for which the many-row kernel takes the layer [r][K], the one with the
    least 4 ceil(nt S / 256) (K / S) + nt S (the deepest of the kernel's 256 workgroups against the slab traffic; ties: the
    smaller S); where there is none, the detection head's split (on k_fc_splitk)."""
    if r % 128 == 0:
        nt = r // 128
        fit = [S for S in range(-(-256 // nt), K // 64 + 1) if fits12(r, K, S)]
        if fit:
            return min(fit, key=lambda S: (4 * -(-nt * S // 256) * (K // S) + nt * S, S))
    return LR.split_ref(K, r)


def rois_all():
    """CAP rois on the 384 x 512 image: det_rows_ref.rois2048 followed by the first 256 of rois300."""
    import det_rows_ref as DR
    return np.concatenate([DR.rois2048(), H.rois300()[:CAP - 2048]], 0)


def head_on_pool5(head, p5, dtype):
    """(zoom_prob [R, 1], adj_prob [R, 11], adj_bbox [R, 44]) of the (possibly compressed) AZ head on pooled rows
    [R, C*49], every operation in `dtype` (float32: Caffe's Sigmoid as head_sizes_ref states it)."""
    f = lambda k: np.asarray(head[k], dtype)          # noqa: E731
    x = np.asarray(p5, dtype)
    if "L6" in head:
        y = (x @ f("L6").T).astype(dtype) @ f("U6").T + f("b6")
    else:
        y = x @ f("W6").T + f("b6")
    h6 = np.maximum(y, 0).astype(dtype)
    h71 = np.maximum(h6 @ f("W71").T + f("b71"), 0).astype(dtype)
    h72 = np.maximum(h6 @ f("W72").T + f("b72"), 0).astype(dtype)
    sig = H.sigmoid64 if dtype == np.float64 else H.sigmoid32
    return sig(h72 @ f("Wz").T + f("bz")), sig(h71 @ f("Was").T + f("bas")), (h71 @ f("Wab").T + f("bab")).astype(dtype)


def product_head(head):
    """The full-rank head whose W6 is the product U6 L6 of a compressed head's factors (float64 product, cast)."""
    out = {k: v for k, v in head.items() if k not in ("L6", "U6")}
    out["W6"] = (head["U6"].astype(np.float64) @ head["L6"].astype(np.float64)).astype(np.float32)
    return out


def compress_head(full, r6):
    """The head dict with W6 replaced by lowrank_ref.compress_layer's factors (the definition, NumPy's float64 SVD)."""
    out = {k: v for k, v in full.items() if k != "W6"}
    out["L6"], out["U6"] = LR.compress_layer(full["W6"], r6)
    return out


# ---- planted exact factorisations ---------------------------------------------------------------------------------------
def planted_az_head(dims, r6, seed=0, pool=None, rois=None):
    """An AZ head of size `dims` on `rois` (default rois_all) whose int6 has small-integer factors: L6 rows with
    min(64, K6) entries +-1, U6 rows with min(r6, 8) entries +-1, integer b6; int7_1, int7_2, adj_bbox ternary with integer
    biases and the score layers ternary times one power of two, as head_sizes_ref.int_az_case makes them.  Returns head
    (factors), full (the product head), fmap, rois, bbox (exact, float32), p64 {zoom, adj} (float64 sigmoid of the exact
    scores), abs_sum (the bound on every partial sum of either evaluation, asserted below 2^24)."""
    C, n6, n71, n72 = dims
    rng = np.random.Generator(np.random.PCG64(7000 + 1000 * C + n6 + 13 * r6 + seed))
    fmap, rois = H.int_map(seed + C, C), rois_all() if rois is None else rois
    p5 = (pool or (lambda f, r: __import__("train_step_ref").roi_pool(f, r)[0]))(fmap, rois).astype(np.float64)
    p5 = p5.reshape(rois.shape[0], -1)
    K6 = C * 49
    Lf, U, b6 = H.sparse_rows(rng, r6, K6, min(64, K6)), H.sparse_rows(rng, n6, r6, min(r6, 8)), H.small_ints(rng, n6)
    aL = np.abs(p5) @ np.abs(Lf).astype(np.float64).T
    aU = aL @ np.abs(U).astype(np.float64).T + float(np.abs(b6).max())     # (also bounds the full head's sums with W = U L)
    t = p5 @ Lf.astype(np.float64).T
    h6 = np.maximum(t @ U.astype(np.float64).T + b6, 0)
    assert np.array_equal(h6, np.rint(h6))
    head = {"L6": Lf, "U6": U, "b6": b6, "W71": H.ternary(rng, n71, n6), "b71": H.small_ints(rng, n71),
            "W72": H.ternary(rng, n72, n6), "b72": H.small_ints(rng, n72), "Wab": H.ternary(rng, 44, n71),
            "bab": H.small_ints(rng, 44)}
    asum = {"int6": max(float(aL.max()), float(aU.max()))}
    h71 = H._layer(h6, head["W71"], head["b71"], True, asum, "int7")
    h72 = H._layer(h6, head["W72"], head["b72"], True, asum, "int7")
    bbox = H._layer(h71, head["Wab"], head["bab"], False, asum, "tail")
    s = H._score_layers(rng, {"h71": h71, "h72": h72}, (("adj", 11, "h71", 0.25), ("zoom", 1, "h72", 1.0)),
                        {"adj": H.sigmoid64, "zoom": H.sigmoid64}, {"adj": H.sigmoid32, "zoom": H.sigmoid32})
    head.update(Was=s["W"]["adj"], bas=s["b"]["adj"], Wz=s["W"]["zoom"], bz=s["b"]["zoom"])
    asum["tail"] = max(asum["tail"], s["abs_sum"]["adj"], s["abs_sum"]["zoom"])
    assert max(asum.values()) < EXACT, asum
    head = {k: np.ascontiguousarray(v, np.float32) for k, v in head.items()}
    return {"dims": dims, "r6": r6, "head": head, "full": product_head(head), "fmap": fmap, "rois": rois,
            "pool5": p5.astype(np.float32), "bbox": bbox.astype(np.float32), "p64": s["p64"], "abs_sum": asum, "k": s["k"]}


# ---- random heads ---------------------------------------------------------------------------------------------------------
def random_az_case(dims, r6, seed=0):
    """head_sizes_ref.random_az_case with int6 compressed at rank r6 by the restated compress_layer, on rois300."""
    c = H.random_az_case(dims, seed)
    c["uncompressed"] = c["head"]
    c["head"] = compress_head(c["head"], r6)
    c["r6"] = r6
    return c


# ---- the zoom-exact factorisation of a planted search head ------------------------------------------------------------------
def zoom_exact_factors(head, r6, zoom_channel=0):
    """The compressed twin of a synth.make_object_head head (rows 0 and 1 of W6 are the 0/1 indicator row of the zoom
    channel) that keeps the zoom path exact:
        L6 row 0 = that indicator row;  U6 column 0 = 1 in rows 0 and 1, 0 elsewhere;  rows 0 and 1 of U6 are 0 outside
        column 0;  the remaining factors = the rows 2.. of W6 at rank r6 - 1 (compress_layer).
    Then t[0] = s is a sum of 0/1 values (exact in any order), int6 units 0 and 1 are relu(s + b6[0]) and relu(s + b6[1])
    exactly as in the full head, and the zoom score -- which reads those two units only (noise = 0) -- keeps its bits: the
    planted tree of the case is the compressed head's tree."""
    W6 = np.asarray(head["W6"], np.float32)
    n6, K6 = W6.shape
    ind = np.zeros(K6, np.float32)
    ind[zoom_channel * 49:(zoom_channel + 1) * 49] = 1.0
    assert np.array_equal(W6[0], ind) and np.array_equal(W6[1], ind)
    Lr, Ur = LR.compress_layer(W6[2:], r6 - 1)
    L6 = np.zeros((r6, K6), np.float32)
    U6 = np.zeros((n6, r6), np.float32)
    L6[0], L6[1:] = ind, Lr
    U6[0, 0] = U6[1, 0] = 1.0
    U6[2:, 1:] = Ur
    out = {k: v for k, v in head.items() if k != "W6"}
    out["L6"], out["U6"] = L6, U6
    return out
