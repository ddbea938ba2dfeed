"""Case builders of tests/test_gpu_solver_edges.py and its host twin tests/test_solver_edges_host.py (test infrastructure):
the trainer off its defaults.  Hyper-parameters other than az_solver_create's, rois that RoIPool and its backward gather
have not met (empty bins, degenerate / off-map / oversized rois, unsorted batch indices, bins narrower than a cell) on maps
with ties, the (M, N, K) of the GEMM sweep, and SmoothL1 weights that are not 0 / 1.  Everything is seeded; the references
are tests/train_step_ref.py's."""
import numpy as np

import train_step_ref as R

# ---- 1. hyper-parameters ----------------------------------------------------------------------------------------------------
MASK_CASE = dict(rows=130, seed=276, iteration=0, ratios=(0.3, 0.6, 0.8), row=21, unit=78)     # element 21 * 128 + 78 = 2766
RATIO_SETS = ((0.3, 0.0, 0.6), (0.0, 0.0, 0.0), (0.25, 0.9, 0.5))
HYPER_ROWS = (37, 130)
FRONT_DOOR = dict(ratios=(0.3, 0.0, 0.6), steps=3)


def _f32(v):
    """What the trainer holds of a multiplier or ratio: its float32."""
    return float(np.float32(v))


def hyper_multipliers():
    """(lr_mult, decay_mult) by parameter name: int7_1 frozen (0 / 0), adj_score's weights at 0.1, zoom_score's bias at 3;
    decay on int6's bias, none on int7_2's weights.  As the float32 values the trainer multiplies with."""
    lr = dict(R.LR_MULT, W71=0.0, b71=0.0, Was=_f32(0.1), bz=3.0)
    dc = dict(R.DECAY_MULT, b6=1.0, W72=0.0)
    return lr, dc


def front_door_multipliers():
    return dict(R.LR_MULT, W71=0.0, b71=0.0), dict(R.DECAY_MULT)


def front_door_rows(rows):
    """prototxt.layer_table's rows with dropout 0.3 on int6, no Dropout block on int7_1, 0.6 on int7_2 and int7_1 frozen."""
    out = []
    for name, typ, lw, lb, dw, db, std, drop in rows:
        if name == "int6":
            drop = 0.3
        elif name == "int7_1":
            lw, lb, drop = 0.0, 0.0, None
        elif name == "int7_2":
            drop = 0.6
        out.append((name, typ, lw, lb, dw, db, std, drop))
    return out


def f32_scale(ratio):
    """The kernel's dropout scale: 1.0f / (1.0f - ratio) in float32."""
    return np.float32(1) / (np.float32(1) - np.float32(ratio))


# ---- 2. hostile rois ----------------------------------------------------------------------------------------------------------
MAP = dict(N=3, C=8, H=13, W=17)
MAP_KINDS = ("plateau", "negative", "normal")
ROI_DIMS = (MAP["C"], 128, 64, 32)


def hostile_rois():
    """The 43 rows [b, x1, y1, x2, y2] of the issue on the 208 x 272 px image of a 13 x 17 map."""
    X, Y = 16 * MAP["W"], 16 * MAP["H"]
    rows = [[0, 0, 0, X - 1, Y - 1],                          # the whole map
            [1, 8, 8, 8, 8],                                  # one point
            [2, -40, -24, 60, 50],                            # over the top-left corner
            [0, -300, -300, -200, -200],                      # off the map, top-left
            [1, X + 100, Y + 100, X + 400, Y + 300],          # off the map, bottom-right
            [2, X - 40, Y - 40, X + 200, Y + 300],            # over the bottom-right corner
            [0, 100, 100, 50, 40],                            # x2 < x1, y2 < y1
            [1, -1e6, -1e6, 1e6, 1e6],                        # far larger than the map
            [2, 64, 0, 64, Y - 1],                            # one column wide
            [0, -1e8, 5, 1e8, 9]]                             # the largest coordinate the trainer admits
    for rh in range(1, 15):                                   # bins narrower than a cell: one cell is the arg-max of several
        for off in (0, 3):
            rows.append([(rh + off) % 3, 16 * off, 16 * off, 16 * (off + rh) - 1, 16 * (off + (2 * rh) % 15 + 1) - 1])
    rows += [rows[2]] * 5
    rois = np.array(rows, dtype=np.float32)
    assert rois.shape == (43, 5)
    return rois


def hostile_map(kind, seed=41):
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = (MAP["N"], MAP["C"], MAP["H"], MAP["W"])
    if kind == "plateau":                                      # mostly zeros, few levels: ties everywhere
        return rng.choice(np.array([0, 0, 0, 1, 2, 3], np.float32), size=shape)
    if kind == "negative":                                     # a maximum below the 0 an empty bin gets
        return rng.integers(-4, 0, shape).astype(np.float32)
    assert kind == "normal"
    return rng.standard_normal(shape).astype(np.float32)


def roi_case(kind, reverse=False):
    """(head, fmap, blobs): the 43 rows on one of the three maps, the other blobs from random_blobs; reverse: the same rows
    with their blobs in reversed row order."""
    head = R.filler_head(43, *ROI_DIMS)
    blobs = R.random_blobs(43, 43, MAP["N"], MAP["H"], MAP["W"])
    blobs["rois"] = hostile_rois()
    if reverse:
        blobs = {k: np.ascontiguousarray(v[::-1]) for k, v in blobs.items()}
    return head, hostile_map(kind), blobs


def bin_windows(rois, H, W):
    """(row, image, hs, he, ws, we) of every NON-EMPTY bin window, by Caffe's arithmetic in float32 (as R.roi_pool)."""
    f32 = np.float32
    for r in range(len(rois)):
        rsw, rsh, rew, reh = (R._roundf(f32(rois[r, q]) * f32(0.0625)) for q in (1, 2, 3, 4))
        bh, bw = f32(max(reh - rsh + 1, 1)) / f32(7), f32(max(rew - rsw + 1, 1)) / f32(7)
        for ph in range(7):
            hs = min(max(int(np.floor(f32(ph) * bh)) + rsh, 0), H)
            he = min(max(int(np.ceil(f32(ph + 1) * bh)) + rsh, 0), H)
            for pw in range(7):
                ws = min(max(int(np.floor(f32(pw) * bw)) + rsw, 0), W)
                we = min(max(int(np.ceil(f32(pw + 1) * bw)) + rsw, 0), W)
                if he > hs and we > ws:
                    yield r, int(rois[r, 0]), hs, he, ws, we


def roi_pool_stats(fmap, rois):
    """(fraction of empty bins, number of non-empty (bin, channel) windows, how many of them hold their maximum more than
    once)."""
    N, C, H, W = fmap.shape
    bins = tied = 0
    for r, n, hs, he, ws, we in bin_windows(rois, H, W):
        win = fmap[n, :, hs:he, ws:we].reshape(C, -1)
        tied += int(np.sum((win == win.max(axis=1, keepdims=True)).sum(axis=1) > 1))
        bins += 1
    return 1.0 - bins / (49.0 * len(rois)), bins * C, tied


def roi_pool_backward_loop(dpool, argmax, rois, shape):
    """RoIPool backward with the order written out: rows ascending, then channels, then bins ascending, one float32 add at
    a time -- per (channel, cell) the order the kernel documents."""
    N, C, H, W = shape
    d = np.zeros((N, C, H * W), dtype=dpool.dtype)
    dp, am = dpool.reshape(-1, C, 49), argmax.reshape(-1, C, 49)
    for r in range(rois.shape[0]):
        n = int(rois[r, 0])
        for c in range(C):
            for p in range(49):
                if am[r, c, p] >= 0:
                    d[n, c, am[r, c, p]] = d[n, c, am[r, c, p]] + dp[r, c, p]
    return d.reshape(N, C, H, W)


def window_cover(rois, shape):
    """bool [N, H, W]: the cells inside at least one bin window of a roi of their image."""
    N, C, H, W = shape
    cov = np.zeros((N, H, W), dtype=bool)
    for r, n, hs, he, ws, we in bin_windows(rois, H, W):
        cov[n, hs:he, ws:we] = True
    return cov


# ---- 3. GEMM sweep --------------------------------------------------------------------------------------------------------
GEMM_MN = ((1, 1), (127, 129), (128, 128), (129, 257), (300, 21), (130, 84), (37, 324))
GEMM_K = (1, 31, 32, 33, 512, 513)
GEMM_BIG = (2049, 2049, 5)                                     # 17 x 17 = 289 tiles: past the 256 of pick_split; forms 0, 1
GEMM_RANDOM = (129, 257, 513)


def gemm_operands(form, M, N, K, draw):
    """(a, b, float64 product) of az_solver_gemm_unit's form: 0 a[M,K] b[N,K]^T, 1 a[M,K] b[K,N], 2 a[K,M]^T b[K,N]."""
    if form == 0:
        a, b = draw((M, K)), draw((N, K))
        return a, b, a.astype(np.float64) @ b.T.astype(np.float64)
    if form == 1:
        a, b = draw((M, K)), draw((K, N))
        return a, b, a.astype(np.float64) @ b.astype(np.float64)
    a, b = draw((K, M)), draw((K, N))
    return a, b, a.T.astype(np.float64) @ b.astype(np.float64)


def gemm_abs_sum(form, a, b):
    """max over outputs of sum_k |a||b|: below 2^24 every partial sum of integer operands is exact in float32."""
    a, b = np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))
    return float({0: lambda: a @ b.T, 1: lambda: a @ b, 2: lambda: a.T @ b}[form]().max())


def integer_draw(rng):
    return lambda s: rng.integers(-8, 9, s).astype(np.float32)


# ---- 4. SmoothL1 with weights that are not 0 / 1 -------------------------------------------------------------------------------
LOSS_WEIGHTS = (0.0, 0.5, 1.0, 2.0)
ONE_DOWN, ONE_UP = float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2)))
LOSS_D = (0.0, 0.5, -0.5, 1.0, -1.0, ONE_DOWN, -ONE_DOWN, ONE_UP, -ONE_UP)


def loss_case(rows=37, seed=17):
    """(head, fmap, blobs, x): small_case with Wab = 0, so that adj_bbox == bab == x[j] exactly in every row; weights cycle
    through LOSS_WEIGHTS and the targets are t = x - d / w (float32) with d cycling through LOSS_D, so that the kernel's
    w (x - t) lands on 0, +-0.5, +-1 and the floats next to +-1 (all weights are powers of two: the product is exact
    wherever x - t is)."""
    head, fmap, blobs = R.small_case(R=rows, seed=seed)
    x = ((np.arange(44) % 5 - 2) * 0.25).astype(np.float32)
    head["Wab"] = np.zeros_like(head["Wab"])
    head["bab"] = x.copy()
    e = np.arange(rows * 44).reshape(rows, 44)
    w = np.array(LOSS_WEIGHTS, np.float32)[e % 4]
    d = np.array(LOSS_D, np.float64)[(e // 4) % 9]
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.where(w > 0, x.astype(np.float64)[None, :] - d / np.where(w > 0, w, 1), rng.standard_normal((rows, 44))).astype(np.float32)
    blobs["adj_loss_weights"], blobs["adj_targets"] = w, t
    return head, fmap, blobs, x


def smooth_l1_landing(x, t, w):
    """The float32 w (x - t) of the kernel."""
    return (w * (np.asarray(x, np.float32)[None, :] - t)).astype(np.float32)
