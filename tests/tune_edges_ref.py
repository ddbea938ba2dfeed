"""NumPy restatements and case builders for the zoom-threshold tuner's edges (tests/test_tune_edges_host.py,
tests/test_gpu_tune_edges.py; DESIGN.md, "Tuner edges").

The path (az-net_amd/csrc): the tuner-variant search (params.reserved bit 2) records every anchor with its zoom score
(k_record_anchors: capHis = 2 * max_regions rows), appends the scores to an HBM pool (k_pool_append, k_pool_advance) and
az_tune_kth_largest / az_tune_top radix-select over order-preserving 32-bit keys of the pooled floats: four byte passes
from the top byte down (pool_kth_key over k_pool_hist, grids capped at GRID_BLOCKS x GRID_THREADS threads), then
k_pool_keep (key >= the k-th key).  Restated here: the keys, the select pass by pass, the keep, the multi-rank merge of
detect.tune.tune_thresh(gather=), three WRONG variants of them (the host test shows each one disagrees with np.sort
somewhere in the table), the pool cases, and the populations of a planted tree under the TUNER's loop.
"""
import numpy as np

from oracle import az_oracle as orc
import search_limits_ref as R

GRID_BLOCKS, GRID_THREADS = 2048, 256
GRID = GRID_BLOCKS * GRID_THREADS                       # 524 288: one turn of the grid-stride loops
TOP_SLACK = 65536                                       # ffi.tune_top's first cap is k + TOP_SLACK
HIS_FACTOR = 2                                          # capHis = HIS_FACTOR * max_regions
MIN_REGIONS = 64                                        # az_set_limits' minimum
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------------------------------
# keys
def fkey(a):
    """Order-preserving key of f32 bits (az_eval.hip: fkey): negative -> all bits flipped, otherwise the sign bit set."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(k):
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return u.view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def has_nan(a):
    return bool(np.isnan(np.asarray(a, dtype=np.float32)).any())


# ---------------------------------------------------------------------------------------------------------------------
# the plain references: np.sort on the values, a stable sort on the bit key
def sorted_desc_by_key(a):
    """The scores, largest first, -0.0 below +0.0 (a stable sort on the key)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a[np.argsort(fkey(a), kind="stable")][::-1]


def ref_kth(a, k):
    """k-th largest as an f32 scalar (bits by the key order); -inf when the set holds <= k scores (the reference's heap
    never overflowed: tune.py:343-350)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= k:
        return np.float32(NEG_INF)
    return sorted_desc_by_key(a)[k - 1]


def ref_kth_by_value(a, k):
    """np.sort alone (values: -0.0 == +0.0)."""
    a = np.asarray(a, dtype=np.float32)
    return np.float32(NEG_INF) if a.size <= k else np.sort(a)[::-1][k - 1]


def ref_top(a, k):
    """Every score >= the k-th largest in key order, sorted (a multiset); everything when the set holds <= k."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= k:
        return sorted_desc_by_key(a)
    s = sorted_desc_by_key(a)
    kk = fkey(s)
    return s[kk >= kk[k - 1]]


# ---------------------------------------------------------------------------------------------------------------------
# the device's select, pass by pass (az_units.hip: pool_kth_key over k_pool_hist)
def radix_kth_key(a, k, skip_shift=None):
    """skip_shift: a WRONG variant that leaves one byte pass out (that byte of the answer stays 0)."""
    keys = fkey(a)
    prefix, want = 0, int(k)
    for shift in (24, 16, 8, 0):
        if shift == skip_shift:
            continue
        hi_mask = 0 if shift == 24 else (0xffffffff << (shift + 8)) & 0xffffffff
        sel = (keys & np.uint32(hi_mask)) == np.uint32(prefix & hi_mask)
        h = np.bincount(((keys[sel] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        b = 255
        while b > 0:
            if h[b] >= want:
                break
            want -= int(h[b])
            b -= 1
        prefix |= b << shift
    return np.uint32(prefix)


def dev_kth(a, k, skip_shift=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= k:
        return np.float32(NEG_INF)
    return key_to_float(radix_kth_key(a, k, skip_shift))[()]


def dev_top(a, k, strict=False):
    """az_tune_top: key 0 keeps everything when the pool holds <= k.  strict: the WRONG keep (`>` for `>=`)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    key = radix_kth_key(a, k) if a.size > k else np.uint32(0)
    kk = fkey(a)
    out = a[(kk > key) if strict else (kk >= key)]
    return sorted_desc_by_key(out)


def signed_bits_kth(a, k):
    """The WRONG order: raw bits compared as signed integers (right for positives, reversed among negatives)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= k:
        return np.float32(NEG_INF)
    return a[np.argsort(a.view(np.int32), kind="stable")][::-1][k - 1]


def merged_thresh(shards, k):
    """tune_thresh(gather=): every rank's tune_top(k), pushed into one pool in rank order, then the k-th largest."""
    tops = [dev_top(s, k) for s in shards]
    return dev_kth(np.concatenate(tops) if tops else np.zeros(0, np.float32), k)


def heap_thresh(lists, k):
    """The reference's heap over the lists (orc.tune_thresh), as a float."""
    return float(orc.tune_thresh([np.asarray(x, dtype=np.float32) for x in lists], k))


# ---------------------------------------------------------------------------------------------------------------------
# case builders
def byte_set(byte, negative=False):
    """256 distinct f32 values whose keys agree outside byte `byte` (0 = lowest).  Byte 3 holds the sign and seven
    exponent bits: with the low 23 bits all ones and bit 23 clear no key of the set is a NaN's (key 0x007fffff is -inf,
    key 0xff7fffff is FLT_MAX)."""
    if byte == 3:
        base = 0x007fffff
    else:
        base = int(fkey(np.array([-0.8125 if negative else 0.4375], dtype=np.float32))[0]) | 0x00001234
    shift = 8 * byte
    base &= ~(0xff << shift) & 0xffffffff
    keys = np.array([base | (v << shift) for v in range(256)], dtype=np.uint32)
    return key_to_float(keys)


def byte_case(byte, negative=False, seed=0):
    """(scores, ks): the byte set shuffled among `above` larger and some smaller scores of other top-byte buckets, and the
    k at the first, a middle and the last score of the set's bucket, plus one on each side of it."""
    rng = np.random.RandomState(100 + seed + 10 * byte + (5 if negative else 0))
    s = byte_set(byte, negative)
    if byte == 3:
        a = np.concatenate([s, s[:1]])                     # (a second -inf: k = 256 is then the set's last score, n = 257)
        above = 0
    else:
        hi = np.float32(3.0) + rng.uniform(0, 1, 37).astype(np.float32)
        lo = np.float32(-7.0) - rng.uniform(0, 1, 41).astype(np.float32)
        a = np.concatenate([s, hi, lo])
        above = hi.size
    rng.shuffle(a)
    ks = [above + 1, above + 2, above + 128, above + 255, above + 256] + ([above + 257, above] if above else [])
    return a, [k for k in ks if k >= 1]


def random_bits(n, seed):
    """n f32 values of random bit patterns: every magnitude and both signs, denormals included, NaNs replaced."""
    rng = np.random.RandomState(seed)
    u = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    nan = ((u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)) & ((u & np.uint32(0x007fffff)) != 0)
    u[nan] &= np.uint32(0xff7fffff)                        # clear the exponent's lowest bit: finite
    return u.view(np.float32).copy()


def size_case(n, seed=0):
    """n scores in [0, 1) with heavy ties and a few negatives; ks = 1, 2, n - 1."""
    rng = np.random.RandomState(1000 + seed)
    a = rng.uniform(0, 1, n).astype(np.float32)
    if n > 8:
        a[::7] = a[3]
        a[5] = -0.25
        a[6] = 0.0
    return a, sorted({k for k in (1, 2, n - 1) if k >= 1})


GRID_SIZES = (1, 255, 256, 257, GRID - 1, GRID, GRID + 1, 2 * GRID + 1)


def value_cases():
    """name -> (scores, ks): the key-byte sets, signs, zeros, denormals, infinities, all equal."""
    out = {}
    for b in (3, 2, 1, 0):
        out["byte%d" % b] = byte_case(b)
        if b != 3:
            out["byte%d_neg" % b] = byte_case(b, negative=True)
    a = random_bits(4099, 5)
    out["mixed_signs"] = (a, [1, 2, 1000, 2050, 4097, 4098])
    tiny = np.float32(1e-45)
    z = np.array([0.0, -0.0, 0.0, -0.0, -0.0, 1.0, -1.0, tiny, -tiny], dtype=np.float32)
    out["zeros"] = (z, [1, 2, 3, 4, 5, 6, 7, 8])            # k = 3, 4: +0.0; k = 5, 6, 7: -0.0 (adjacent keys)
    d = np.concatenate([np.arange(1, 300, dtype=np.uint32).view(np.float32),
                        (np.arange(1, 300, dtype=np.uint32) | np.uint32(0x80000000)).view(np.float32),
                        np.array([0.0, -0.0, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny], dtype=np.float32)])
    np.random.RandomState(6).shuffle(d)
    out["denormals"] = (d, [1, 2, 299, 300, 301, 302, 303, 304, 600, d.size - 1])
    inf = np.array([np.inf, -np.inf, 1.0, np.inf, -np.inf, -1.0, 0.5, np.finfo(np.float32).max,
                    -np.finfo(np.float32).max], dtype=np.float32)
    out["infinities"] = (inf, [1, 2, 3, 4, 7, 8])
    out["all_equal"] = (np.full(777, 0.3125, dtype=np.float32), [1, 2, 400, 776])
    return out


def tie_cases():
    """name -> (scores, k, run): a run of `run` equal scores with the cut at its first, a middle and its last score;
    ref_top then holds more than k entries unless the cut is the run's last."""
    rng = np.random.RandomState(21)
    above = (0.75 + 0.25 * rng.uniform(0, 1, 50)).astype(np.float32)
    below = (0.25 * rng.uniform(0, 1, 90)).astype(np.float32)
    run = 33
    a = np.concatenate([above, np.full(run, 0.5, dtype=np.float32), below])
    rng.shuffle(a)
    return {"first": (a, above.size + 1, run), "middle": (a, above.size + 17, run), "last": (a, above.size + run, run)}


def grow_case():
    """tune_top(k) whose answer outgrows ffi.tune_top's first cap (k + TOP_SLACK): every score ties with the k-th."""
    k = 10
    return np.full(k + TOP_SLACK + 100, 0.625, dtype=np.float32), k


def nk_cases():
    """(lists, k) with k - 1, k and k + 1 finite scores: -inf, -inf, the minimum -- the heap's answers."""
    rng = np.random.RandomState(31)
    k = 12
    out = []
    for n in (k - 1, k, k + 1):
        a = rng.uniform(-1, 1, n).astype(np.float32)
        out.append(([a[:n // 2], a[n // 2:]], k))
    return out


def shard_cases():
    """(scores, k, list of splits): one fixed score set split into 1, 2, 3 and 8 shards in order -- an empty shard, shards
    with fewer and with more than k scores, and the tie at the cut spread over shards."""
    rng = np.random.RandomState(41)
    a = rng.uniform(0, 1, 500).astype(np.float32)
    k = 60
    cut = np.sort(a)[::-1][k - 1]
    a[[3, 130, 260, 390, 499]] = cut                       # the k-th value now ties across the set (and across shards)
    splits = [[0, 500], [0, 130, 500], [0, 20, 20, 500], [0, 5, 5, 70, 131, 200, 261, 391, 500]]
    return a, k, [[a[s[i]:s[i + 1]] for i in range(len(s) - 1)] for s in splits]


# ---------------------------------------------------------------------------------------------------------------------
# planted trees under the tuner's loop (tune.py:256-316: K levels, level 0 against 0, root not forced)
def tuner_populations(H, W, scale, mask, Tz=R.TZ, min_side=10):
    """Per level: P regions, PZ regions that divide, CH children before _sift_dup; `his` = the history's rows."""
    B = np.array([[0, 0, W - 1.0, H - 1.0]])
    K = orc.num_levels(H, W, min_side)
    P, PZ, CH = [0] * K, [0] * K, [0] * K
    for l in range(K):
        z = R.zoom_predicate(B, scale, mask)
        if l == 0:
            z[:] = True                                    # a sigmoid output is >= 0
        elif Tz <= 0:
            z[:] = True
        P[l], PZ[l] = B.shape[0], int(z.sum())
        if PZ[l] == 0 or l + 1 == K:                       # (the last level is recorded and never divided)
            break
        ch = orc.divide_children(B[z])
        CH[l] = ch.shape[0]
        if ch.shape[0] == 0:
            break
        B = orc.sift_dup(ch, float(min_side))
        if B.shape[0] == 0:
            break
    return dict(P=P, PZ=PZ, CH=CH, his=int(sum(P)), K=K)


def cap_cases():
    """The frozen capHis pair (tests/tune_edges_cases.py)."""
    import tune_edges_cases
    return tune_edges_cases.CASES


def mask_of_case(c):
    return R.mask_of(c["runs"], *R.map_size(c["H"], c["W"], c["scale"]))


# ---------------------------------------------------------------------------------------------------------------------
# shapes of the tuner-variant search
LEVEL_SHAPES = [(16, 16), (30, 37), (640, 640)]         # one level (side 10..19), two (20..39), seven: the deepest that
TOO_DEEP = (1280, 1280)                                 # fits 16384 regions -- eight levels end in 19073 regions
THRESH_SHAPE = (120, 200)                               # four levels: the plain search has a level below anchor j's
DEFAULT_REGIONS = 16384


def shape_scale(H, W):
    return R.default_scale(H, W)


def full_tree(H, W):
    """Level sizes of the tuner's loop at Tz = 0 (every region divides): a function of the shape."""
    fh, fw = R.map_size(H, W, shape_scale(H, W))
    return tuner_populations(H, W, shape_scale(H, W), np.zeros((fh, fw), dtype=bool), Tz=0.0)


def level_sizes(Bhis, Tz=0.0, min_side=10):
    """The level sizes of a level-major history [B | zoom], re-walked: level l + 1 is divide_region of level l's rows at
    or above the threshold (0 for the first level), compared in float64."""
    sizes, off, n, l = [], 0, 1, 0
    while n > 0 and off < Bhis.shape[0]:
        rows = Bhis[off:off + n]
        sizes.append(rows.shape[0])
        Z = rows[rows[:, 4].astype(np.float64) >= (0.0 if l == 0 else np.float64(Tz)), :4]
        off += n
        n = orc.divide_region(Z, min_side).shape[0] if Z.shape[0] else 0
        l += 1
    assert off == Bhis.shape[0], (off, Bhis.shape[0], sizes)
    return sizes


def pick_anchor(zoom, sizes):
    """(row, f32 score) of the anchor of level 1 with the largest zoom score, which must be unique: at Tz = that score
    it is the only region of its level that divides."""
    z = np.asarray(zoom, dtype=np.float32)[1:1 + sizes[1]]
    j = int(np.argmax(z))
    assert (z == z[j]).sum() == 1 and len(sizes) > 2
    return 1 + j, z[j]


def thresholds_at(zj):
    """(float(z_j), the next double above it): float32 holds the first and not the second."""
    at = float(np.float32(zj))
    return at, float(np.nextafter(at, 1.0))
