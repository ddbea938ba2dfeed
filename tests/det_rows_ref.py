"""Cases for the detection head on the many-row GEMM across row counts (test infrastructure, plain NumPy; the yardstick of
tests/test_det_rows_host.py and tests/test_gpu_det_rows.py).

The detection head reaches k_fc_splitk12 (az_head12.hip) in ways the AZ head never does: fc7 qualifies as well as fc6 (a
short work-item chain whose A operand is a ReLU output), the kernel is chosen by the number of boxes BEFORE the 1/16 dedup
while the row count is what the device finds after it, and the rows of several images share a launch (launch_det_head in
az_detect.hip, which reads what a pass needs from one DetPass record).  Two shapes, the smallest at which both layers still
satisfy `can12` (azk_fc_gemm12_fits, az_head12.hip):

  FULL   (512, 4096, 4096, 21)   fc6 16 chunks of 1568, fc7 8 chunks of 512: the reference's own shape
  SHORT  (512, 2048, 4096, 81)   fc6 16 n-tiles x 16 chunks = 256 groups, the minimum; fc7 K = 2048: 8 chunks of 256 = 8 K-steps
                                 per work item, the shortest chain the contract allows

on a 24 x 32 map and ONE set of 2048 rois that stay distinct under the 1/16 dedup key.  The integer-exact heads are
head_sizes_ref.int_det_case's on that roi set, the random head is synth.make_det_head's; tolerances are
train_step_ref.bound.  Nothing here restates a layer: the float64 evaluations are head_sizes_ref's."""
import numpy as np

import head_sizes_ref as H
import train_step_ref as R

FULL = (512, 4096, 4096, 21)
SHORT = (512, 2048, 4096, 81)
SHAPES = {"FULL": FULL, "SHORT": SHORT}
NROIS = 2048
CAP_SMALL = 512                 # max_regions of the capacity-split context
CAP_TERMS = 1024                # max_regions of the mode 2 / mode 3 contexts (1000 rows)
GEMM12_MIN = 161                # AzEnv::gemm12_min's default
# the density of W6 / W7 / Wb that keeps every partial sum of every layer below 2^24 on all 2048 rows (asserted by the
# host test; head_sizes_ref's quarter density was enough for both shapes)
DENSITY = {"FULL": 0.25, "SHORT": 0.25}

# n: what it reaches under the detection head (both windows rois[:n] and rois[2048 - n:])
ROWS_A = (1, 16, 17, 160,                 # k_fc_splitk
          161,                            # the switch to k_fc_splitk12
          176, 177, 191, 192, 193,        # half strip, full masked strip, exact multiple of 32
          384, 385, 400, 401,             # one m-tile -> two; with and without the half slot
          768, 769,                       # two -> three
          1000,                           # mid-range
          2000,                           # test_net's proposal count
          2047,                           # M & 31 = 31
          2048)                           # M equal to the context's capacity: every slab filled to capM * N exactly
ROWS_B = tuple(n for n in ROWS_A if n >= GEMM12_MIN)
CHUNK_B = 160                             # the reference launches of part B: k_fc_splitk
# (P boxes, u distinct ones): the launch is chosen by P, the device finds M = u
FEW_P, FEW_U = (161, 300, 2000), (1, 5, 16, 17, 32, 33, 96, 97, 160)
FEW_CASES = tuple((P, u) for P in FEW_P for u in FEW_U) + ((300, 300), (2000, 161))
# proposals per image of the three detect_batch cases, and the context each runs on
BATCH_CASES = {"3x150": ((150, 150, 150), NROIS), "2x1000": ((1000, 1000), NROIS), "split": ((300, 300, 100), CAP_SMALL)}
ROWS_E = (255, 256, 257, 511, 512, 513, 1000)
TERM_MODES = (2, 3)


def fc_chunk(K, S):
    """azk_fc_chunk: a layer's K chunk, a multiple of the K step of 32."""
    return (-(-K // S) + 31) // 32 * 32


def can12(N, K):
    """azk_fc_gemm12_fits (az_head12.hip), the many-row kernel's condition on a layer: whole n-tiles of 128, at least 256
    (n-tile, chunk) groups, whole K steps, whole chunks of at least 64."""
    S = H.fc_split(K)
    return N % 128 == 0 and (N // 128) * S >= 256 and K % 32 == 0 and fc_chunk(K, S) * S == K and fc_chunk(K, S) >= 64


def layers(dims):
    """((N, K) of fc6, (N, K) of fc7)."""
    C, n6, n7, _ = dims
    return (n6, 49 * C), (n7, n6)


def strips_of(M):
    """(m-tiles, strips, has_half) of a k_fc_splitk12 launch of M rows."""
    strips = (M + 31) >> 5
    return (strips + 11) // 12, strips, 0 < (M & 31) <= 16


def rois2048(seed=11):
    """2048 rois [0, x1, y1, x2, y2] on the 384 x 512 image, each in its own cell of the 1/16 dedup key: the corners are
    16 x (distinct integer 4-tuples) plus an offset of less than 5 px, so no rounding of coordinate / 16 is in doubt."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kx, ky = H.IM_W // 16, H.IM_H // 16
    seen, keys = set(), []
    while len(keys) < NROIS:
        x1, y1 = int(rng.integers(0, kx - 1)), int(rng.integers(0, ky - 1))
        x2, y2 = int(rng.integers(x1 + 1, kx)), int(rng.integers(y1 + 1, ky))
        if (x1, y1, x2, y2) not in seen:
            seen.add((x1, y1, x2, y2))
            keys.append((x1, y1, x2, y2))
    k = np.asarray(keys, np.float64)
    off = rng.uniform(-5.0, 5.0, k.shape)
    off[k == 0] = np.abs(off[k == 0])
    return np.concatenate([np.zeros((NROIS, 1)), 16.0 * k + off], 1).astype(np.float32)


def boxes2048():
    """The same rois as float64 image boxes at scale 1 (az_detect projects them back to the float32 rois)."""
    return rois2048()[:, 1:].astype(np.float64)


def int_case(name, pool=None):
    """The integer-exact head of a shape on the 2048 rois (head_sizes_ref.int_det_case at DENSITY)."""
    return H.int_det_case(SHAPES[name], pool=pool, rois=rois2048(), density=DENSITY[name])


def random_case(orc):
    """The random FULL head on a random map with its float64 and float32-CPU evaluations of all 2048 rois."""
    from aznet_hip import synth
    C, n6, n7, ncls = FULL
    c = {"dims": FULL, "head": synth.make_det_head(seed=911, C=C, n6=n6, n7=n7, ncls=ncls),
         "fmap": synth.make_feature_map(77, C, H.MAP_H, H.MAP_W), "rois": rois2048()}
    c["r64"] = H.f64_det_head(orc, c["head"], c["fmap"], c["rois"])
    c["r32"] = orc.det_head_forward(c["head"], c["fmap"][0], c["rois"])
    return c


def batch_maps(n):
    """The maps of a detect_batch case: image i's own random map."""
    from aznet_hip import synth
    return [synth.make_feature_map(80 + i, FULL[0], H.MAP_H, H.MAP_W) for i in range(n)]


def batch_boxes(counts):
    """Image i's proposals: consecutive slices of the 2048 distinct boxes."""
    b, off = boxes2048(), np.concatenate([[0], np.cumsum(counts)])
    return [b[off[i]:off[i + 1]] for i in range(len(counts))]


def passes(counts, cap):
    """az_detect_batch's passes: the following images while their boxes fit the region capacity."""
    out, i = [], 0
    while i < len(counts):
        j, P = i, 0
        while j < len(counts) and P + counts[j] <= cap:
            P += counts[j]
            j += 1
        assert j > i
        out.append(tuple(range(i, j)))
        i = j
    return out


def few_unique(P, u):
    """(boxes [P, 4], distinct [u, 4], rep [P]): boxes = distinct[rep], every distinct box present, shuffled order."""
    rng = np.random.Generator(np.random.PCG64(1000 * P + u))
    start = int(rng.integers(0, NROIS - u + 1))
    distinct = boxes2048()[start:start + u]
    rep = rng.permutation(np.arange(P) % u)
    return distinct[rep], distinct, rep


def window(n, back):
    return slice(NROIS - n, NROIS) if back else slice(0, n)


def prob_tol(c, rows):
    """The tolerance of cls_prob on a window of an integer case: train_step_ref.bound of the float32 softmax restatement's
    error against float64 on those rows."""
    pre = c["pre"]["cls"][rows]
    return R.bound(R.rel_err(H.softmax32(pre.astype(np.float32)), c["p64"]["cls"][rows]))


def tiny_az_head():
    """An AZ head of the detection head's C (az_set_feature_map needs one); loading it in a 16-bit-term mode sends the
    detection fc6 down that path."""
    return R.filler_head(3, FULL[0], 4, 4, 4)


def fp16_scale(x):
    """The load-time power of two of the two-fp16-term mode: max |x| into [2^14, 2^15)."""
    mx = float(np.abs(x).max())
    return 1.0 if not (0.0 < mx < np.inf) else float(np.ldexp(1.0, 15 - int(np.frexp(np.float32(mx))[1])))
