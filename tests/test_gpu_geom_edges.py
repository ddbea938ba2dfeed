"""The geometry unit entries (az_divide_region, az_sift_dup, az_roi_dedup, az_roi_pool) at their own edges, bit for bit
against the oracle: the multi-launch kernels behind them are the form every other search form falls back to.  Capacities
on a 64-region context (child capacity 4 x 64 = 256), degenerate and colliding regions, chunk boundaries of the
feature-space dedup, RoIPool on tiny maps on both sides of the many-roi path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipAZNet
    from oracle import az_oracle as orc
    return ffi, synth, HipAZNet, orc


@pytest.fixture(scope="module")
def ctx64(mods):
    ffi = mods[0]
    return ffi.AzContext(0, max_regions=64)


@pytest.fixture(scope="module")
def big(mods):
    ffi = mods[0]
    return ffi.AzContext(0)


def ref_sift(orc, regions, ms):
    regions = np.asarray(regions, dtype=np.float64).reshape(-1, 4)
    if regions.shape[0] == 0:
        return np.zeros((0, 4))
    a = orc.sift_dup_numpy(regions, ms)                      # np.round(regions / ms).dot(v), np.unique: div.pyx:85-89
    assert np.array_equal(a, orc.sift_dup(regions, ms))      # (the oracle's int64-key restatement agrees)
    return a


def ref_divide(orc, regions, ms):
    regions = np.asarray(regions, dtype=np.float64).reshape(-1, 4)
    return ref_sift(orc, orc.divide_children(regions), ms)


def grid_regions(n, w, h, step=400.0):
    """n regions of w x h px far enough apart that no two children share a hash"""
    return np.array([[step * i, step * (i % 3), step * i + w - 1, step * (i % 3) + h - 1] for i in range(n)])


A5, B8 = (100, 100), (100, 170)            # (w, h): 5 children (aspect < 1.5), 8 children (1.5 <= aspect < 2)


# ---------------------------------------------------------------------------------------------- divide_region / sift_dup
DIVIDE = {
    "none": np.zeros((0, 4)),
    "one": np.array([[0.0, 0.0, 999.0, 599.0]]),
    "1x1_px": np.array([[5.0, 7.0, 5.0, 7.0], [300.0, 300.0, 300.0, 300.0], [5.2, 7.4, 5.2, 7.4]]),
    "thin_wide": np.array([[10.0, 20.0, 49.0, 23.0]]),                                            # a side of 4 px < min_side: 59 children
    "thin_tall": np.array([[50.0, 300.0, 53.0, 339.0]]),
    "square_tie": np.array([[0.0, 0.0, 99.0, 99.0], [200.5, 100.25, 263.5, 163.25]]),             # L0 == L1: argmin takes the width
    "negative": np.array([[-50.5, -30.25, 20.0, 40.0], [-400.0, -300.0, -301.0, -180.0], [-5.0, -5.0, 4.0, 4.0]]),
    "identical": np.tile(np.array([[17.0, 33.0, 140.0, 121.0]]), (10, 1)),
    "overlapping": np.array([[0.0, 0.0, 199.0, 199.0], [50.0, 50.0, 249.0, 249.0], [0.0, 0.0, 199.0, 199.0],
                             [100.0, 0.0, 299.0, 199.0]]),
}


@pytest.mark.parametrize("name", sorted(DIVIDE))
@pytest.mark.parametrize("ms", [10.0, 1.0, 7.5])
def test_divide_region_equals_the_oracle_bit_for_bit(mods, ctx64, name, ms):
    orc = mods[3]
    regions = DIVIDE[name]
    want = ref_divide(orc, regions, ms)
    assert want.shape[0] <= 64 and orc.divide_children(regions).shape[0] <= 256
    got = ctx64.divide_region(regions, ms)
    assert got.shape == want.shape and np.array_equal(got, want), name


def test_hash_digits_that_carry_collide_as_in_the_reference(mods, ctx64):
    """min_side = 1 with coordinates above 999: round(x / 1) no longer fits its three decimal digits of the hash and
    carries into the next field, so different regions share a hash -- x1 = 1000, y1 = 5 and x1 = 0, y1 = 6 both give
    6000 + ... .  The reference keeps the first of them; so must the device."""
    orc = mods[3]
    R = np.array([[1000.0, 5.0, 1040.0, 60.0], [0.0, 6.0, 1040.0, 60.0], [2000.0, 4.0, 1040.0, 60.0],
                  [1000.4, 5.2, 1040.0, 60.0], [999.0, 5.0, 1040.0, 60.0], [1999.0, 1234.0, 2100.0, 1300.0],
                  [999.0, 1235.0, 1100.0, 1301.0]])
    want = ref_sift(orc, R, 1.0)
    assert want.shape[0] < np.unique(np.round(R), axis=0).shape[0]          # the carry really merges distinct regions
    assert np.array_equal(ctx64.sift_dup(R, 1.0), want)
    assert np.array_equal(ctx64.sift_dup(R[::-1].copy(), 1.0), ref_sift(orc, R[::-1].copy(), 1.0))
    big_regions = np.array([[1000.4, 1200.6, 1100.2, 1290.9], [1010.0, 1195.0, 1139.0, 1299.0]])
    assert np.array_equal(ctx64.divide_region(big_regions, 1.0), ref_divide(orc, big_regions, 1.0))


def test_sift_dup_orderings_and_which_duplicate_survives(mods, ctx64):
    """np.unique(return_index): ascending hash (signed), the FIRST occurrence of each -- whatever the input order."""
    orc = mods[3]
    rng = np.random.RandomState(5)
    x1, y1 = rng.uniform(-300, 900, 40), rng.uniform(-200, 500, 40)
    R = np.stack([x1, y1, x1 + rng.uniform(10, 200, 40), y1 + rng.uniform(10, 200, 40)], 1)
    R = ref_sift(orc, R, 10.0)                                        # sorted by hash, one per hash
    assert R.shape[0] >= 30
    dup = R[7] + 0.3                                                  # same hash as R[7], other coordinates
    assert np.array_equal(np.round(dup / 10.0), np.round(R[7] / 10.0))
    for name, inp in (("sorted", R), ("reversed", R[::-1].copy()), ("dup_first", np.vstack([dup[None], R])),
                      ("dup_last", np.vstack([R, dup[None]])), ("shuffled", np.vstack([R, dup[None]])[rng.permutation(len(R) + 1)])):
        want = ref_sift(orc, inp, 10.0)
        got = ctx64.sift_dup(inp, 10.0)
        assert np.array_equal(got, want), name
    assert np.array_equal(ctx64.sift_dup(np.vstack([dup[None], R]), 10.0)[7], dup)            # the first occurrence, not the sorted one
    same = np.tile(R[3][None], (256, 1))                              # all identical, a full child buffer
    assert np.array_equal(ctx64.sift_dup(same, 10.0), R[3][None])
    assert ctx64.sift_dup(np.zeros((0, 4)), 10.0).shape == (0, 4)


def test_region_and_child_capacities_of_a_64_region_context(mods, ctx64):
    ffi, synth, HipAZNet, orc = mods
    probe = grid_regions(4, *A5)

    def still_works():
        assert np.array_equal(ctx64.divide_region(probe, 10.0), ref_divide(orc, probe, 10.0))

    # survivors == max_regions: 8 regions of 5 children + 3 of 8, all distinct
    R64 = np.vstack([grid_regions(8, *A5), grid_regions(3, *B8) + 4000.0])
    want = ref_divide(orc, R64, 10.0)
    assert want.shape[0] == 64
    assert np.array_equal(ctx64.divide_region(R64, 10.0), want)
    # ... and one more: 13 x 5 distinct children
    R65 = grid_regions(13, *A5)
    assert ref_divide(orc, R65, 10.0).shape[0] == 65
    with pytest.raises(ffi.AzError) as e:
        ctx64.divide_region(R65, 10.0)
    assert e.value.code == ffi.AZ_ERR_CAPACITY
    still_works()
    # the same through az_sift_dup: 64 distinct hashes among 256 rows; 65 among 65
    S = np.vstack([grid_regions(64, 50, 50, step=30.0)] * 4)
    assert np.array_equal(ctx64.sift_dup(S, 10.0), ref_sift(orc, S, 10.0)) and ref_sift(orc, S, 10.0).shape[0] == 64
    with pytest.raises(ffi.AzError) as e:
        ctx64.sift_dup(grid_regions(65, 50, 50, step=30.0), 10.0)
    assert e.value.code == ffi.AZ_ERR_CAPACITY
    with pytest.raises(ffi.AzError) as e:
        ctx64.sift_dup(np.vstack([S, S[:1]]), 10.0)                   # 257 rows: more than the child buffer holds
    assert e.value.code == ffi.AZ_ERR_CAPACITY
    still_works()
    # children == the child capacity (4 * max_regions = 256): 48 x 5 + 2 x 8, identical parents so that few survive
    a, b = grid_regions(1, *A5), grid_regions(1, *B8) + 2000.0
    R256 = np.vstack([np.tile(a, (48, 1)), np.tile(b, (2, 1))])
    assert orc.divide_children(R256).shape[0] == 256
    want = ref_divide(orc, R256, 10.0)
    assert want.shape[0] == 13 and np.array_equal(ctx64.divide_region(R256, 10.0), want)
    # ... and one parent more: 261 children
    with pytest.raises(ffi.AzError) as e:
        ctx64.divide_region(np.vstack([R256, a]), 10.0)
    assert e.value.code == ffi.AZ_ERR_CAPACITY
    still_works()
    # P == max_regions: every region has at least five children (num_long >= 2), so 64 parents always outgrow the 256
    # children of this context -- a capacity error, not a wrong answer; 65 parents are refused by count
    for P in (64, 65):
        with pytest.raises(ffi.AzError) as e:
            ctx64.divide_region(np.tile(a, (P, 1)), 10.0)
        assert e.value.code == ffi.AZ_ERR_CAPACITY
        still_works()
    # the largest P that fits: 51 identical parents of five children
    assert np.array_equal(ctx64.divide_region(np.tile(a, (51, 1)), 10.0), ref_divide(orc, a, 10.0))


# ---------------------------------------------------------------------------------------------- roi_dedup
def ref_roi_dedup(orc, boxes, scale, dedup, batch):
    """test.py:202-218: one np.unique per chunk of `batch` boxes; index / inv_index in whole-level numbering"""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    rois = orc.get_rois_blob(boxes, scale)
    index, inv, U = [], np.zeros(boxes.shape[0], dtype=np.int64), 0
    for s in range(0, boxes.shape[0], batch):
        idx, iv = orc.roi_dedup(rois[s:s + batch], dedup)
        index.extend((s + idx).tolist())
        inv[s:s + batch] = U + iv
        U += len(idx)
    return rois, np.asarray(index, dtype=np.int64), inv


def check_roi_dedup(orc, ctx, boxes, scale, dedup, batch):
    rois, index, inv = ctx.roi_dedup(boxes, scale, dedup, batch)
    wr, wi, wv = ref_roi_dedup(orc, boxes, scale, dedup, batch)
    assert np.array_equal(rois, wr)
    assert np.array_equal(index, wi), (len(boxes), batch)
    assert np.array_equal(inv, wv), (len(boxes), batch)
    return len(wi)


def coarse_boxes(rng, P, kinds=None):
    """boxes on a coarse grid with sub-cell jitter: many share a feature-space hash (`kinds`: drawn from that many grid
    boxes only, so that any `kinds` + 1 of them hold a collision)"""
    n = kinds or P
    x1, y1 = 32.0 * rng.randint(0, 6, n), 32.0 * rng.randint(0, 4, n)
    B = np.stack([x1, y1, x1 + 32.0 * rng.randint(1, 3, n), y1 + 32.0 * rng.randint(1, 3, n)], 1)
    if kinds:
        B = B[rng.randint(0, kinds, P)]
    return B + rng.uniform(-3.0, 3.0, B.shape)


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_roi_dedup_at_chunk_boundaries(mods, big, batch):
    orc = mods[3]
    rng = np.random.RandomState(batch)
    for k in (1, 3):
        for P in (k * batch - 1, k * batch, k * batch + 1):
            if P <= 0:
                continue
            B = coarse_boxes(rng, P, kinds=5)
            for scale in (1.0, 1.6):
                U = check_roi_dedup(orc, big, B, scale, 1.0 / 16.0, batch)
                assert U < P or P < 7 or batch == 1               # (six boxes of a chunk hold a collision)


def test_roi_dedup_identity_ties_full_context_and_equal_rows(mods, big, ctx64):
    orc = mods[3]
    rng = np.random.RandomState(9)
    B = coarse_boxes(rng, 50)
    for dedup in (0.0, -1.0):                                     # cfg.DEDUP_BOXES <= 0: no dedup (test.py:211)
        rois, index, inv = big.roi_dedup(B, 1.0, dedup, 10000)
        assert np.array_equal(index, np.arange(50)) and np.array_equal(inv, np.arange(50))
        assert np.array_equal(rois, orc.get_rois_blob(B, 1.0))
    # x * dedup on .5 in f32: np.round is half to even (8 -> 0, 24 -> 2, 40 -> 2, 56 -> 4)
    v = np.array([0.0, 8.0, 16.0, 24.0, 32.0, 40.0, 48.0, 56.0, 72.0, 88.0])
    T = v[rng.randint(0, len(v), (120, 4))]
    assert check_roi_dedup(orc, big, T, 1.0, 1.0 / 16.0, 10000) < 120
    check_roi_dedup(orc, big, T, 1.0, 1.0 / 16.0, 7)
    check_roi_dedup(orc, big, T * 0.5, 2.0, 1.0 / 16.0, 10000)      # the same ties through the scale
    # P == max_regions, in one chunk and in chunks that end exactly there
    B64 = coarse_boxes(rng, 64)
    for batch in (10000, 64, 32, 63):
        check_roi_dedup(orc, ctx64, B64, 1.0, 1.0 / 16.0, batch)
    # all rows equal; nothing at all
    E = np.tile(B[:1], (64, 1))
    assert check_roi_dedup(orc, ctx64, E, 1.0, 1.0 / 16.0, 10000) == 1
    assert check_roi_dedup(orc, ctx64, E, 1.0, 1.0 / 16.0, 7) == 10
    rois, index, inv = ctx64.roi_dedup(np.zeros((0, 4)), 1.0, 1.0 / 16.0, 10000)
    assert rois.shape[0] == 0 and index.shape == (0,) and inv.shape == (0,)


# ---------------------------------------------------------------------------------------------- roi_pool
MAPS = [(1, 1), (1, 9), (7, 7), (13, 5)]


def edge_rois(fh, fw, rng):
    """97 rois (feature cells x 16 px) for an fh x fw map: the listed edges first, random ones behind them"""
    W, H = 16.0 * fw, 16.0 * fh
    r = [
        (-200.0, 0.0, -40.0, H), (W + 40.0, 0.0, W + 300.0, H), (0.0, -300.0, W, -40.0), (0.0, H + 40.0, W, H + 200.0),    # off each side
        (-100.0, -100.0, -20.0, -20.0), (-64.0, -48.0, 31.0, 47.0),                                                       # negative
        (W - 16.0, 0.0, 0.0, H - 16.0), (0.0, H - 16.0, W - 16.0, 0.0), (80.0, 64.0, 16.0, 0.0),                          # reversed
        (-8.0, -8.0, 8.0, 8.0), (-24.0, -40.0, 24.0, 40.0), (-8.0, -24.0, -8.0, -24.0), (8.0, 24.0, 40.0, 56.0),            # .5 ties
        (0.0, 0.0, 0.0, 0.0), (16.0, 0.0, 16.0, H), (0.0, 32.0, W, 32.0), (W - 16.0, H - 16.0, W - 16.0, H - 16.0),         # one cell wide
        (0.0, 0.0, 16.0 * 7, 16.0 * 7), (-16.0, -16.0, 16.0 * 6, 16.0 * 6),                                               # 8 cells: bins of 1
        (0.0, 0.0, 16.0 * 48, 16.0 * 48), (-16.0 * 20, -16.0 * 20, 16.0 * 28, 16.0 * 28),                                 # 49 cells: bins of 7
        (0.0, 0.0, 16.0 * 49, 16.0 * 49), (-16.0 * 20, -16.0 * 30, 16.0 * 29, 16.0 * 19),                                 # 50 cells: just over 7
        (0.0, 0.0, W - 1.0, H - 1.0), (0.0, 0.0, W, H), (-1000.0, -1000.0, 1000.0, 1000.0),
    ]
    r = np.array(r)
    n = 97 - len(r)
    x1, y1 = rng.uniform(-40, W + 20, n), rng.uniform(-40, H + 20, n)
    more = np.stack([x1, y1, x1 + rng.uniform(-20, 1.5 * W, n), y1 + rng.uniform(-20, 1.5 * H, n)], 1)
    rois = np.vstack([r, more])
    return np.hstack([np.zeros((97, 1)), rois]).astype(np.float32)


@pytest.fixture(scope="module")
def pool_net(mods):
    ffi, synth, HipAZNet, orc = mods
    return HipAZNet(synth.make_head(seed=77, **synth.SMALL_DIMS), name="geom_edges_pool")


@pytest.mark.parametrize("fh,fw", MAPS, ids=["%dx%d" % m for m in MAPS])
def test_roi_pool_on_tiny_maps_on_both_sides_of_the_many_roi_path(mods, pool_net, fh, fw):
    """Same rows at R = 96 (workgroup per bin) and R = 97 (wave per bin): both Caffe's ROIPooling as the oracle restates
    it, bit for bit.  The map has negative values, so an empty bin (0) and a maximum differ everywhere."""
    ffi, synth, HipAZNet, orc = mods
    rng = np.random.RandomState(100 * fh + fw)
    fmap = rng.standard_normal((1, synth.SMALL_DIMS["C"], fh, fw)).astype(np.float32)
    pool_net.set_conv(fmap)
    rois = edge_rois(fh, fw, rng)
    want = orc.roi_pool(fmap[0], rois)
    assert (want == 0).any() and (want < 0).any()
    for R in (96, 97, 1):
        got = pool_net.ctx.roi_pool(rois[:R])
        assert got.shape == (R, want.shape[1])
        bad = np.flatnonzero(~np.all(got == want[:R], axis=1))
        assert bad.size == 0, (R, bad[:8], rois[bad[:8]])
    assert pool_net.ctx.roi_pool(rois[:0]).shape[0] == 0
