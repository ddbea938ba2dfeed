"""CPU: the premises of tests/test_gpu_lowrank_sizes.py (cases: tests/lowrank_ref.py).  Apart from az_lowrank_split, which
is host arithmetic of the library, these check the fixtures and the tile arithmetic the GPU test relies on: which launches
give k_lowrank_gemm's workgroups a second item, which never did, what the split counts are, and that the planted heads
of every size are exact."""
import functools

import numpy as np
import pytest

import det_rows_ref as DR
import head_sizes_ref as H
import lowrank_ref as LR

PLANTED = tuple((name,) + case for name in ("WIDE", "DEEP", "TINY", "LONG", "DIMS") for case in LR.SIZES[name][2])


@functools.lru_cache(maxsize=None)
def planted(name, ncls, r6, r7):
    from oracle import az_oracle as orc
    return LR.sized_planted(name, ncls, r6, r7, pool=lambda f, r: orc.roi_pool(f[0], r))


# ---- the launcher's tile arithmetic -----------------------------------------------------------------------------------------
def test_the_new_launches_give_workgroups_a_second_item():
    """nt * mt > grid and no whole number of turns: WIDE's fc6_U at 2048 rows on a context of 2304 regions, and every unit
    shape (the unit entry sizes its launch for M + 64 rows)."""
    (C, n6, n7), cap, _ = LR.SIZES["WIDE"]
    nt, mt, grid = LR.tiles(2048, n6, cap)
    assert (nt, mt, grid) == (34, 32, 1024) and n6 - 64 * (nt - 1) == 4, "34 n-tiles, the last 4 columns wide"
    assert nt * mt == 1088 and nt * mt > grid and nt * mt % grid != 0
    # the second items are m-tiles 30 and 31: rows 1920 .. 2047
    second = sorted(set(item // nt for item in range(grid, nt * mt)))
    assert second == [30, 31] and LR.SECOND_TURN == slice(64 * 30, 64 * 32)
    # the row counts of the GPU test on either side of the first second item (item 1024 = m-tile 30: M > 1920)
    turns = {n: LR.tiles(n, n6, cap)[0] * LR.tiles(n, n6, cap)[1] > grid for n in LR.WIDE_ROWS}
    assert turns == {1: False, 64: False, 65: False, 300: False, 1024: False, 1025: False, 1984: True, 2047: True, 2048: True}
    assert LR.tiles(2048, n7, cap)[2] == 36, "fc7 of WIDE: one n-tile"
    for M, N, K in LR.UNIT_BIG:
        nt, mt, grid = LR.tiles(M, N, M + LR.UNIT_GUARD)
        assert M + LR.UNIT_GUARD <= LR.UNIT_BIG_CAP and grid == LR.LR_GRID
        assert nt * mt > grid and nt * mt % grid != 0, (M, N, K)
    (M0, N, K), rows = LR.UNIT_BIG_MASKED
    for M in rows:
        nt, mt, grid = LR.tiles(M, N, M + LR.UNIT_GUARD)
        assert nt * mt > grid and nt * mt % grid != 0 and M % 64 == 1 and M <= M0
        assert (mt - 1) * nt + nt - 1 >= grid, "the masked last m-tile holds second items"
    # the batches and the duplicate lists of the WIDE random head
    assert all(sum(b) in (2000, 2048) for b in LR.BATCHES)
    for b in LR.BATCHES:
        nt, mt, grid = LR.tiles(sum(b), n6, cap)
        assert nt * mt > grid, "the rows of the images together reach the second turn"
        for n in b:
            nt, mt, grid = LR.tiles(n, n6, cap)
            assert nt * mt <= grid, "an image alone does not"
    nt, mt, grid = LR.tiles(LR.CHUNK, n6, cap)
    assert nt * mt == 102 and nt * mt <= grid, "the 160-row reference launches stay on the first turn"


def test_no_earlier_case_reached_the_second_item():
    """What the tests before this file did not reach: every launch of tests/test_gpu_lowrank.py has at most as many tiles
    as workgroups (72 at most at head level)."""
    most = 0
    for N in LR.UNIT_N:
        for M in LR.UNIT_M + (LR.UNIT_CAP,):
            nt, mt, grid = LR.tiles(M, N, M + LR.UNIT_GUARD)
            assert nt * mt <= grid
    for N in LR.DIMS[1:]:
        for M in (1, 300, 512):
            nt, mt, grid = LR.tiles(M, N, 512)
            assert nt * mt <= grid
            most = max(most, grid)
    assert most == 72
    # ... and the other sizes of this file stay below it as well: only WIDE's fc6_U turns twice
    for name in ("DEEP", "TINY", "LONG", "DIMS"):
        (C, n6, n7), cap, _ = LR.SIZES[name]
        for N in (n6, n7):
            nt, mt, grid = LR.tiles(cap, N, cap)
            assert nt * mt <= grid


# ---- the split counts ---------------------------------------------------------------------------------------------------------
def test_split_counts_of_the_new_cases():
    from aznet_hip import ffi
    pairs = set()
    for name, (dims, cap, cases) in LR.SIZES.items():
        for ncls, r6, r7 in cases:
            pairs.update(LR.layer_shapes(name, r6, r7)[0])
    pairs.update((49 * LR.SIZES[name][0][0], r) for name, r6, r7 in LR.RANDOM_SIZES for r in (r6,))
    pairs.update((LR.SIZES[name][0][1], r7) for name, r6, r7 in LR.RANDOM_SIZES)
    pairs.add((49 * LR.SIZES["WIDE"][0][0], LR.RANDOM_WIDE[0]))
    assert {(7840, 36), (7840, 132), (7840, 260), (2116, 4), (196, 8), (8, 8), (260, 256), (2156, 260)} <= pairs
    for K, r in sorted(pairs):
        S = ffi.lowrank_split(K, r)
        assert S == LR.split_ref(K, r) and S == ffi.lowrank_split(K, r) and 1 <= S <= 512, (K, r, S)
        Kc = LR.fc_chunk(K, S)
        assert (S - 1) * Kc < K <= S * Kc, (K, r, S, Kc)
        assert S == 1 or Kc >= 64, (K, r, S, Kc)
        assert S * -(-r // 128) <= 512
    # DEEP's fc6: the full size's 61-odd chunks, 128 long, the last one 32, at one, two and three n-tiles of the L stage
    for r in (36, 132, 260):
        S = ffi.lowrank_split(7840, r)
        assert S == 62 >= 61 and LR.fc_chunk(7840, S) == 128 and 7840 - 61 * 128 == 32
    assert ffi.lowrank_split(2116, 4) == 17 and ffi.lowrank_split(260, 132) == 3 and ffi.lowrank_split(8, 8) == 1
    assert ffi.lowrank_split(196, 36) == 2 and ffi.lowrank_split(2156, 260) == 17


def test_the_n_tile_term_of_the_split_shows_at_long_only():
    """512 // nt enters the count only where ceil(K / (512 // nt)) exceeds 128: K > 32768 at two n-tiles, K > 21760 at
    three.  LONG's fc6 (C = 672: K = 32928) is the shallowest that shows it between ranks 128 and 132; at every other K of
    the table the two ranks give the same count."""
    from aznet_hip import ffi
    table = sorted(set(K for name in LR.SIZES for K in (49 * LR.SIZES[name][0][0], LR.SIZES[name][0][1])))
    assert table == [8, 132, 196, 260, 2116, 2156, 7840, 32928]
    for K in table[:-1]:
        assert ffi.lowrank_split(K, 128) == ffi.lowrank_split(K, 132) == LR.split_ref(K, 132)
    K = table[-1]
    assert K == 49 * 672 and 49 * 668 <= 32768 < K
    assert (ffi.lowrank_split(K, 128), ffi.lowrank_split(K, 132)) == (258, 206) == (LR.split_ref(K, 128), LR.split_ref(K, 132))
    assert (LR.fc_chunk(K, 258), LR.fc_chunk(K, 206)) == (128, 160)
    assert set(LR.SIZES["LONG"][2]) == {(21, 132, 0), (21, 128, 0)}
    # ... and at the paper's fc6
    assert (ffi.lowrank_split(25088, 1024), ffi.lowrank_split(25088, 1028)) == (61, 56) == (LR.split_ref(25088, 1024), LR.split_ref(25088, 1028))


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------
def test_the_sizes_are_what_the_table_says():
    for name, (dims, cap, cases) in LR.SIZES.items():
        C, n6, n7 = dims
        rois = LR.size_rois(name)
        assert rois.shape[0] == {"WIDE": 2048, "TINY": 64, "LONG": 64}.get(name, 812) and rois.shape[0] - (300 if cap == 512 else 0) <= cap
        for ncls, r6, r7 in cases:
            assert r6 % 4 == 0 and r7 % 4 == 0 and r6 <= min(n6, 49 * C) and r7 <= min(n7, n6) and (r6 or r7)
    assert LR.SIZES["DIMS"][0] == LR.DIMS and LR.SIZES["DEEP"][0][1:] == LR.DIMS[1:]
    assert (260, 256) == LR.SIZES["DEEP"][2][2][1:] and min(260, 49 * 160) == 260, "r6 at the rank bound min(out, in)"
    assert (8, 0) == LR.SIZES["TINY"][2][1][1:] and LR.SIZES["TINY"][0][1] == 8, "a rank equal to n6"
    # ranks above 128: two and three n-tiles in the L stage, columns past 128 in dlr_t
    assert sorted(set(-(-r // 128) for name in ("DEEP", "DIMS") for c in LR.SIZES[name][2] for r in c[1:] if r)) == [1, 2, 3]
    r = DR.rois2048()
    assert np.array_equal(LR.size_rois("DEEP")[300:], r[:512]) and np.array_equal(LR.size_rois("DEEP")[:300], H.rois300())
    # defaults unchanged: the earlier callers get the same bits
    a, b = LR.planted_head(21, 4, 0), LR.planted_head(21, 4, 0, dims=LR.DIMS, rois=H.rois300())
    assert all(np.array_equal(a["head"][k], b["head"][k]) for k in a["head"]) and np.array_equal(a["bbox"], b["bbox"])


@pytest.mark.parametrize("case", PLANTED, ids=lambda c: "%s_ncls%d_r6_%d_r7_%d" % c)
def test_planted_heads_of_every_size_are_exact(case):
    c = planted(*case)
    name, ncls, r6, r7 = case
    assert c["abs_sum"] < LR.EXACT
    assert ("L6" in c["head"]) == bool(r6) and ("L7" in c["head"]) == bool(r7)
    for i, r in ((6, r6), (7, r7)):
        W = c["full"]["W%d" % i]
        assert np.array_equal(W, np.rint(W))
        if r:
            assert c["head"]["U%d" % i].shape[1] == r and (np.count_nonzero(c["head"]["U%d" % i], axis=1) == min(r, 8)).all()
    p_lr, b_lr = LR.head_on_pool5(c["head"], c["pool5"], np.float64)
    p_fu, b_fu = LR.head_on_pool5(c["full"], c["pool5"], np.float64)
    assert np.array_equal(b_lr, b_fu) and np.array_equal(b_lr.astype(np.float32), c["bbox"])
    assert np.array_equal(p_lr, p_fu) and np.abs(p_lr - c["p64"]).max() < 1e-12
    assert (c["bbox"] != 0).mean() > 0.5
    if name == "WIDE":
        w = c["bbox"][LR.SECOND_TURN]
        assert len(np.unique(w, axis=0)) > 64 and not (w == c["bbox"][0]).all(axis=1).any()


def test_unit_cases_have_both_signs_and_distinct_rows():
    for M, N, K in LR.UNIT_BIG:
        X, W, b, Y = LR.unit_case(M, N, K)
        assert (Y < 0).any() and (Y > 0).any() and len(np.unique(Y[1920:], axis=0)) > 64
        assert np.array_equal(Y, np.rint(Y)) and np.abs(Y).max() < LR.EXACT


def test_few_unique_and_batches_fit_the_wide_context():
    cap = LR.SIZES["WIDE"][1]
    for P, u in LR.FEW:
        boxes, distinct, rep = DR.few_unique(P, u)
        assert boxes.shape == (P, 4) and P <= cap and distinct.shape == (u, 4) and np.array_equal(boxes, distinct[rep])
        assert len(set(rep.tolist())) == u
    for counts in LR.BATCHES:
        assert DR.passes(counts, cap) == [tuple(range(len(counts)))], "one pass: the images share the launch"
