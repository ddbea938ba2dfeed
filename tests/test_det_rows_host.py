"""CPU: the premises of tests/test_gpu_det_rows.py, on the reference alone -- no GPU (cases: tests/det_rows_ref.py).

  * both layers of both shapes satisfy `can12` (azk_fc_gemm12_fits), and no size of head_sizes_ref.DET_SIZES does -- which is
    why the detection head's many-row path needs a file of its own;
  * the 2048 rois are distinct under the oracle's 1/16 dedup, lie inside the image, and are the float32 projection of the
    boxes that az_detect is given;
  * the integer heads: every layer's max sum |w||x| + |b| on all 2048 rows is below 2^24 at the densities of
    det_rows_ref.DENSITY, the score layer meets the sensitivity condition, its pre-activations are exact multiples of
    2^-k, and fc6's operands are exact in two fp16 terms at the load-time scales and in three bf16 terms;
  * the row counts visit what the GPU file's table says (kernel switch, half strip, masked full strip, m-tile seams);
  * the lists of part C really dedup to u rows, and the batches of part D split into the passes the GPU test expects."""
import functools

import numpy as np
import pytest

import det_rows_ref as D
import head_sizes_ref as H
import train_step_ref as R


@functools.lru_cache(maxsize=None)
def case(name):
    from oracle import az_oracle as orc
    return D.int_case(name, pool=lambda f, r: orc.roi_pool(f[0], r))


def test_both_layers_of_both_shapes_take_the_many_row_gemm_and_no_other_detection_size_does():
    for name, dims in D.SHAPES.items():
        for N, K in D.layers(dims):
            assert D.can12(N, K), (name, N, K)
    for dims in H.DET_SIZES:
        assert not any(D.can12(N, K) for N, K in D.layers(dims)), dims
    # the chains: K-steps per work item
    (n6, K6), (n7, K7) = D.layers(D.FULL)
    assert (H.fc_split(K6), D.fc_chunk(K6, 16) // 32) == (16, 49) and (H.fc_split(K7), D.fc_chunk(K7, 8) // 32) == (8, 16)
    (n6, K6), (n7, K7) = D.layers(D.SHORT)
    assert (n6 // 128) * H.fc_split(K6) == 256 and (H.fc_split(K7), D.fc_chunk(K7, 8) // 32) == (8, 8)
    assert not D.can12(D.SHORT[1] - 128, K6) and not D.can12(4096, 1024)      # (one n-tile fewer, a shorter K: out)
    # the AZ head's int7 at the full size never qualifies
    assert not D.can12(1280, 4096)


def test_rois_are_distinct_under_the_oracles_dedup():
    from oracle import az_oracle as orc
    rois, boxes = D.rois2048(), D.boxes2048()
    assert rois.shape == (D.NROIS, 5) and rois.dtype == np.float32 and np.array_equal(rois, D.rois2048())
    assert rois[:, 1:].min() >= 0 and rois[:, 3].max() < H.IM_W and rois[:, 4].max() < H.IM_H
    assert (rois[:, 3] - rois[:, 1]).min() > 6 and (rois[:, 4] - rois[:, 2]).min() > 6
    index, inv = orc.roi_dedup(rois)
    assert len(index) == D.NROIS and len(np.unique(inv)) == D.NROIS
    assert np.array_equal(orc.get_rois_blob(boxes, 1.0), rois)
    # no key is near a rounding tie: |x / 16 - round(x / 16)| <= 5 / 16
    q = rois[:, 1:].astype(np.float64) / 16.0
    assert np.abs(q - np.rint(q)).max() <= 5.0 / 16.0 + 1e-6


def _is_ternary(w, unit=1.0):
    return set(np.unique(w / np.float32(unit)).tolist()) <= {-1.0, 0.0, 1.0}


def _exact_in_terms(x, scale, kind):
    """x * scale is the exact sum of two fp16 / three bf16 terms, each the rounding of what the previous ones left."""
    from aznet_hip import ffi
    v = np.unique(np.asarray(x, np.float32)).astype(np.float64) * scale
    left = v.copy()
    for _ in range(2 if kind == "fp16" else 3):
        t = left.astype(np.float16).astype(np.float64) if kind == "fp16" else ffi.bf16_round(left.astype(np.float32)).astype(np.float64)
        assert np.isfinite(t).all()
        left = left - t
    return bool(np.all(left == 0))


@pytest.mark.parametrize("name", sorted(D.SHAPES))
def test_integer_head(name):
    from oracle import az_oracle as orc
    c, dims = case(name), D.SHAPES[name]
    fmap, head, k = c["fmap"], c["head"], c["k"]
    assert c["dims"] == dims and np.array_equal(c["rois"], D.rois2048())
    assert fmap.shape == (1, dims[0], H.MAP_H, H.MAP_W) and set(np.unique(fmap).tolist()) <= {0.0, 1.0, 2.0, 3.0}
    assert 0.4 < (fmap == 0).mean() < 0.6
    assert c["pool5"].shape == (D.NROIS, 49 * dims[0])
    assert np.array_equal(c["pool5"][::97], R.roi_pool(fmap, c["rois"][::97])[0])        # (the oracle's RoIPool built the case)
    dens = D.DENSITY[name]
    for w, b in (("W6", "b6"), ("W7", "b7"), ("Wb", "bb")):
        assert _is_ternary(head[w]) and np.array_equal(head[b], np.rint(head[b])) and np.abs(head[b]).max() <= 4
        assert 0.88 * dens < (head[w] != 0).mean() < 1.12 * dens, w
    unit = 2.0 ** -k
    assert _is_ternary(head["Wc"], unit) and (head["Wc"] != 0).sum(axis=1).tolist() == [c["nnz"]["cls"]] * dims[3]
    assert np.array_equal(head["bc"] / np.float32(unit), np.rint(head["bc"] / np.float32(unit)))
    pre = c["pre"]["cls"]
    assert pre.shape == (D.NROIS, dims[3])
    assert np.array_equal(pre / unit, np.rint(pre / unit)) and np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
    top = float(np.abs(pre).max())
    assert top <= 4.0 and (k == 0 or top > 2.0)                                          # (the smallest k)
    assert c["tol"]["cls"] >= 1e-6 and c["unit_move"]["cls"] > 4.0 * c["tol"]["cls"], (c["unit_move"], c["tol"])
    # every partial sum of every layer, in any order, on all 2048 rows: an integer below 2^24
    assert set(c["abs_sum"]) == {"fc6", "fc7", "tail"}
    for layer, v in c["abs_sum"].items():
        assert v < 2.0 ** 24, (layer, v)
    assert np.array_equal(c["bbox"].astype(np.float64), np.rint(c["bbox"])) and c["bbox"].shape == (D.NROIS, 4 * dims[3])
    assert np.allclose(c["p64"]["cls"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # the float64 evaluation of head_sizes_ref on the oracle's RoIPool says the same
    p, b = H.f64_det_head(orc, head, fmap, c["rois"][:64])
    assert np.array_equal(b, c["bbox"][:64]) and np.array_equal(p, c["p64"]["cls"][:64])
    # every window's tolerance has the standing floor; the rows of a window do not all saturate
    for n in D.ROWS_A:
        for back in (False, True):
            assert D.prob_tol(c, D.window(n, back)) >= 1e-6
    # fc6's operands in the 16-bit-term modes (part E runs FULL; the construction is the same for both)
    sx, sw = D.fp16_scale(fmap), D.fp16_scale(head["W6"])
    assert (sx, sw) == (2.0 ** 13, 2.0 ** 14)
    assert _exact_in_terms(c["pool5"], sx, "fp16") and _exact_in_terms(head["W6"], sw, "fp16")
    assert _exact_in_terms(c["pool5"], 1.0, "bf16") and _exact_in_terms(head["W6"], 1.0, "bf16")
    assert not _exact_in_terms(np.float32([1.0]) / np.float32(3.0), 1.0, "fp16")         # (the check can fail: 24 bits)
    print("%s: density %.4g, k = %d, score non-zeros %s, max sum |w||x| %s, unit move %.2e, tolerance %.2e"
          % (name, dens, k, c["nnz"], {n: "%.4g" % v for n, v in c["abs_sum"].items()}, c["unit_move"]["cls"], c["tol"]["cls"]))


def test_row_counts_visit_what_the_table_says():
    rows = D.ROWS_A
    assert [n for n in rows if n < D.GEMM12_MIN] == [1, 16, 17, 160] and D.GEMM12_MIN in rows
    assert rows == tuple(sorted(set(rows))) and rows[-1] == D.NROIS and D.ROWS_B == rows[4:]
    st = {n: D.strips_of(n) for n in D.ROWS_B}
    # the half strip alone in its row group (strips = 6 = 3 x 2 -> the last group has one full strip and the half slot),
    # the full-but-masked last strip (M & 31 in 17..31), an exact multiple of 32
    assert st[161] == (1, 6, True) and st[176] == (1, 6, True) and st[177] == (1, 6, False) and st[191] == (1, 6, False)
    assert st[192] == (1, 6, False) and 192 % 32 == 0 and st[193] == (1, 7, True)
    assert any(17 <= (n & 31) <= 31 for n in D.ROWS_B) and (2047 & 31) == 31
    # the m-tile seams: 12 strips -> 13 (with the half slot), 13 without it; 24 -> 25; six m-tiles
    assert st[384] == (1, 12, False) and st[385] == (2, 13, True) and st[400] == (2, 13, True) and st[401] == (2, 13, False)
    assert st[768] == (2, 24, False) and st[769] == (3, 25, True)
    assert st[1000][0] == 3 and st[2000][0] == 6 and st[2047] == (6, 64, False) and st[2048] == (6, 64, False)
    # part B's reference launches and part E's rows
    assert D.CHUNK_B < D.GEMM12_MIN and max(D.ROWS_E) <= D.CAP_TERMS
    assert [n - 256 for n in D.ROWS_E[:3]] == [-1, 0, 1] and [n - 512 for n in D.ROWS_E[3:6]] == [-1, 0, 1]


@pytest.mark.parametrize("P,u", D.FEW_CASES, ids=lambda v: str(v))
def test_few_unique_lists_dedup_to_u_rows(P, u):
    from oracle import az_oracle as orc
    boxes, distinct, rep = D.few_unique(P, u)
    assert boxes.shape == (P, 4) and distinct.shape == (u, 4) and np.array_equal(boxes, distinct[rep])
    assert sorted(set(rep.tolist())) == list(range(u))
    assert P >= D.GEMM12_MIN and P <= D.NROIS and (u == P or u < D.GEMM12_MIN or (P, u) == (2000, 161))
    index, inv = orc.roi_dedup(orc.get_rois_blob(boxes, 1.0))
    assert len(index) == u
    if u > 1:
        assert not np.array_equal(rep, np.arange(P) % u)                                 # (shuffled)
    # the reference launch (the u distinct boxes alone) dedups to itself
    assert len(orc.roi_dedup(orc.get_rois_blob(distinct, 1.0))[0]) == u


def test_batches_split_into_the_passes_the_gpu_test_expects():
    from oracle import az_oracle as orc
    counts, cap = D.BATCH_CASES["3x150"]
    assert D.passes(counts, cap) == [(0, 1, 2)] and sum(counts) >= D.GEMM12_MIN > max(counts)
    counts, cap = D.BATCH_CASES["2x1000"]
    assert D.passes(counts, cap) == [(0, 1)] and D.strips_of(sum(counts))[0] == 6 and 1000 % 384
    counts, cap = D.BATCH_CASES["split"]
    assert D.passes(counts, cap) == [(0,), (1, 2)] and max(counts) <= cap
    for counts, cap in D.BATCH_CASES.values():
        bl = D.batch_boxes(counts)
        assert [len(b) for b in bl] == list(counts)
        for b in bl:                                                                      # (dedup is per image: all rows stay)
            assert len(orc.roi_dedup(orc.get_rois_blob(b, 1.0))[0]) == len(b)
        maps = D.batch_maps(len(counts))
        assert all(m.shape == (1, D.FULL[0], H.MAP_H, H.MAP_W) for m in maps) and not np.array_equal(maps[0], maps[1])
