"""CPU: the conditions on the cases of tests/head_sizes_ref.py that tests/test_gpu_head_sizes.py relies on -- on the reference
alone, no GPU.

  * integer-exact heads: the operands are what the construction says (integers 0..3 with about half zeros, ternary weights at
    density about 0.25, integer biases, score layers ternary x 2^-k), every layer's max sum |w||x| + |b| is below 2^24 (so no
    partial sum in any order leaves fp32's integers), max |pre-sigmoid| and |pre-softmax| <= 4 with the smallest such k, every
    pre-activation an exact multiple of 2^-k that float32 holds exactly, and one unit 2^-k at the largest |pre-activation|
    moves the float64 probability by more than 4 x the tolerance of the probability check;
  * the float64 evaluations of the helper agree with the training restatement's forward (an independent statement of the same
    layers);
  * the sizes exercise what the GPU test's table says (chunk counts, ragged K steps, partial n-tiles, work-item counts)."""
import numpy as np
import pytest

import head_sizes_ref as H
import train_step_ref as R

BN, BK, GRID = 128, 32, 512        # the GEMM's n-tile, K step and grid (include/aznet_hip.h)


def _is_ternary(w, unit=1.0):
    return set(np.unique(w / np.float32(unit)).tolist()) <= {-1.0, 0.0, 1.0}


def _common(c, dense, scores):
    fmap, head, k = c["fmap"], c["head"], c["k"]
    assert fmap.shape[2:] == (H.MAP_H, H.MAP_W) and set(np.unique(fmap).tolist()) <= {0.0, 1.0, 2.0, 3.0}
    assert 0.4 < (fmap == 0).mean() < 0.6 or fmap.size < 4000
    assert c["rois"].shape == (300, 5) and c["rois"][:, 3].max() < H.IM_W and c["rois"][:, 4].max() < H.IM_H
    assert np.array_equal(c["pool5"], R.roi_pool(fmap, c["rois"])[0])          # (whichever RoIPool built the case)
    for w, b in dense:
        assert _is_ternary(head[w]) and np.array_equal(head[b], np.rint(head[b])) and np.abs(head[b]).max() <= 4
        if head[w].size >= 4000:
            assert 0.22 < (head[w] != 0).mean() < 0.28, w
    unit = 2.0 ** -k
    for name, w, b in scores:
        assert _is_ternary(head[w], unit) and (head[w] != 0).sum(axis=1).tolist() == [c["nnz"][name]] * head[w].shape[0]
        assert np.array_equal(head[b] / np.float32(unit), np.rint(head[b] / np.float32(unit)))
        pre = c["pre"][name]
        assert np.array_equal(pre / unit, np.rint(pre / unit)) and np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
        assert c["tol"][name] >= 1e-6
        assert c["unit_move"][name] > 4.0 * c["tol"][name], (name, c["unit_move"][name], c["tol"][name])
    top = max(float(np.abs(c["pre"][n]).max()) for n, _, _ in scores)
    assert top <= 4.0 and (k == 0 or top > 2.0)                                # (the smallest k)
    for layer, v in c["abs_sum"].items():
        assert v < 2.0 ** 24, (layer, v)
    assert np.array_equal(c["bbox"].astype(np.float64), np.rint(c["bbox"]))
    print("%s: k = %d, score non-zeros %s, max sum |w||x| %s, unit moves %s, tolerances %s"
          % (c["dims"], k, c["nnz"], {n: "%.3g" % v for n, v in c["abs_sum"].items()},
             {n: "%.2e" % v for n, v in c["unit_move"].items()}, {n: "%.2e" % v for n, v in c["tol"].items()}))


@pytest.mark.parametrize("dims", H.AZ_SIZES, ids=lambda d: "x".join(map(str, d)))
def test_integer_az_case(dims):
    c = H.int_az_case(dims)
    _common(c, (("W6", "b6"), ("W71", "b71"), ("W72", "b72"), ("Wab", "bab")), (("adj", "Was", "bas"), ("zoom", "Wz", "bz")))
    # the same head through the training restatement's float64 forward
    r = R.step(c["head"], c["pool5"][:64], {"zoom_labels": np.zeros(64), "adj_labels": np.zeros((64, 11)),
                                            "adj_targets": np.zeros((64, 44)), "adj_loss_weights": np.zeros((64, 44))},
               None, want_dpool=False)
    assert np.array_equal(r["adj_bbox"], c["bbox"][:64]) and np.array_equal(r["adj_score"], c["pre"]["adj"][:64])
    assert np.array_equal(r["zoom_score"], c["pre"]["zoom"][:64, 0])
    z, a, b = H.f64_head_on_pool5(c["head"], c["pool5"])
    assert np.array_equal(b, c["bbox"]) and np.array_equal(a, c["p64"]["adj"]) and np.array_equal(z, c["p64"]["zoom"])


@pytest.mark.parametrize("dims", H.DET_SIZES, ids=lambda d: "x".join(map(str, d)))
def test_integer_det_case(dims):
    c = H.int_det_case(dims)
    _common(c, (("W6", "b6"), ("W7", "b7"), ("Wb", "bb")), (("cls", "Wc", "bc"),))
    assert np.allclose(c["p64"]["cls"].sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_float64_head_is_the_training_restatements_forward():
    c = H.random_az_case((12, 132, 68, 36))
    pool = R.roi_pool(c["fmap"], c["rois"][:33])[0]
    r = R.step(c["head"], pool, {"zoom_labels": np.zeros(33), "adj_labels": np.zeros((33, 11)), "adj_targets": np.zeros((33, 44)),
                                 "adj_loss_weights": np.zeros((33, 44))}, None, want_dpool=False)
    z, a, b = H.f64_head_on_pool5(c["head"], pool)
    assert np.array_equal(b, r["adj_bbox"])
    assert np.abs(a - H.sigmoid64(r["adj_score"])).max() == 0 and np.abs(z[:, 0] - H.sigmoid64(r["zoom_score"])).max() == 0
    assert R.rel_err(H.sigmoid32(r["adj_score"]), a) < 1e-6
    x = np.random.Generator(np.random.PCG64(1)).standard_normal((5, 21)) * 3
    assert R.rel_err(H.softmax32(x), H.softmax64(x)) < 1e-6 and np.allclose(H.softmax64(x).sum(1), 1.0)


def _chunk(K, S):
    return (-(-K // S) + BK - 1) // BK * BK


def test_sizes_exercise_what_the_table_says():
    split = H.fc_split
    K6 = lambda d: 49 * d[0]                                                          # noqa: E731
    a = dict(zip(("min", "odd", "s8", "s16", "lds", "i7s8", "i7s16", "g528", "big"), H.AZ_SIZES))
    assert [split(K6(a[n])) for n in ("odd", "s8", "s16", "big")] == [2, 8, 16, 8]
    assert [split(a[n][1]) for n in ("min", "odd", "lds", "i7s8", "i7s16", "g528")] == [1, 1, 2, 8, 16, 8]
    # ragged K steps and short last slabs
    assert K6(a["odd"]) % BK and _chunk(K6(a["odd"]), 2) * 2 > K6(a["odd"])
    assert K6(a["s16"]) % BK and _chunk(K6(a["s16"]), 16) * 16 > K6(a["s16"]) and K6(a["s16"]) >= 16384
    assert a["min"][1] < BK and a["odd"][1] % BK and a["i7s8"][1] % BK and a["i7s16"][1] % BK
    # partial n-tiles; the int7_1 / int7_2 seam inside an n-tile
    assert a["odd"][1] % BN == 4 and a["s8"][2] > BN and a["s8"][2] % BN
    # work items of the tile GEMM against its grid
    tiles = lambda n: -(-n // BN)                                                     # noqa: E731
    assert tiles(a["g528"][1]) * split(K6(a["g528"])) == 528 > GRID
    # the second many-row shape: whole chunks of 1568
    assert a["big"] == H.AZ_LARGEST and _chunk(K6(a["big"]), 8) == 1568 and 1568 * 8 == K6(a["big"])
    assert (a["big"][1] // BN) * split(K6(a["big"])) >= 256
    # the tail kernel's LDS tile: n71 + n72 = 3072 is the last size that fits
    assert a["lds"][2] + a["lds"][3] == 3072 and H.AZ_REFUSED_LDS[2] + H.AZ_REFUSED_LDS[3] == 3076
    d = H.DET_SIZES
    assert d[1][2] % BK and d[2][2] % BK and d[3][2] % BK and d[0][2] < 8              # ragged / empty chunks of the tail GEMM
    assert [split(x[1]) for x in d] == [1, 1, 1, 8] and [x[3] for x in d] == [2, 21, 81, 256]
