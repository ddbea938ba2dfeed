"""CPU: truncated-SVD compression of the AZ head's int6 -- compress.compress_az_head, tools/compress_net.py --int6, the
model-file mapping, the AZ L stage's split and the ABI's new entries (references: tests/lowrank_az_ref.py)."""
import hashlib
import os
import sys

import numpy as np
import pytest

import head_sizes_ref as H
import lowrank_az_ref as AZ
import lowrank_ref as LR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")


@pytest.fixture(scope="module")
def tool():
    sys.path[:0] = [TOOLS]
    try:
        import compress_net
    finally:
        sys.path.remove(TOOLS)
    return compress_net


# ---- the split ------------------------------------------------------------------------------------------------------------
GRID_K = (4, 36, 128, 260, 588, 784, 2156, 4096, 8192, 12544, 16464, 25088)
GRID_R = (4, 36, 128, 132, 256, 512, 1024, 2048)


def test_az_split_is_a_function_of_k_and_r_and_keeps_the_many_row_kernel():
    """The library's split equals the restated rule over a grid of (K, r); every chunk is a non-empty multiple of the K
    step (32); where the restated `fits` predicate can hold for some split it holds for the chosen one, and it does at the
    paper's int6 (K = 25088, r = 1024) with 56 chunks of 448 -- of 49, 56, 98, 112, 196, 392 the one whose 448 groups leave the
    many-row kernel's 256 workgroups at most two each, 448 deep, for the fewest slabs."""
    from aznet_hip import ffi
    assert ffi.az_lowrank_split(25088, 1024) == 56
    assert [S for S in range(1, 25088 // 64 + 1) if AZ.fits12(1024, 25088, S)] == [49, 56, 98, 112, 196, 392]
    for K in GRID_K:
        for r in GRID_R:
            S = ffi.az_lowrank_split(K, r)
            assert S == AZ.az_split_ref(K, r), (K, r)
            Kc = AZ.fc_chunk(K, S)
            assert Kc % 32 == 0 and (S - 1) * Kc < K <= S * Kc, (K, r, S, Kc)
            could = r % 128 == 0 and any(AZ.fits12(r, K, s) for s in range(1, K // 64 + 1))
            assert AZ.fits12(r, K, S) == could, (K, r, S)
            if not could:
                assert S == LR.split_ref(K, r) == ffi.lowrank_split(K, r)
    assert AZ.fits12(1024, 25088, ffi.az_lowrank_split(25088, 1024))
    K = 49 * AZ.MANY[0]
    assert ffi.az_lowrank_split(K, AZ.MANY_RANK) == 294 and AZ.fits12(AZ.MANY_RANK, K, 294)
    assert not AZ.fits12(AZ.MANY[1], K, H.fc_split(K))                       # (the full int6 of that head stays on k_fc_splitk)
    assert not AZ.fits12(1024, 25088, ffi.lowrank_split(25088, 1024))          # (61 chunks of 416 do not divide K)
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ffi.AzError) as e:
            ffi.az_lowrank_split(*bad)
        assert e.value.code == ffi.AZ_ERR_INVALID


# ---- compress_az_head -------------------------------------------------------------------------------------------------------
def test_full_rank_reproduces_w6():
    from aznet_hip import compress, synth
    head = synth.make_head(seed=5, **synth.SMALL_DIMS)
    out, err = compress.compress_az_head(head, r6=min(head["W6"].shape))
    assert "W6" not in out and out["L6"].dtype == np.float32 and out["U6"].dtype == np.float32
    assert out["L6"].shape == (128, 784) and out["U6"].shape == (128, 128)
    for k in head:
        if k != "W6":
            assert out[k] is head[k], k
    U, Lf = out["U6"].astype(np.float64), out["L6"].astype(np.float64)
    back = U @ Lf
    # float32 rounding of the factors: |dU||L| + |U||dL| <= 2 eps32 sum_j |U_ij||L_jk|
    tol = 2 * np.finfo(np.float32).eps * (np.abs(U) @ np.abs(Lf)).max()
    assert np.abs(back - head["W6"]).max() <= tol + 1e-12, (np.abs(back - head["W6"]).max(), tol)
    assert err == compress.rel_error(head["W6"], out["L6"], out["U6"]) and err < 1e-6


@pytest.mark.parametrize("r", [4, 36])
def test_rank_r_reproduces_a_planted_rank_r_matrix(r):
    from aznet_hip import compress, synth
    head = synth.make_head(seed=6, **synth.SMALL_DIMS)
    s = np.concatenate([np.geomspace(30.0, 2.0, r), np.zeros(128 - r)])
    head["W6"] = LR.planted_spectrum(128, 784, s, seed=r).astype(np.float32)
    out, err = compress.compress_az_head(head, r6=r)
    assert out["L6"].shape == (r, 784) and out["U6"].shape == (128, r)
    back = out["U6"].astype(np.float64) @ out["L6"].astype(np.float64)
    # W6 is the planted matrix rounded to float32 (a perturbation of eps32 |W6| per entry, Frobenius norm <= eps32 ||W6||,
    # which the truncation can at most double) plus the float32 rounding of the factors
    eps = np.finfo(np.float32).eps
    assert np.linalg.norm(back - head["W6"]) <= 4 * eps * np.sqrt(r) * np.linalg.norm(head["W6"])
    assert err <= 4 * eps * np.sqrt(r)
    # one rank less loses the smallest planted singular value (Eckart-Young), to float32 rounding of the input
    _, err1 = compress.compress_az_head(head, r6=r - 1)
    assert abs(err1 - 2.0 / np.linalg.norm(s)) <= 1e-5


# ---- the tool and the model file -----------------------------------------------------------------------------------------
def test_compress_net_az_round_trip(tool, tmp_path, capsys):
    from aznet_hip import caffemodel as cm
    from aznet_hip import compress, synth
    out = str(tmp_path / "az_svd.caffemodel")
    path = tool.main(["--net", "synthetic:7", "--int6", "36", "--out", out])
    assert path == out and os.path.getsize(out) < (1 << 20)
    text = capsys.readouterr().out
    assert "int6 [128, 784] -> int6_L [36, 784] + int6_U [128, 36]" in text and text.count("||W - U L|| / ||W|| =") == 1
    layers = cm.load_caffemodel(out)
    assert list(layers) == ["int6_L", "int6_U", "int7_1", "int7_2", "adj_score", "adj_bbox", "zoom_score"]
    assert len(layers["int6_L"]) == 1 and len(layers["int6_U"]) == 2
    assert layers["int6_L"][0].size == 36 * 784 and layers["int6_U"][0].size == 128 * 36 and layers["int6_U"][1].size == 128
    head = cm.az_head_from_layers(layers)
    src = synth.make_head(seed=7, **synth.SMALL_DIMS)
    want, err = compress.compress_az_head(src, 36)
    assert "W6" not in head and set(head) == set(want)
    for k in want:
        assert head[k].dtype == np.float32 and np.array_equal(head[k], want[k]), k
    # the printed error is the Eckart-Young figure of the source weight
    s = np.linalg.svd(src["W6"].astype(np.float64), compute_uv=False)
    line = [ln for ln in text.splitlines() if ln.startswith("int6 ")][0]
    assert abs(float(line.split("=")[-1]) - np.sqrt((s[36:] ** 2).sum() / (s ** 2).sum())) < 1e-6
    assert abs(float(line.split("=")[-1]) - err) <= 0.5e-6 * err                  # (printed to seven digits)


def test_default_name_default_rank_and_refusals(tool, tmp_path, monkeypatch):
    from aznet_hip import caffemodel as cm
    from aznet_hip import synth
    monkeypatch.chdir(tmp_path)
    path = tool.main(["--net", "synthetic:3", "--int6", "8"])
    assert path == "vgg16_az_net_synthetic_3_svd_int6_8.caffemodel" and os.path.exists(path)
    # a file, recognised by its int6 layer, with no flag at all: rank 1024 -- which this reduced int6 cannot have
    head = synth.make_head(seed=3, **synth.SMALL_DIMS)
    full = str(tmp_path / "az.caffemodel")
    cm.write_caffemodel(full, tool.synthetic_az_layers(3))
    with pytest.raises(ValueError, match="rank 1024"):
        tool.main(["--net", full])
    again = tool.main(["--net", full, "--int6", "8"])
    assert again == str(tmp_path / "az_svd_int6_8.caffemodel")
    assert open(again, "rb").read() == open(path, "rb").read()
    assert np.array_equal(cm.az_head_from_layers(cm.load_caffemodel(full))["W6"], head["W6"])
    # an already compressed file has neither int6 nor fc6; so has a file of other layers
    with pytest.raises(ValueError, match="neither an int6 layer .* nor an fc6 layer"):
        tool.main(["--net", path, "--int6", "4"])
    other = str(tmp_path / "other.caffemodel")
    cm.write_caffemodel(other, {"int7_1": [head["W71"], head["b71"]]})
    with pytest.raises(ValueError, match="neither an int6 layer .* nor an fc6 layer"):
        tool.main(["--net", other])


def test_the_three_value_errors_of_az_head_from_layers(tool):
    from aznet_hip import caffemodel as cm
    layers, _ = tool.compress_az_layers(tool.synthetic_az_layers(7), 36, log=lambda s: None)
    cm.az_head_from_layers(layers)
    for drop in ("int6_L", "int6_U"):
        half = {k: v for k, v in layers.items() if k != drop}
        with pytest.raises(ValueError, match="needs both"):
            cm.az_head_from_layers(half)
    both = dict(layers)
    both["int6"] = tool.synthetic_az_layers(7)["int6"]
    with pytest.raises(ValueError, match="int6 and its compressed pair"):
        cm.az_head_from_layers(both)
    loose = dict(layers)
    loose["int6_L"] = [layers["int6_L"][0].ravel()[:-1]]            # 36 * 784 - 1 values: no whole rows of int6_U's rank
    with pytest.raises(ValueError, match="does not chain"):
        cm.az_head_from_layers(loose)


def test_the_detection_file_is_written_as_before(tool, tmp_path):
    """Same arguments, same bytes: the detection branch of the tool writes what its own functions (unchanged: synthetic_layers,
    compress_layers, write_caffemodel) give, in the file's order, under the name it had."""
    from aznet_hip import caffemodel as cm
    out = str(tmp_path / "det.caffemodel")
    assert tool.main(["--net", "synthetic:7", "--fc6", "36", "--fc7", "20", "--out", out]) == out
    want = str(tmp_path / "want.caffemodel")
    layers, _ = tool.compress_layers(tool.synthetic_layers(7), 36, 20, log=lambda s: None)
    cm.write_caffemodel(want, layers)
    a, b = open(out, "rb").read(), open(want, "rb").read()
    assert hashlib.sha256(a).hexdigest() == hashlib.sha256(b).hexdigest()
    assert list(cm.load_caffemodel(out)) == ["fc6_L", "fc6_U", "fc7_L", "fc7_U", "cls_score", "bbox_pred"]
    # the bytes of the commit before this feature, recorded from its tool for `--net synthetic:7 --fc6 0 --fc7 0` (no SVD in
    # it, so no LAPACK or GPU rounding either: layer order, blob layout and the synthetic head are what it pins); with ranks
    # the same call gave sha256 109dd5d8...f62b there and here on one machine's NumPy SVD, which no test can pin elsewhere
    out0 = str(tmp_path / "det0.caffemodel")
    tool.main(["--net", "synthetic:7", "--fc6", "0", "--fc7", "0", "--out", out0])
    assert hashlib.sha256(open(out0, "rb").read()).hexdigest() == "c022d5a3a91bc18d8ac41243e393b1f9cd104129439cd9d1b45a3c61357c82c3"
    # --int6 beside a detection flag still means the detection net's synthetic head
    out2 = str(tmp_path / "det2.caffemodel")
    tool.main(["--net", "synthetic:7", "--fc6", "36", "--fc7", "20", "--int6", "8", "--out", out2])
    assert open(out2, "rb").read() == a


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_exported():
    from aznet_hip import compress, ffi
    L = ffi.load_library()
    for name in ("az_load_head_lowrank", "az_az_lowrank_split"):
        assert name in ffi.SYMBOLS and hasattr(L, name), name
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    for name in ("az_load_head_lowrank", "az_az_lowrank_split"):
        assert "int %s(" % name in src, name
    assert "compress_az_head" in compress.__all__
    assert hasattr(ffi.AzContext, "load_head_lowrank")


def test_planted_az_heads_are_exact():
    """A self-check of the fixtures, not of the feature (it runs no code of it): the integer cases of the GPU test have every
    partial sum below 2^24, W6 = U6 L6 integer, and both evaluations give the same integers."""
    for dims, r in ((AZ.SMALL, 4), (AZ.SMALL, 128), (AZ.ODD, 36)):
        c = AZ.planted_az_head(dims, r, rois=H.rois300()[:40])
        assert max(c["abs_sum"].values()) < AZ.EXACT
        W = c["full"]["W6"]
        assert np.array_equal(W, np.rint(W)) and W.shape == (dims[1], 49 * dims[0])
        lo = AZ.head_on_pool5(c["head"], c["pool5"], np.float64)
        fu = AZ.head_on_pool5(c["full"], c["pool5"], np.float64)
        for a, b in zip(lo, fu):
            assert np.array_equal(a, b)
        assert np.array_equal(lo[2].astype(np.float32), c["bbox"]) and (c["bbox"] != 0).mean() > 0.5
        assert np.abs(lo[0] - c["p64"]["zoom"]).max() < 1e-12 and np.abs(lo[1] - c["p64"]["adj"]).max() < 1e-12


def test_zoom_exact_factors_keep_the_planted_path():
    """A self-check of the search fixture: in float32, in either order of the L stage's terms, units 0 and 1 of int6 and
    the zoom score of the compressed head are the full head's on 0/1 zoom-channel rows."""
    import search_limits_ref as R
    from aznet_hip import synth
    kw = dict(R.HEAD_KW)
    kw.update(synth.SMALL_DIMS)
    head = synth.make_object_head(**kw)
    low = AZ.zoom_exact_factors(head, 36)
    assert low["L6"].shape == (36, 784) and low["U6"].shape == (128, 36) and "W6" not in low
    rng = np.random.Generator(np.random.PCG64(1))
    p5 = rng.standard_normal((64, 784)).astype(np.float32)
    p5[:, :49] = rng.integers(0, 2, (64, 49))
    p5[:8, :49] = 0                                                 # (windows without a planted cell)
    for order in (slice(None), slice(None, None, -1)):
        z_lo = AZ.head_on_pool5({k: (v[:, order] if k == "L6" else v) for k, v in low.items()}, p5[:, order], np.float32)[0]
        z_fu = AZ.head_on_pool5(head, p5, np.float32)[0]
        assert np.array_equal(z_lo, z_fu)
    assert set(np.unique(AZ.head_on_pool5(low, p5, np.float32)[0] > R.TZ)) == {False, True}
