"""CPU: truncated-SVD compression of the detection head -- aznet_hip.compress, tools/compress_net.py, the model-file
mapping and the ABI's new entries (references: tests/lowrank_ref.py)."""
import os
import sys

import numpy as np
import pytest

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


# ---- compress_layer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 96), (96, 40), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_truncation_error_is_eckart_young(shape):
    """||W - U L||_F = sqrt(sum_{i >= r} s_i^2) for a planted spectrum, to 1e-10 relative in float64 (the factors are
    float32, so the product is compared against the float64 truncation the same SVD gives, and the float64 factors against
    the formula)."""
    from aznet_hip import compress
    k = min(shape)
    s = np.geomspace(50.0, 1e-3, k)
    W = LR.planted_spectrum(shape[0], shape[1], s, seed=sum(shape))
    for r in (4, 12, k - 4, k):
        U_, s_, Vt_ = compress._svd64(W)
        assert np.allclose(s_, s, rtol=1e-10, atol=0)
        err = np.linalg.norm(W - (U_[:, :r] * s_[:r]) @ Vt_[:r])
        want = np.sqrt((s[r:] ** 2).sum())
        assert abs(err - want) <= 1e-10 * np.linalg.norm(W), (r, err, want)
        Lf, U = compress.compress_layer(W, r)
        assert Lf.dtype == np.float32 and U.dtype == np.float32 and Lf.shape == (r, shape[1]) and U.shape == (shape[0], r)
        # the float32 factors: the same truncation to float32 rounding of the factors (compared through U L only)
        got = U.astype(np.float64) @ Lf.astype(np.float64)
        trunc = (U_[:, :r] * s_[:r]) @ Vt_[:r]
        assert np.abs(got - trunc).max() <= 4 * np.finfo(np.float32).eps * r * np.abs(U_[:, :r]).max() * np.abs(s_[:r, None] * Vt_[:r]).max()
        assert abs(compress.rel_error(W, Lf, U) - want / np.linalg.norm(W)) <= 1e-5
        Lr, Ur = LR.compress_layer(W, r)
        assert np.allclose(Ur.astype(np.float64) @ Lr.astype(np.float64), got, rtol=0, atol=1e-5 * s[0])


def test_full_rank_reproduces_the_weight():
    from aznet_hip import compress
    rng = np.random.Generator(np.random.PCG64(3))
    for shape in ((36, 100), (100, 36)):
        W = rng.standard_normal(shape).astype(np.float32)
        Lf, U = compress.compress_layer(W, min(shape))
        back = U.astype(np.float64) @ Lf.astype(np.float64)
        # float32 rounding of the factors: |dU||L| + |U||dL| <= 2 eps32 sum_j |U_ij||L_jk|
        tol = 2 * np.finfo(np.float32).eps * (np.abs(U).astype(np.float64) @ np.abs(Lf).astype(np.float64)).max()
        assert np.abs(back - W).max() <= tol + 1e-12, (np.abs(back - W).max(), tol)
    with pytest.raises(ValueError):
        compress.compress_layer(W, min(shape) + 1)
    with pytest.raises(ValueError):
        compress.compress_layer(W, 0)


def test_compress_det_head_keeps_everything_else():
    from aznet_hip import compress, synth
    head = synth.make_det_head(seed=5, **synth.SMALL_DET_DIMS)
    head["skip_front"] = {"marker": 1}
    for r6, r7 in ((36, 20), (36, 0), (0, 20)):
        out = compress.compress_det_head(head, r6, r7)
        assert ("W6" in out) == (not r6) and ("L6" in out) == bool(r6) and ("W7" in out) == (not r7) and ("L7" in out) == bool(r7)
        for k in ("b6", "b7", "Wc", "bc", "Wb", "bb", "skip_front"):
            assert out[k] is head[k]
        if r6:
            assert out["L6"].shape == (r6, head["W6"].shape[1]) and out["U6"].shape == (head["W6"].shape[0], r6)


# ---- the tool and the model file -----------------------------------------------------------------------------------------
def _skip_cfg(tmp_path):
    y = tmp_path / "skip.yml"
    y.write_text("SEAR:\n  FRCNN_CONV: [conv3_3, conv4_3, conv5_3]\n")
    return str(y)


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip_cfg"])
def test_compress_net_round_trip(tool, tmp_path, capsys, skip):
    from aznet_hip import caffemodel as cm
    from aznet_hip import compress, synth
    from detect import config as C
    saved = list(C.cfg.SEAR.FRCNN_CONV)
    out = str(tmp_path / "net_svd.caffemodel")
    try:
        path = tool.main(["--net", "synthetic:7", "--fc6", "36", "--fc7", "20", "--out", out] +
                         (["--cfg", _skip_cfg(tmp_path)] if skip else []))
    finally:
        C.cfg.SEAR.FRCNN_CONV = saved
    assert path == out and os.path.getsize(out) < (1 << 20)
    text = capsys.readouterr().out
    assert "fc6_L [36, 784]" in text and "fc7_U [96, 20]" in text and text.count("||W - U L|| / ||W|| =") == 2
    layers = cm.load_caffemodel(out)
    assert set(layers) == {"fc6_L", "fc6_U", "fc7_L", "fc7_U", "cls_score", "bbox_pred"} | ({"conv_pool5"} if skip else set())
    assert len(layers["fc6_L"]) == 1 and len(layers["fc6_U"]) == 2 and len(layers["fc7_L"]) == 1 and len(layers["fc7_U"]) == 2
    head = cm.det_head_from_layers(layers)
    src = synth.make_det_head(seed=7, **synth.SMALL_DET_DIMS)
    want = compress.compress_det_head(src, 36, 20)
    assert "W6" not in head and "W7" not in head
    for k in ("L6", "U6", "b6", "L7", "U7", "b7", "Wc", "bc", "Wb", "bb"):
        assert head[k].dtype == np.float32 and np.array_equal(head[k], want[k]), k
    assert np.array_equal(head["b6"], src["b6"]) and np.array_equal(head["b7"], src["b7"])
    if skip:
        C_ = synth.SMALL_DET_DIMS["C"]
        front = synth.make_skip_front(seed=9, Cs=synth.SKIP_CS, Cout=C_)
        assert np.array_equal(head["skip_front"]["Wp"], front["Wp"]) and np.array_equal(head["skip_front"]["bp"], front["bp"])
    else:
        assert "skip_front" not in head
    # the printed error is the Eckart-Young figure of the source weight
    s = np.linalg.svd(src["W6"].astype(np.float64), compute_uv=False)
    line = [ln for ln in text.splitlines() if ln.startswith("fc6 ")][0]
    assert abs(float(line.split("=")[-1]) - np.sqrt((s[36:] ** 2).sum() / (s ** 2).sum())) < 1e-6


def test_default_name_and_one_layer_only(tool, tmp_path, monkeypatch, capsys):
    from aznet_hip import caffemodel as cm
    monkeypatch.chdir(tmp_path)
    path = tool.main(["--net", "synthetic:3", "--fc6", "0", "--fc7", "20"])
    assert path == "vgg16_frcnn_synthetic_3_svd_fc6_0_fc7_20.caffemodel" and os.path.exists(path)
    layers = cm.load_caffemodel(path)
    assert "fc6" in layers and "fc6_L" not in layers and "fc7_L" in layers and "fc7" not in layers
    head = cm.det_head_from_layers(layers)
    assert "W6" in head and "L7" in head and "W7" not in head
    # a file that is already compressed has no fc7 left to compress
    with pytest.raises(ValueError, match="no fc7"):
        tool.main(["--net", path, "--fc6", "0", "--fc7", "8"])


@pytest.mark.parametrize("drop", ["fc6_L", "fc6_U", "fc7_L", "fc7_U"])
def test_half_a_pair_raises(tool, drop):
    from aznet_hip import caffemodel as cm
    layers, _ = tool.compress_layers(tool.synthetic_layers(7), 36, 20, log=lambda s: None)
    cm.det_head_from_layers(layers)
    del layers[drop]
    with pytest.raises(ValueError, match="needs both"):
        cm.det_head_from_layers(layers)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_exported():
    from aznet_hip import ffi
    L = ffi.load_library()
    for name in ("az_load_det_head_lowrank", "az_lowrank_gemm_unit", "az_lowrank_split"):
        assert name in ffi.SYMBOLS and hasattr(L, name), name
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    import re
    assert int(re.search(r"#define\s+AZ_LOWRANK_MAX\s+(\d+)", src).group(1)) == ffi.AZ_LOWRANK_MAX == LR.UNIT_K[-1]


def test_split_count_is_a_function_of_k_and_r():
    """The L stage's number of K chunks: host arithmetic of (K, r) alone -- the entry takes no row count and no context --,
    every chunk a non-empty multiple of the GEMM's K step (32), of at least 64 where there are several (the count comes
    from chunks of >= 128; re-cutting K into that many equal chunks can at most halve them), and 8 n-tiles x 61
    chunks = 488 of the 512 resident workgroups at the paper's fc6 (K = 25088, r = 1024)."""
    from aznet_hip import ffi
    assert ffi.lowrank_split(25088, 1024) == 61 and ffi.lowrank_split(4096, 256) == 32
    for K in (4, 36, 128, 260, 588, 2156, 4096, 16464, 25088):
        for r in (4, 36, 128, 132, 256, 1024, 2048):
            S = ffi.lowrank_split(K, r)
            assert S == ffi.lowrank_split(K, r) and 1 <= S <= 512
            Kc = -(-(-(-K // S)) // 32) * 32                     # the GEMM's chunk: ceil(K / S) rounded up to the K step
            assert (S - 1) * Kc < K <= S * Kc, (K, r, S, Kc)
            assert S == 1 or Kc >= 64, (K, r, S, Kc)
            assert S * -(-r // 128) <= 512
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ffi.AzError) as e:
            ffi.lowrank_split(*bad)
        assert e.value.code == ffi.AZ_ERR_INVALID
    assert ffi.is_lowrank_head({"L6": 0, "U6": 0}) and not ffi.is_lowrank_head({"W6": 0, "W7": 0})


def test_planted_heads_are_exact():
    """A self-check of the fixtures, not of the feature (it runs no code of it): the integer cases of the GPU test have
    every partial sum below 2^24, W = U L integer, and both evaluations give the same integers."""
    for ncls, r6, r7 in ((21, 4, 0), (81, 0, 128), (21, 128, 36)):
        c = LR.planted_head(ncls, r6, r7)
        assert c["abs_sum"] < LR.EXACT
        for i in (6, 7):
            W = c["full"]["W%d" % i]
            assert np.array_equal(W, np.rint(W))
        p_lr, b_lr = LR.head_on_pool5(c["head"], c["pool5"], np.float64)
        p_fu, b_fu = LR.head_on_pool5(c["full"], c["pool5"], np.float64)
        assert np.array_equal(b_lr, b_fu) and np.array_equal(b_lr.astype(np.float32), c["bbox"]) and np.abs(c["bbox"]).max() > 0
        assert np.array_equal(p_lr, p_fu) and np.abs(p_lr - c["p64"]).max() < 1e-12
        assert (c["bbox"] != 0).mean() > 0.5
