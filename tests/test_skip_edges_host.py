"""CPU: the input conditions of tests/test_gpu_skip_edges.py, asserted on the references alone (tests/skip_ref.py,
tests/skip_train_ref.py), so that the comparison with the device is never the first place a reference runs.

  * the float32 restatement stays as close to float64 as float32 arithmetic allows at every new configuration (CLOSE and
    CAT_CLOSE below: figures from the number format and the lengths of the sums, not from what the runs give), and nothing
    in either is non-finite;
  * the share of empty bins: under one half per source, except on the maps of 5 x 9 / 1 x 16 / 1 x 1 cells, where every
    source has at least 49 bins that are not empty;
  * on the tie-heavy maps with eps = 0 every sum of squares is a whole number in float64;
  * the ReLU gates: the first of skip_train_ref.SEED_TRIALS for which no float64 pre-activation of relu_pool, fc6 or fc7
    lies within twice the forward bound of zero is the seed recorded in skip_train_ref.STEP_SEEDS -- with it the device's
    gates have to be float64's exactly;
  * the gather's whole-number sums stay below 2^24, every x-range and y-range of the sweep occurs, window sizes of 1 to 6
    cells, multiples of 7 and their neighbours are among them.
Every figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest

import skip_ref as S
import skip_train_ref as T

# How far the float32 restatement may be from float64, as a share of the tensor's largest magnitude.  One float32 rounding is
# 2^-24 = 6.0e-8.  `cat` is a sum of squares, a square root, a division and a product: 8 roundings' worth, 5e-7, whatever the
# channel count (NumPy sums pairwise).  Every other tensor is behind a chain of at most 8 matrix products or reductions (front,
# fc6, fc7, scores, and back) whose longest sum has 1552 terms (sumC of the mixed channel set; R * 49 <= 980 rows, 588 fc6
# inputs): roundings that add like a random walk give 8 * sqrt(1552) * 2^-24 = 1.9e-5, so 2e-5.  A restatement that drops a
# term or takes a stage in another precision is orders of magnitude outside both.
EPS32 = 2.0 ** -24
CAT_CLOSE = 5e-7
CLOSE = 2e-5
assert 8 * EPS32 <= CAT_CLOSE and 8 * np.sqrt(1552) * EPS32 <= CLOSE
STEP_TENSORS = ("cat", "pool5", "pre6", "a6", "pre7", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score", "d_bbox_pred", "d_pre7",
                "d_pre6", "d_pool5", "d_y", "d_cat", "d_raw", "losses")


def close(name, r32, r64):
    e = T.rel_err(r32, r64)
    print("  %-14s float32 vs float64 %.3e   (bound of the GPU test %.3e)" % (name, e, T.bound(e)))
    assert np.isfinite(np.asarray(r32, np.float64)).all() and np.isfinite(np.asarray(r64, np.float64)).all(), name
    return e


# ---- 1. the channel sets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["relu", "ties"])
@pytest.mark.parametrize("Cs", S.CHANNEL_SETS, ids=lambda Cs: "x".join(map(str, Cs)))
def test_channel_set_reference(Cs, kind):
    c = T.channel_reference(Cs, kind)
    assert sum(Cs) <= 4096 and all(C % 4 == 0 for C in Cs) and c["raw"].shape == (20 * 49, sum(Cs))
    shares = S.empty_share(c["arg"], Cs)
    print("  %s %s: empty bins per source %s" % (Cs, kind, ", ".join("%.3f" % s for s, _ in shares)))
    assert all(0.0 < s < 0.5 for s, _ in shares)                        # (empty bins are in the set: the hostile rois)
    assert close("cat", c["cat32"], c["f64"]["cat"]) <= CAT_CLOSE
    tot, fac = c["f64"]["tot"], c["f64"]["fac"]
    assert (fac[tot == 0] == 0).all() and np.isfinite(fac).all()
    if kind == "ties":
        assert c["front"]["eps"] == 0.0 and set(np.unique(c["raw"])) <= {0.0, 1.0, 2.0, 3.0}
        assert np.array_equal(tot, np.rint(tot)) and tot.max() < 2.0 ** 53 and (tot == 0).any() and (tot > 0).any()
        # ties are what the maps are for: windows of zeros alone (every cell ties) and windows whose maximum is the largest
        # value there is (any second 3 ties), past 1024 channels on both sides of the pass boundary
        live = c["arg"] >= 0
        assert (c["raw"][live] == 3).mean() > 0.1 and (c["raw"][live] == 0).mean() > 0.1
        if max(Cs) > 1024:
            off = T.offsets(Cs)[int(np.argmax(Cs))]
            assert live[:, off:off + 1024].any() and live[:, off + 1024:off + max(Cs)].any()
    else:
        assert c["front"]["eps"] == 1e-10 and (c["raw"] == 0).mean() > 0.05


# ---- 2 - 4. the steps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.STEP_CASES))
def test_step_reference(name):
    seed = T.find_seed(name)
    for s in T.SEED_TRIALS[:T.SEED_TRIALS.index(seed) + 1 if seed is not None else None]:
        print("  seed %d: " % s + "; ".join("%s min |pre| %.3e, twice the forward bound %.3e" % m for m in T.edge_reference(name, s)["margins"]))
    assert seed is not None, "no seed of SEED_TRIALS keeps every pre-activation outside twice the forward bound"
    print("  %s: seed %d (recorded %d)" % (name, seed, T.STEP_SEEDS[name]))
    assert seed == T.STEP_SEEDS[name]
    r = T.edge_reference(name, seed)
    d, r64, r32 = T.STEP_CASES[name], r["r64"], r["r32"]
    Cs, Rn = d["Cs"], r["blobs"]["rois"].shape[0]
    assert [m.shape[1:] for m in r["maps"]] == [(C,) + tuple(hw) for C, hw in zip(Cs, d["hw"])] and len(r["scales"]) == len(Cs)
    assert all(np.array_equal(r64["gates"][k], r32["gates"][k]) for k in ("pool", 6, 7))
    shares = S.empty_share(r["pooled"][1], Cs)
    print("  empty bins per source: " + ", ".join("%.3f (%d not empty)" % s for s in shares))
    if name == "tiny":
        assert all(n >= 49 for _, n in shares)
    else:
        assert all(s < 0.5 for s, _ in shares)
    assert close("cat", r32["cat"], r64["cat"]) <= CAT_CLOSE
    worst = max(close(nm, r32[nm], r64[nm]) for nm in STEP_TENSORS)
    worst = max([worst] + [close("g_" + k, r32["grads"][k], r64["grads"][k]) for k in T.KEYS])
    worst = max([worst] + [close("d map %d" % i, a, b) for i, (a, b) in enumerate(zip(r32["dmaps"], r64["dmaps"]))])
    assert worst <= CLOSE
    live = [i for i in range(len(Cs)) if i not in d.get("zero", ())]
    if d.get("gain", 1000.0) != 0.0:
        assert 0.2 < (r64["pool5"] > 0).mean() < 0.8 and all(np.abs(r64["dmaps"][i]).max() > 0 for i in live)
    # what the GPU test asserts exactly must first be so in the reference
    if name == "gain0":
        assert not r64["cat"].any() and not r64["grads"]["Wp"].any() and not any(m.any() for m in r64["dmaps"])
        assert np.array_equal(r64["pool5"], T.flatten_caffe(np.tile(np.maximum(r["front"]["bp"].astype(np.float64), 0), (Rn * 49, 1)), Rn))
        assert np.abs(r64["grads"]["bp"]).max() > 0
    if name == "eps0_zero_source":
        assert not r["maps"][1].any() and not r64["dmaps"][1].any() and not r32["dmaps"][1].any()
        o = T.offsets(Cs)
        assert not r64["cat"][:, o[1]:o[2]].any() and not r64["d_raw"][:, o[1]:o[2]].any()
    if name == "image_without_rois":
        assert sorted(set(r["blobs"]["rois"][:, 0])) == [0.0, 2.0] and r["maps"][0].shape[0] == 3
        assert all(not m[1].any() and m[0].any() and m[2].any() for m in r64["dmaps"])
    if name == "r1":
        assert Rn == 1 and r["blobs"]["rois"][0, 0] == 1
    if name == "gain_negative":
        assert r["front"]["gain"] == -2.5 and (r64["cat"] <= 0).all() and (r64["cat"] < 0).any()
    if name == "gain1_eps1":
        # eps weighs in: it is a fifth or more of the smallest non-empty sum of squares
        tot = (r["pooled"][0].astype(np.float64) ** 2)[:, :Cs[0]].sum(1)
        assert r["front"]["eps"] == 1.0 and 1.0 / (tot[tot > 0].min() + 1.0) > 0.05


def test_fetch_shapes_of_the_reference_factor():
    for name in ("one", "two"):
        r = T.edge_reference(name, T.STEP_SEEDS[name])
        fw = T.front_forward(r["front"], r["pooled"][0], T.STEP_CASES[name]["Cs"])
        assert fw["fac"].shape == (r["blobs"]["rois"].shape[0] * 49, len(T.STEP_CASES[name]["Cs"]))


# ---- 3, 7. the gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["sweep_ties", "sweep_perm", "all_in_last", "descending"])
def test_gather_reference(tag):
    g = T.gather_reference(tag)
    Cs = tuple(int(m.shape[1]) for m in g["maps"])
    shares = S.empty_share(g["arg"], Cs)
    big = max(float(np.abs(w).max()) for w in g["want"])
    print("  %s: %d rois, empty bins per source %s, largest |sum| %.0f" % (tag, g["rois"].shape[0], ", ".join("%.4f" % s for s, _ in shares), big))
    assert all(s < 0.5 for s, _ in shares) and 0 < big < 2 ** 24
    assert all(np.array_equal(w, np.rint(w)) for w in g["want"]) and np.abs(g["d_raw"]).max() == 8
    if tag.startswith("sweep"):
        rois, xs, ys = S.sweep_rois()
        assert rois.shape == (2048, 5) and np.array_equal(rois, np.rint(rois))
        assert {(a, b) for a, b in rois[:, [1, 3]]} >= set(xs) and {(a, b) for a, b in rois[:, [2, 4]]} >= set(ys)
        # windows of one and two cells on the last column and the last row (the hand-added rois)
        W, Hh = S.SWEEP["W"], S.SWEEP["H"]
        assert {(W - 1, W - 1), (W - 2, W - 1)} <= {(a, b) for a, b in rois[:, [1, 3]]}
        assert {(Hh - 1, Hh - 1), (Hh - 2, Hh - 1)} <= {(a, b) for a, b in rois[:, [2, 4]]}
        assert (g["arg"] == Hh * W - 1).any()
        widths = set(S.SWEEP["widths"])
        assert {b - a + 1 for a, b in xs} == widths == {b - a + 1 for a, b in ys}
        assert widths >= set(range(1, 10)) | {13, 14, 15} and min(a for a, _ in xs) < 0 and max(b for _, b in xs) >= S.SWEEP["W"]
        m = g["maps"][0]
        if tag == "sweep_perm":
            assert all(len(np.unique(m[0, c])) == m[0, c].size for c in range(m.shape[1]))
        else:
            assert set(np.unique(m)) == {0.0, 1.0, 2.0, 3.0}
        # windows narrower than 7 cells replicate bins: one cell is then the arg-max of several bins of a roi
        a = g["arg"].reshape(2048, 49, -1)[:, :, 0]
        assert max(int(np.bincount(r[r >= 0]).max()) for r in a[:200] if (r >= 0).any()) >= 7
    else:
        assert set(g["rois"][:, 0]) == ({2.0} if tag == "all_in_last" else {0.0, 1.0, 2.0})
        if tag == "descending":
            assert (np.diff(g["rois"][:, 0]) <= 0).all()


# ---- 2. the inference head at one and two sources, other scales and map shapes ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.SOURCE_CASES))
def test_inference_reference(name):
    from oracle import az_oracle as orc
    c = S.source_case(name)
    assert 6 <= c["rois"].shape[0] <= 9 and c["front"]["scales"] == tuple(c["scales"]) and c["front"]["Wp"].shape == (12, sum(c["Cs"]))
    r64, r32 = S.det_forward(c["front"], c["head"], c["maps"], c["rois"], np.float64), S.det_forward(c["front"], c["head"], c["maps"], c["rois"], np.float32)
    assert close("cls_prob", r32[0], r64[0]) <= CLOSE and close("bbox_pred", r32[1], r64[1]) <= CLOSE
    names = S.NAMES[3 - len(c["Cs"]):]                                 # (the oracle reshapes a blob named conv5_3)
    s64, b64 = S.detect(orc, c["front"], c["head"], c["maps"], c["boxes"], 1.0, (S.IM_H, S.IM_W), 1. / 16., np.float64, names=names)
    s32, b32 = S.detect(orc, c["front"], c["head"], c["maps"], c["boxes"], 1.0, (S.IM_H, S.IM_W), 1. / 16., np.float32, names=names)
    assert close("detect boxes", b32, b64) <= CLOSE and b32.shape == b64.shape
    assert s64.shape == (c["boxes"].shape[0], 21) and b64.shape == (c["boxes"].shape[0], 84) and close("detect scores", s32, s64) <= CLOSE
    assert np.array_equal(s64[-3:], s64[:3])                              # the copies share their original's row
    _, arg = T.pool_argmax(c["maps"], c["rois"], c["scales"])
    shares = S.empty_share(arg, c["Cs"])
    print("  %s: empty bins per source %s" % (name, ", ".join("%.3f (%d not empty)" % s for s in shares)))
    assert all(n >= 49 for _, n in shares) if name == "tiny" else all(s < 0.5 for s, _ in shares)
