"""CPU: the conditions that tests/test_gpu_solver_edges.py relies on, asserted on the references alone (the cases are built
in tests/solver_edges_ref.py): the pinned element of the dropout mask that tells the float32 ratio's threshold from the
double's; the float32 dropout scale against float64's; the restatement off its defaults (ratio 0 ignores the mask, lr_mult 0
freezes a blob, RefTrajectory carries both); the float32 gates under the cap for the new cases; how hostile the 43 rois are
(empty bins, tied windows, cells outside every window) and that np.add.at adds in the order the backward kernel documents;
that every integer GEMM case is exact in float32; and where the SmoothL1 case lands."""
import numpy as np
import pytest

import solver_edges_ref as E
import train_step_ref as R

LAYERS = ((6, 0, "b6"), (71, 1, "b71"), (72, 2, "b72"))


def _word(seed, iteration, layer, e):
    """The generator's 24-bit word of element e (include/aznet_hip.h's formula in Python integers)."""
    M, G = (1 << 64) - 1, 0x9E3779B97F4A7C15

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    key = mix((mix((mix((seed + G) & M) + iteration) & M) + layer) & M)
    return mix((key + G * (e + 1)) & M) >> 40


def test_mask_threshold_is_the_float32_ratios():
    from aznet_hip import ffi
    M = E.MASK_CASE
    e = M["row"] * 128 + M["unit"]
    assert e == 2766 and _word(M["seed"], M["iteration"], 0, e) == 5033164
    # (ratio, threshold from the double, threshold from the float32 the trainer holds): they differ for these three
    for ratio, t64, t32 in ((0.3, 5033164, 5033165), (0.6, 10066329, 10066330), (0.8, 13421772, 13421773)):
        assert int(ratio * 16777216.0) == t64 and int(float(np.float32(ratio)) * 16777216.0) == t32
    for ratio in (0.1, 0.2, 0.25, 0.5, 0.75):
        assert int(ratio * 16777216.0) == int(float(np.float32(ratio)) * 16777216.0)
    n = M["rows"] * 128
    m = ffi.dropout_mask(M["seed"], M["iteration"], 0, n, ratio=0.3)
    assert m[e] == 0                                                   # 5033164 >= 5033165 is false: dropped
    words = np.array([_word(M["seed"], M["iteration"], 0, i) for i in range(2700, 2800)])
    assert np.array_equal(m[2700:2800], (words >= 5033165).astype(np.uint8))
    for l, ratio in enumerate(M["ratios"]):
        m = ffi.dropout_mask(M["seed"], M["iteration"], l, 1 << 16, ratio=ratio)
        assert abs(m.mean() - (1 - ratio)) < 4 * 0.5 / np.sqrt(m.size)
        assert np.array_equal(m, ffi.dropout_mask(M["seed"], M["iteration"], l, 1 << 16, ratio=np.float32(ratio)))


def test_dropout_scale_of_the_float32_ratio():
    """R.step rounds the ratio to float32 in both dtypes: in float32 its scale IS the kernel's 1.0f / (1.0f - ratio), and the
    float64 scale rounds to it for every ratio in use (with the double ratio it does not, at 0.6, 0.8 and 0.9)."""
    off = []
    for r in (0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9):
        s32 = E.f32_scale(r)
        assert np.float32(1.0 / (1.0 - float(np.float32(r)))) == s32, r
        if np.float32(1.0 / (1.0 - r)) != s32:
            off.append(r)
    assert off == [0.6, 0.8, 0.9]
    x = np.array([[1.0, 3.0]], np.float32)
    head = {k: np.zeros((2, 2) if k[0] == "W" else 2, np.float32) for k in R.KEYS}
    head["W6"] = np.eye(2, dtype=np.float32)
    for k, n in (("Was", 11), ("Wab", 44), ("Wz", 1)):
        head[k], head["b" + k[1:]] = np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
    blobs = dict(adj_labels=np.zeros((1, 11)), adj_targets=np.zeros((1, 44)), adj_loss_weights=np.zeros((1, 44)), zoom_labels=np.zeros(1))
    keep = {t: np.ones((1, 2), np.uint8) for t in (6, 71, 72)}
    for dt in (np.float32, np.float64):
        a6 = R.step(head, x, blobs, keep, dtype=dt, ratios=(0.3, 0.5, 0.5))["a6"]
        assert np.array_equal(a6.astype(np.float32), x * E.f32_scale(0.3))


def _masks(seed, it, n, head, ratios):
    from aznet_hip import ffi
    return {t: ffi.dropout_mask(seed, it, l, n * head[k].shape[0], ratio=ratios[l]).reshape(n, -1) for t, l, k in LAYERS if ratios[l] > 0}


@pytest.mark.parametrize("rows", E.HYPER_ROWS)
@pytest.mark.parametrize("ratios", E.RATIO_SETS, ids=lambda r: "-".join("%g" % x for x in r))
def test_restatement_with_other_hyper_parameters(ratios, rows):
    """The float32 restatement's gates stay under device_gates' cap for the new cases; a zero ratio ignores its mask; the
    multipliers do what the GPU test expects of them."""
    head, fmap, blobs = R.small_case(R=rows)
    pool, _ = R.roi_pool(fmap, blobs["rois"])
    masks = _masks(3, 0, rows, head, ratios)
    assert sorted(masks) == [t for t, l, _ in LAYERS if ratios[l] > 0]
    r64 = R.step(head, pool, blobs, masks, ratios=ratios, want_dpool=False)
    r32 = R.step(head, pool, blobs, masks, dtype=np.float32, ratios=ratios, want_dpool=False)
    for t, l, _ in LAYERS:
        frac = R.gate_mismatch(r32["pre%d" % t], r64["pre%d" % t])
        print("ratios %s, R %d, layer %d: %.3g of the float32 gates differ from float64" % (ratios, rows, t, frac))
        assert frac <= 1e-4
        if ratios[l] == 0:
            assert np.array_equal(r64["a%d" % t], np.maximum(r64["pre%d" % t], 0))
            assert np.array_equal(r64["d_pre%d" % t] != 0, (r64["d_pre%d" % t] != 0) & (r64["pre%d" % t] > 0))
    junk = dict(masks)
    junk.update({t: np.zeros_like(r64["pre%d" % t], dtype=np.uint8) for t, l, _ in LAYERS if ratios[l] == 0})
    again = R.step(head, pool, blobs, junk, ratios=ratios, want_dpool=False)
    assert all(np.array_equal(again["grads"][k], r64["grads"][k]) for k in R.KEYS)
    assert np.all(r64["losses"] > 0) and all(np.abs(r64["grads"][k]).max() > 0 for k in R.KEYS)
    lr, dc = E.hyper_multipliers()
    assert lr["Was"] == float(np.float32(0.1)) and lr["W71"] == lr["b71"] == 0 and lr["bz"] == 3 and dc["b6"] == 1 and dc["W72"] == 0
    zeros = {k: np.zeros_like(v) for k, v in head.items()}
    for dt in (np.float32, np.float64):
        p, h = R.sgd(head, r64["grads"], zeros, 0.001, 0.9, 0.0005, 0.5, dtype=dt, lr_mult=lr, decay_mult=dc)
        p, h = R.sgd(p, r64["grads"], h, 0.001, 0.9, 0.0005, 1.0, dtype=dt, lr_mult=lr, decay_mult=dc)
        for k in ("W71", "b71"):
            assert np.array_equal(p[k], head[k]) and not h[k].any()
        assert all(not np.array_equal(p[k], head[k]) for k in R.KEYS if k not in ("W71", "b71"))
    # decay on b6 (and none on W72) is visible against the default multipliers
    q, _ = R.sgd(head, r64["grads"], zeros, 0.001, 0.9, 0.0005, 0.5)
    p, _ = R.sgd(head, r64["grads"], zeros, 0.001, 0.9, 0.0005, 0.5, lr_mult=lr, decay_mult=dc)
    assert not np.array_equal(p["b6"], q["b6"]) and not np.array_equal(p["W72"], q["W72"]) and np.array_equal(p["W6"], q["W6"])


def test_front_door_rows_and_trajectory(tmp_path):
    from detect import prototxt as P
    R.traj_solver_files(str(tmp_path), True, E.front_door_rows)
    net = P.read_train_net(str(tmp_path / "train_shared.prototxt"))
    assert [net[k]["dropout_ratio"] for k in ("int6", "int7_1", "int7_2")] == [0.3, None, 0.6]
    assert net["int7_1"]["lr_mult"] == [0.0, 0.0] and net["int6"]["lr_mult"] == [1.0, 2.0] and net["int7_2"]["lr_mult"] == [1.0, 2.0]
    assert all(net[k]["lr_mult"] == [0.0, 0.0] for k in P.CONV_LAYERS)
    # RefTrajectory carries the ratios and the multipliers
    head, fmap, blobs = R.small_case(R=12)
    lr, dc = E.front_door_multipliers()
    ref = R.RefTrajectory(head, np.float64, ratios=E.FRONT_DOOR["ratios"], lr_mult=lr, decay_mult=dc)
    base = R.RefTrajectory(head, np.float64)
    for _ in range(2):
        r, b = ref.step(fmap, blobs, 3), base.step(fmap, blobs, 3)
    assert np.array_equal(r["a71"], np.maximum(r["pre71"], 0)) and not np.array_equal(b["a71"], np.maximum(b["pre71"], 0))
    assert np.array_equal(ref.p["W71"], head["W71"]) and np.array_equal(ref.p["b71"], head["b71"]) and ref.it == 2
    assert all(not np.array_equal(ref.p[k], head[k]) for k in R.KEYS if k not in ("W71", "b71"))
    assert not np.array_equal(base.p["W71"], head["W71"])


def test_hostile_rois_are_hostile():
    rois = E.hostile_rois()
    assert rois.shape == (43, 5) and np.any(np.diff(rois[:, 0]) < 0) and set(rois[:, 0]) == {0.0, 1.0, 2.0}
    assert np.abs(rois[:, 1:]).max() == 1e8 and np.all(np.isfinite(rois))
    shape = (E.MAP["N"], E.MAP["C"], E.MAP["H"], E.MAP["W"])
    for kind in E.MAP_KINDS:
        fmap = E.hostile_map(kind)
        assert fmap.shape == shape and fmap.dtype == np.float32
        empty, windows, tied = E.roi_pool_stats(fmap, rois)
        print("%s map: %.1f %% of the bins empty, %d of %d non-empty (bin, channel) windows hold their maximum more than once"
              % (kind, 100 * empty, tied, windows))
        assert empty >= 0.15
        if kind == "plateau":
            assert tied >= 0.25 * windows and set(np.unique(fmap)) == {0.0, 1.0, 2.0, 3.0} and np.mean(fmap == 0) > 0.4
        if kind == "negative":
            assert fmap.max() == -1 and fmap.min() == -4
        pool, arg = R.roi_pool(fmap, rois)
        assert np.array_equal(arg < 0, np.repeat((arg.reshape(43, -1, 49)[:, :1] < 0), shape[1], axis=1).reshape(43, -1))
        assert not pool[arg < 0].any() and abs(np.mean(arg < 0) - empty) < 1e-12
        if kind == "negative":
            assert np.all(pool[arg >= 0] < 0)                       # a maximum below the 0 of an empty bin
        flat = fmap.reshape(shape[0], shape[1], -1)
        am = arg.reshape(43, shape[1], 49)
        for r in range(43):                                          # the arg-max is the FIRST maximum of its window
            n = int(rois[r, 0])
            for c in range(shape[1]):
                ok = am[r, c] >= 0
                assert np.array_equal(flat[n, c][am[r, c][ok]], pool.reshape(43, shape[1], 49)[r, c][ok])
        # one cell is the arg-max of several bins of one roi
        assert max(np.unique(am[r, 0][am[r, 0] >= 0], return_counts=True)[1].max() for r in range(10, 38)) >= 2
        # np.add.at adds in the order the backward kernel documents (rows ascending, bins ascending), to the bit
        dp = np.random.Generator(np.random.PCG64(2)).standard_normal(pool.shape).astype(np.float32)
        a, b = R.roi_pool_backward(dp, arg, rois, shape), E.roi_pool_backward_loop(dp, arg, rois, shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        outside = ~E.window_cover(rois, shape)
        assert outside.any() and not a.transpose(0, 2, 3, 1)[outside].any()
    # reversed rows: the same rows, the blobs permuted with them
    _, _, fwd = E.roi_case("plateau")
    _, _, rev = E.roi_case("plateau", reverse=True)
    assert all(np.array_equal(rev[k], fwd[k][::-1]) for k in fwd) and not np.array_equal(rev["rois"], fwd["rois"])


def test_gemm_cases_are_exact_in_float32():
    cases = [(f, M, N, K) for M, N in E.GEMM_MN for K in E.GEMM_K for f in (0, 1, 2)] + [(f,) + E.GEMM_BIG for f in (0, 1)]
    assert len(cases) == 7 * 6 * 3 + 2
    worst = 0.0
    for f, M, N, K in cases:
        worst = max(worst, 64.0 * K)                                 # |a|, |b| <= 8: sum |a||b| <= 64 K whatever the draw
    assert worst < 2.0 ** 24
    rng = np.random.Generator(np.random.PCG64(1))
    for f in (0, 1, 2):
        a, b, want = E.gemm_operands(f, 129, 257, 513, E.integer_draw(rng))
        assert want.shape == (129, 257) and E.gemm_abs_sum(f, a, b) <= 64.0 * 513 and np.abs(a).max() == 8
        cpu = {0: lambda: a @ b.T, 1: lambda: a @ b, 2: lambda: a.T @ b}[f]()
        assert np.array_equal(cpu, want.astype(np.float32))


def test_smooth_l1_case_lands_where_it_should():
    head, fmap, blobs, x = E.loss_case()
    w, t = blobs["adj_loss_weights"], blobs["adj_targets"]
    assert not head["Wab"].any() and np.array_equal(head["bab"], x) and set(np.unique(w)) == set(np.float32(E.LOSS_WEIGHTS))
    d = E.smooth_l1_landing(x, t, w)
    assert E.ONE_DOWN < 1 < E.ONE_UP and np.float32(E.ONE_DOWN) == E.ONE_DOWN and np.float32(E.ONE_UP) == E.ONE_UP
    for wv in E.LOSS_WEIGHTS[1:]:
        hits = [int(np.sum((w == wv) & (d == np.float32(v)))) for v in E.LOSS_D]
        print("weight %g: elements on %s: %s" % (wv, E.LOSS_D, hits))
        assert min(hits) >= 20
    assert not d[w == 0].any() and np.abs(t[w == 0]).max() > 1
    # |d| < 1 decides between d and sign d: the floats next to 1 fall on both sides, and at |d| = 1 sign d is d.  The
    # kernel multiplies by a float32 1 / num where the restatement divides by num: w g is a power of two or (1 - 2^-24)
    # times one here, for which the two round alike, so the gradient can be compared bit for bit
    pred = np.broadcast_to(x, t.shape).astype(np.float32)
    _, g = R.smooth_l1(pred, t, w, np.float32(37))
    want = w * np.where(np.abs(d) < 1, d, np.sign(d)).astype(np.float32) * (np.float32(1) / np.float32(37))
    assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), want.view(np.uint32))
    l64, g64 = R.smooth_l1(pred.astype(np.float64), t.astype(np.float64), w.astype(np.float64), 37.0)
    assert np.allclose(g, g64, rtol=1e-6, atol=0) and l64 > 0
