"""GPU: the training data layer's kernels (csrc/az_train.hip) at their loop, buffer and configuration edges.  The cases are
built in tests/train_edges_ref.py; tests/test_train_edges_host.py asserts on the CPU that each reaches what it is meant to
reach and that tests/train_ref.py gives the REFERENCE's bits for it (tests/golden/g23_train_roidb_edges.npz).

  A  levels larger than the chain kernel's 1024 threads: several passes over parents, zoomed regions, children, one parent's
     children and the super-regions; the fullest level that fits and the clean errors past it (4096 children, the hash range)
  B  az_train_params off its defaults; image sizes at the MIN_SIDE edges; images without example regions
  C  the S x N match matrix beyond one wave and beyond 64 KB of LDS, up to the 128 KB limit and the clean error past it
  D  az_train_target_stats at every n_sub and chunk edge: exact rows bit for bit, rows of no class, random rows within bounds
  E  az_data_layer.roidb over the device on the overflowing image and on a mixed imdb

Bounds: those of tests/test_gpu_train.py, unchanged (tests/train_edges_ref.py restates them): everything bit for bit except
dw / dh at 4 ulp (f64); means / stds of random rows within check_stats' bounds; where the reference yields a nan the device
yields one in the same place.  Compared with g23 where it records arrays, element by element with train_ref elsewhere (the
host twin ties train_ref to the reference's SHA-256s), and the device's own arrays are hashed against g23 too."""
import os

import numpy as np
import pytest

import train_edges_ref as E
import train_ref as tr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G23 = os.path.join(HERE, "golden", "g23_train_roidb_edges.npz")
G20 = os.path.join(HERE, "golden", "g20_train_roidb.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(G23)


@pytest.fixture(scope="module")
def g20():
    return np.load(G20)


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def levels():
    """train_ref on the cases of group A that the device answers, once -> name: (boxes f64, labels, used, level summary)."""
    out = {}
    for name, case in E.LEVEL_CASES.items():
        if case[4] == "ok":
            st = {}
            b, z, u = E.run_level_case(name, st)
            out[name] = (b, z, u, E.level_summary(st))
    return out


def still_good(ctx, g20):
    """The context after an error: golden case c0 of g20, bit for bit."""
    size = tuple(int(v) for v in g20["c0_size"])
    np.random.seed(int(g20["c0_seed"]))
    noise = np.random.random(int(g20["c0_used"]) + 7)
    ex, zoom, off, used = ctx.train_ex_rois(E.tp_of({}), [size], [g20["c0_gt"]], noise)
    assert int(used[0]) == int(g20["c0_used"]) and off.tolist() == [0, ex.shape[0]]
    assert np.array_equal(ex, g20["c0_ex_boxes"].astype(np.float32)) and np.array_equal(zoom.astype(bool), g20["c0_zoom_gt"])
    t, toff = ctx.train_adj_targets(E.tp_of({}), ex, off, [g20["c0_gt"].astype(np.float32)])
    E.check_targets(t, g20["c0_targets"], "c0 after an error")


def clean_error(ctx, code, call):
    from aznet_hip import ffi
    with pytest.raises(ffi.AzError) as e:
        call()
    assert e.value.code == code, e.value
    assert not hasattr(e.value, "needed") and not hasattr(e.value, "needed_cap")       # needed_out both zero
    return e.value


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in E.LEVEL_CASES.items() if c[4] == "ok"))
def test_large_levels(ctx, g, levels, name):
    size, gt, seed, kw, _ = E.LEVEL_CASES[name]
    b, z, u, s = levels[name]
    tp = E.tp_of(kw)
    ex, zoom, off, used = ctx.train_ex_rois(tp, [size], [gt], E.noise_of(seed, u + 3))
    assert int(used[0]) == u == int(g["L_%s_used" % name]) and off.tolist() == [0, b.shape[0]]
    assert np.array_equal(ex, b.astype(np.float32)) and np.array_equal(zoom.astype(bool), z)
    assert E.sha(ex) == str(g["L_%s_sha_ex32" % name]) and E.sha(zoom.astype(bool)) == str(g["L_%s_sha_zoom" % name])
    ex1, _, _, _ = ctx.train_ex_rois(tp, [size], [gt], E.noise_of(seed, u), cap=b.shape[0])     # exactly enough of both
    assert np.array_equal(ex1, ex)
    t, toff = ctx.train_adj_targets(tp, ex, off, [gt.astype(np.float32)])
    ref = tr.compute_targets(gt, ex, E.cfg_of(kw))
    assert ref.shape[0] == int(g["L_%s_T" % name])
    worst = E.check_targets(t, ref, name)
    print("%s: largest P %d, PZ %d, CH %d, children of one parent %d, N * S %d; E %d, doubles %d, T %d, dw / dh %.2f ulp"
          % (name, s["max_P"], s["max_PZ"], s["max_CH"], s["max_parent"], gt.shape[0] * len(tp["subregion"]), ex.shape[0], u,
             t.shape[0], worst))


@pytest.mark.parametrize("name", sorted(n for n, c in E.LEVEL_CASES.items() if c[4] != "ok"))
def test_levels_past_a_limit_are_clean_errors(ctx, g20, name):
    """A level past 4096 children is AZ_ERR_CAPACITY, a dedup key outside [0, 2^40) AZ_ERR_INVALID: argument checks the kernel
    makes itself with a workgroup-uniform return.  The context then gives c0's bits."""
    from aznet_hip import ffi
    size, gt, seed, kw, answer = E.LEVEL_CASES[name]
    code = ffi.AZ_ERR_CAPACITY if answer == "capacity" else ffi.AZ_ERR_INVALID
    e = clean_error(ctx, code, lambda: ctx.train_ex_rois(E.tp_of(kw), [size], [gt], E.noise_of(seed, 20000)))
    print("%s: %s" % (name, e))
    still_good(ctx, g20)


def test_large_images_share_one_stream(ctx, g):
    S = E.SHARED_STREAM
    tp, c = E.tp_of(S["kw"]), E.cfg_of(S["kw"])
    sizes, gts = [a for a, _ in S["images"]], [b for _, b in S["images"]]
    n = len(sizes)
    total = sum(int(g["S%d_used" % i]) for i in range(n))
    noise = E.noise_of(S["seed"], total + 1)
    ex, zoom, off, used = ctx.train_ex_rois(tp, sizes, gts, noise)
    assert used.tolist() == [int(g["S%d_used" % i]) for i in range(n)]
    assert np.diff(off).tolist() == [int(g["S%d_E" % i]) for i in range(n)]
    at = 0
    for j in range(n):
        e1, z1, o1, u1 = ctx.train_ex_rois(tp, [sizes[j]], [gts[j]], noise[at:])
        assert int(u1[0]) == int(used[j])
        assert np.array_equal(e1, ex[off[j]:off[j + 1]]) and np.array_equal(z1, zoom[off[j]:off[j + 1]])
        b, z, u = tr.compute_ex_rois(sizes[j], gts[j], noise[at:], c)
        assert u == int(used[j]) and np.array_equal(b.astype(np.float32), e1) and np.array_equal(z, z1.astype(bool))
        assert E.sha(e1) == str(g["S%d_sha_ex32" % j]) and E.sha(z1.astype(bool)) == str(g["S%d_sha_zoom" % j])
        at += u
    t, toff = ctx.train_adj_targets(tp, ex, off, [b.astype(np.float32) for b in gts])
    for j in range(n):
        E.check_targets(t[toff[j]:toff[j + 1]], tr.compute_targets(gts[j], ex[off[j]:off[j + 1]], c), "image %d" % j)
    assert toff[3] == toff[2]                                                       # the image without example regions


# ---- B ---------------------------------------------------------------------------------------------------------------------------
def test_params_off_their_defaults(ctx, g):
    worst = 0.0
    for name, size, gt, seed, kw in E.param_cases():
        tp = E.tp_of(kw)
        used = int(g["B_%s_used" % name])
        ex, zoom, off, u = ctx.train_ex_rois(tp, [size], [gt], E.noise_of(seed, used))
        assert int(u[0]) == used, name
        assert np.array_equal(ex, g["B_%s_ex_boxes" % name].astype(np.float32)), name
        assert np.array_equal(zoom.astype(bool), g["B_%s_zoom_gt" % name]) and off.tolist() == [0, ex.shape[0]], name
        t, toff = ctx.train_adj_targets(tp, ex, off, [gt.astype(np.float32)])
        assert toff.tolist() == [0, g["B_%s_targets" % name].shape[0]], name
        worst = max(worst, E.check_targets(t, g["B_%s_targets" % name], name))
    print("%d parameter cases; max |dw, dh| difference to the reference: %.2f ulp" % (len(E.param_cases()), worst))


def test_images_without_example_regions(ctx, g):
    B = E.EMPTY_BATCH
    tp = E.tp_of(B["kw"])
    ims = E.empty_batch_images()
    n = len(ims)
    total = sum(int(g["BE%d_used" % i]) for i in range(n))
    ex, zoom, off, used = ctx.train_ex_rois(tp, [a for a, _ in ims], [b for _, b in ims], E.noise_of(B["seed"], total))
    assert used.tolist() == [int(g["BE%d_used" % i]) for i in range(n)]
    assert off[0] == off[1] and off[2] == off[3] and off[4] == off[5] == ex.shape[0]
    t, toff = ctx.train_adj_targets(tp, ex, off, [b.astype(np.float32) for _, b in ims])
    for i in range(n):
        assert np.array_equal(ex[off[i]:off[i + 1]], g["BE%d_ex_boxes" % i].astype(np.float32)), i
        assert np.array_equal(zoom[off[i]:off[i + 1]].astype(bool), g["BE%d_zoom_gt" % i]), i
        E.check_targets(t[toff[i]:toff[i + 1]], g["BE%d_targets" % i], "image %d" % i)
    # nothing but empty images, and no image at all
    ex0, _, off0, used0 = ctx.train_ex_rois(tp, [ims[0][0]] * 3, [ims[0][1]] * 3, np.zeros(0))
    assert ex0.shape == (0, 4) and off0.tolist() == [0, 0, 0, 0] and used0.tolist() == [0, 0, 0]
    t0, toff0 = ctx.train_adj_targets(tp, ex0, off0, [ims[0][1].astype(np.float32)] * 3)
    assert t0.shape == (0, 7) and toff0.tolist() == [0, 0, 0, 0]


# ---- C ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S", E.MATCH_SIZES)
def test_match_matrix(ctx, N, S):
    from aznet_hip import ffi
    ex, gt, twins = E.match_case(N, S)
    K = ex.shape[0]
    for adj in (0.1, 0.0):
        kw = E.match_kw(S, adj)
        ref = tr.compute_targets(gt, ex, E.cfg_of(kw))
        t, toff = ctx.train_adj_targets(E.tp_of(kw), ex, [0, K], [gt])
        assert toff.tolist() == [0, ref.shape[0]]
        worst = E.check_targets(t, ref, "N=%d S=%d adj_thresh=%g" % (N, S, adj))
        print("N=%d S=%d adj_thresh=%g: %d regions, N * S %d, LDS %d bytes, T %d, dw / dh %.2f ulp"
              % (N, S, adj, K, N * S, N * S * 8, t.shape[0], worst))
    if N * S * 8 > 65536:                                                           # the cap edge at a large N
        T = ref.shape[0]
        t1, _ = ctx.train_adj_targets(E.tp_of(kw), ex, [0, K], [gt], cap=T)
        assert np.array_equal(t1, t)
        with pytest.raises(ffi.AzError) as e:
            ctx.train_adj_targets(E.tp_of(kw), ex, [0, K], [gt], cap=T - 1)
        assert e.value.code == ffi.AZ_ERR_CAPACITY and e.value.needed_cap == T


@pytest.mark.parametrize("N,S", E.MATCH_OVER)
def test_match_matrix_past_its_lds_is_a_clean_error(ctx, g20, N, S):
    from aznet_hip import ffi
    ex, gt, _ = E.match_case(N, S)
    clean_error(ctx, ffi.AZ_ERR_CAPACITY,
                lambda: ctx.train_adj_targets(E.tp_of(E.match_kw(S)), ex, [0, ex.shape[0]], [gt]))
    still_good(ctx, g20)


# ---- D ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sub", E.STATS_NSUB)
def test_target_stats_exact_rows(ctx, n_sub):
    """Rows whose sums are exact in any order, eps 0: the device's means, stds and normalised rows are NumPy's bit for bit, nan
    included (an absent class, a class of one row, a class of identical rows); rows of no class are not touched."""
    for T in E.STATS_T:
        raw = E.stats_exact_rows(n_sub, T, 7 * n_sub + T)
        m_ref, s_ref, t_ref = E.stats_reference(raw, n_sub, 0.0)
        t = raw.copy()
        m, s = ctx.train_target_stats(n_sub, 0.0, t, True)
        what = "n_sub=%d T=%d" % (n_sub, T)
        assert np.array_equal(np.isnan(m), np.isnan(m_ref)) and np.array_equal(np.isnan(s), np.isnan(s_ref)), what
        assert np.array_equal(m, m_ref, equal_nan=True) and np.array_equal(s, s_ref, equal_nan=True), what
        assert np.array_equal(np.isnan(t), np.isnan(t_ref)) and np.array_equal(t, t_ref, equal_nan=True), what
        inside = (raw[:, 5] >= 0) & (raw[:, 5] < n_sub) & (raw[:, 5] == np.floor(raw[:, 5]))
        assert t[~inside].tobytes() == raw[~inside].tobytes(), what
        t2 = raw.copy()
        m2, s2 = ctx.train_target_stats(n_sub, 0.0, t2, False)
        assert t2.tobytes() == raw.tobytes() and m2.tobytes() == m.tobytes() and s2.tobytes() == s.tobytes(), what
    print("n_sub=%d: T in %s bit for bit" % (n_sub, E.STATS_T))


@pytest.mark.parametrize("n_sub", E.STATS_NSUB)
def test_target_stats_random_rows(ctx, n_sub):
    for T in (4097, 3 * 4096 + 1):
        raw = E.stats_random_rows(n_sub, T, 31 * n_sub + T)
        m_ref, s_ref, t_ref = E.stats_reference(raw, n_sub, 1e-14)
        t = raw.copy()
        m, s = ctx.train_target_stats(n_sub, 1e-14, t, True)
        E.check_stats(m, s, t, m_ref, s_ref, raw, t_ref)
        t2 = raw.copy()
        m2, s2 = ctx.train_target_stats(n_sub, 1e-14, t2, True)
        assert t2.tobytes() == t.tobytes() and m2.tobytes() == m.tobytes() and s2.tobytes() == s.tobytes()


def test_target_stats_refuses_n_sub_past_16(ctx):
    from aznet_hip import ffi
    for n_sub in (0, 17):
        with pytest.raises(ffi.AzError) as e:
            ctx.train_target_stats(n_sub, 1e-14, np.zeros((4, 7)), True)
        assert e.value.code == ffi.AZ_ERR_INVALID


# ---- E ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def rdl(ctx):
    from az_data_layer import roidb as m
    from aznet_hip import ffi
    m.set_backend(None)
    ffi.set_default_context(ctx)
    return m


def test_host_layer_surfaces_the_level_overflow(rdl, ctx, g20):
    E.host_overflow(rdl)
    still_good(ctx, g20)


def test_host_layer_on_mixed_images(rdl, monkeypatch):
    roidb, state, means, stds = E.host_mixed(rdl, monkeypatch)
    E.check_mixed(roidb, state, means, stds, in_err_ulps=4)
    rdl.set_backend(tr.RefBackend())
    try:
        roidb2, state2, _, _ = E.host_mixed(rdl, monkeypatch)
    finally:
        rdl.set_backend(None)
    assert np.array_equal(state[1], state2[1]) and state[2] == state2[2]
    for a, b in zip(roidb, roidb2):
        for k in ("ex_boxes", "zoom_gt", "gt_boxes"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])
        assert np.array_equal(a["bbox_targets"][:, 4:], b["bbox_targets"][:, 4:])
