"""GPU: az_head_forward and az_det_forward at layer sizes other than the reduced and the full one (tests/head_sizes_ref.py).

AZ head sizes (C, n6, n71, n72) and what each is for (K6 = 49 C; azk_fc_split(K) = 1 / 2 / 8 / 16 chunks from K = 512 / 2048 /
16384; n-tiles of 128 columns, K steps of 32):
  (4, 4, 4, 4)             every minimum; K < 32 in int7; n7 = 8
  (12, 132, 68, 36)        split 2 in int6 with a short last slab (K6 = 588); a 4-column n-tile; ragged K in int7
  (44, 260, 132, 4)        split 8 in int6 (K6 = 2156); the int7_1 / int7_2 seam past column 128
  (336, 36, 8, 8)          split 16 in int6, K6 = 16464: not a multiple of 32, ragged last slab
  (4, 516, 3000, 72)       split 2 in int7; n7 = 3072, the tail kernel's LDS limit
  (4, 2052, 8, 4)          split 8 in int7 with a ragged K
  (4, 16388, 4, 4)         split 16 in int7
  (44, 8324, 8, 4)         66 n-tiles x 8 chunks = 528 work items for the 512 workgroups of k_fc_splitk
  (256, 4096, 1024, 256)   a second shape of the many-row GEMM (az_head12.hip: split 8, chunks of 1568); GEMM mode 0 only,
                           161 and 300 rows only
Detection head sizes (C, n6, n7, ncls): (4, 4, 4, 2), (12, 132, 100, 21), (44, 260, 516, 81), (4, 2052, 2052, 256).

Every other size runs in GEMM modes 0, 2 and 3 (az_set_gemm_mode; the detection head's fc6 takes the 16-bit-term path when an
AZ head of the same C is loaded in that mode, which these tests do).  Contexts have max_regions = 512; the row counts are
prefixes of ONE 300-roi set: 1, 8, 16, 33, 40, 48, 130, 161, 300.

Integer-exact heads: box outputs and the trainer's raw scores bit for bit, probabilities within train_step_ref.bound of the
float32 restatement's error against the float64 sigmoid / softmax of the exact pre-activation.  Random heads: per output
tensor max |got - f64| / max |f64| within 8 x the same figure of the oracle's float32 head (floor 1e-6), the rule of
tests/test_gpu_train_step.py.  Every figure is printed before it is asserted (run with -s for the table)."""
import functools

import numpy as np
import pytest

import head_sizes_ref as H
import train_step_ref as R

pytestmark = pytest.mark.gpu
MODES = (0, 2, 3)


def _id(d):
    return "x".join(str(v) for v in d)


def _modes(dims):
    return (0,) if dims == H.AZ_LARGEST else MODES


def _rows(dims):
    return (161, 300) if dims == H.AZ_LARGEST else H.ROWS


@pytest.fixture(scope="module")
def env():
    from aznet_hip import ffi
    from oracle import az_oracle as orc
    ctxs = {m: ffi.AzContext(0, max_regions=512, gemm_mode=m) for m in MODES}
    yield ffi, orc, ctxs
    for c in ctxs.values():
        c.close()


def _pool(fmap, rois):
    from oracle import az_oracle as orc
    return orc.roi_pool(fmap[0], rois)


@functools.lru_cache(maxsize=None)
def az_int(dims):
    return H.int_az_case(dims, pool=_pool)


@functools.lru_cache(maxsize=None)
def det_int(dims):
    return H.int_det_case(dims, pool=_pool)


@functools.lru_cache(maxsize=None)
def az_rand(dims):
    """The random case with its float64 and float32-CPU evaluations (the largest is built once, here)."""
    from oracle import az_oracle as orc
    c = H.random_az_case(dims)
    c["r64"] = H.f64_head(orc, c["head"], c["fmap"], c["rois"])
    c["r32"] = orc.head_forward(c["head"], c["fmap"][0], c["rois"])
    return c


@functools.lru_cache(maxsize=None)
def det_rand(dims):
    from oracle import az_oracle as orc
    c = H.random_det_case(dims)
    c["r64"] = H.f64_det_head(orc, c["head"], c["fmap"], c["rois"])
    c["r32"] = orc.det_head_forward(c["head"], c["fmap"][0], c["rois"])
    return c


def _tiny_az_head(C):
    """An AZ head of the detection head's C (the two heads of a context share C and the pooled rows)."""
    return az_int((C, 4, 4, 4))["head"]


def check(tag, got, r64, r32):
    e_dev, e_cpu = R.rel_err(got, r64), R.rel_err(r32, r64)
    b = R.bound(e_cpu)
    print("  %-34s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (tag, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b


def check_prob(tag, e, tol):
    print("  %-34s device %.3e   bound %.3e   %s" % (tag, e, tol, "ok" if e <= tol else "EXCEEDS"))
    return e <= tol


# ---- RoIPool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", H.AZ_SIZES, ids=_id)
def test_roi_pool_bit_for_bit(env, dims):
    """C = 4, 12, 44, 336, 256 at 40 and 130 rois (both sides of ROI_POOL_COOP_MAX), an integer and a random map -- at every
    size set, not every C: az_roi_pool returns its rows through the split-K slab buffer, whose size the other layers set."""
    ffi, orc, ctxs = env
    ctx = ctxs[0]
    ctx.load_head(az_int(dims)["head"])
    for fmap in (az_int(dims)["fmap"], az_rand(dims)["fmap"]):
        ctx.set_feature_map(fmap)
        rois = H.rois300()
        for n in (40, 130):
            assert np.array_equal(ctx.roi_pool(rois[:n]), orc.roi_pool(fmap[0], rois[:n])), n


# ---- the AZ head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", H.AZ_SIZES, ids=_id)
def test_az_integer_head(env, dims):
    ffi, orc, ctxs = env
    import torch
    c = az_int(dims)
    rois, ok = c["rois"], True
    print("integer AZ head %s: k = %d, score non-zeros %s" % (dims, c["k"], c["nnz"]))
    for m in _modes(dims):
        ctx = ctxs[m]
        ctx.load_head(c["head"])
        ctx.set_feature_map(c["fmap"])
        ref, worst = ctx.head_forward(rois), {}
        for n in _rows(dims):
            z, a, d = ctx.head_forward(rois[:n])
            assert np.array_equal(d, c["bbox"][:n]), "adj_bbox, mode %d, %d rows" % (m, n)
            for x, y in zip((z, a, d), ref):
                assert np.array_equal(x, y[:n]), "prefix of the 300-row launch, mode %d, %d rows" % (m, n)
            worst = {k: max(worst.get(k, 0.0), R.rel_err(g, c["p64"][k][:n])) for k, g in (("zoom", z), ("adj", a))}
        for k in ("zoom", "adj"):                                        # (the worst row count)
            ok &= check_prob("%s_prob mode %d" % (k, m), worst[k], c["tol"][k])
    # the trainer's TEST-phase forward: a second device implementation of the same layers
    sol = ffi.AzSolver(ctxs[0], *dims, max_rois=300, head=c["head"])
    try:
        z, a, b = sol.forward_test(torch.from_numpy(c["fmap"]).cuda(), rois)
    finally:
        sol.close()
    assert np.array_equal(b, c["bbox"]), "trainer adj_bbox"
    assert np.array_equal(a, c["pre"]["adj"].astype(np.float32)), "trainer adj_score"
    assert np.array_equal(z.reshape(-1, 1), c["pre"]["zoom"].astype(np.float32)), "trainer zoom_score"
    assert ok, "a probability exceeds 8 x the float32 restatement's error"


@pytest.mark.parametrize("dims", H.AZ_SIZES, ids=_id)
def test_az_random_head(env, dims):
    ffi, orc, ctxs = env
    c = az_rand(dims)
    rois, ok = c["rois"], True
    print("random AZ head %s" % (dims,))
    for m in _modes(dims):
        ctx = ctxs[m]
        ctx.load_head(c["head"])
        ctx.set_feature_map(c["fmap"])
        ref = ctx.head_forward(rois)
        for name, got, r64, r32 in zip(("zoom_prob", "adj_prob", "adj_bbox"), ref, c["r64"], c["r32"]):
            ok &= check("%s mode %d" % (name, m), got, r64, r32)
        for n in _rows(dims):
            for x, y in zip(ctx.head_forward(rois[:n]), ref):
                assert np.array_equal(x, y[:n]), "prefix of the 300-row launch, mode %d, %d rows" % (m, n)
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


# ---- the detection head -------------------------------------------------------------------------------------------------------
def _load_det(ctx, c):
    ctx.load_head(_tiny_az_head(c["dims"][0]))
    ctx.load_det_head(c["head"])
    ctx.set_feature_map(c["fmap"])


@pytest.mark.parametrize("dims", H.DET_SIZES, ids=_id)
def test_det_integer_head(env, dims):
    ffi, orc, ctxs = env
    c = det_int(dims)
    rois, ok = c["rois"], True
    print("integer detection head %s: k = %d, score non-zeros %s" % (dims, c["k"], c["nnz"]))
    for m in MODES:
        ctx = ctxs[m]
        _load_det(ctx, c)
        ref, worst = ctx.det_forward(rois), 0.0
        for n in H.ROWS:
            p, b = ctx.det_forward(rois[:n])
            assert np.array_equal(b, c["bbox"][:n]), "bbox_pred, mode %d, %d rows" % (m, n)
            assert np.array_equal(p, ref[0][:n]) and np.array_equal(b, ref[1][:n]), "prefix, mode %d, %d rows" % (m, n)
            worst = max(worst, R.rel_err(p, c["p64"]["cls"][:n]))
        ok &= check_prob("cls_prob mode %d" % m, worst, c["tol"]["cls"])      # (the worst row count)
    assert ok, "a probability exceeds 8 x the float32 restatement's error"


@pytest.mark.parametrize("dims", H.DET_SIZES, ids=_id)
def test_det_random_head(env, dims):
    ffi, orc, ctxs = env
    c = det_rand(dims)
    rois, ok = c["rois"], True
    print("random detection head %s" % (dims,))
    for m in MODES:
        ctx = ctxs[m]
        _load_det(ctx, c)
        ref = ctx.det_forward(rois)
        for name, got, r64, r32 in zip(("cls_prob", "bbox_pred"), ref, c["r64"], c["r32"]):
            ok &= check("%s mode %d" % (name, m), got, r64, r32)
        for n in H.ROWS:
            for x, y in zip(ctx.det_forward(rois[:n]), ref):
                assert np.array_equal(x, y[:n]), "prefix of the 300-row launch, mode %d, %d rows" % (m, n)
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


# ---- whole searches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(12, 132, 68, 36), (44, 260, 132, 4)], ids=_id)
def test_search(env, dims):
    """A 375 x 500 image at Tz = 0 and at a positive Tz: the default path against the plain level loop and against the oracle's
    loop driven by the HIP head, bit for bit."""
    ffi, orc, ctxs = env
    from aznet_hip.net import HipAZNet
    from test_gpu_parity import _oracle_loop_on_gpu_head
    c = H.random_az_case(dims)
    fmap, (Hi, Wi) = c["fmap"], (375, 500)
    for m in MODES:
        net = HipAZNet(c["head"], name="sizes%d" % m, ctx=ctxs[m])
        net.set_conv(fmap)

        class Injected(object):      # pycaffe-shaped view of the HIP head
            name = "inj"
            blobs = net.blobs

            def forward(self, blobs=None, **kw):
                kw.pop("data", None)
                kw["conv5_3"] = fmap
                return net.forward(blobs=blobs, **kw)

        _, tr0 = _oracle_loop_on_gpu_head(orc, Injected(), fmap, Hi, Wi, 1.0, orc.OracleCfg(Tz=0.0))
        zs = np.unique(np.concatenate([lv["zoom"] for lv in tr0["levels"][1:]]))
        Tz_pos = 0.5 * (float(zs[len(zs) // 2]) + float(zs[len(zs) // 2 + 1]))
        for Tz in (0.0, Tz_pos):
            tr = tr0 if Tz == 0.0 else _oracle_loop_on_gpu_head(orc, Injected(), fmap, Hi, Wi, 1.0, orc.OracleCfg(Tz=Tz))[1]
            outs = []
            for plain in (False, True):
                kw = dict(speculate=False, fused=False, fused_levels=False, static_tree=False, pair_spec=False, full_spec=False,
                          early_end=False) if plain else {}
                Y, S, st = net.propose(ffi.AzContext.make_params(Hi, Wi, 1.0, Tz, **kw), want_scores=True, want_stats=True)
                Ya, Sa = net.ctx.last_candidates()
                outs.append((Y, S, Ya, Sa, st.depth, st.num_eval, list(st.level_regions), list(st.level_unique), list(st.level_zoomed)))
            for a, b in zip(*outs):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, (m, Tz)
            Y, S, Ya, Sa, depth, num_eval, regions, unique, zoomed = outs[0]
            assert depth == tr["depth"] and num_eval == tr["num_eval"]
            assert Tz == 0.0 or num_eval < tr0["num_eval"]                                 # (the positive Tz prunes the tree)
            for l, lev in enumerate(tr["levels"]):
                assert regions[l] == lev["B"].shape[0] and unique[l] == sum(f["U"] for f in lev["fwd"]) and zoomed[l] == len(lev["indZ"])
            assert Ya.shape == tr["Y_all"].shape
            assert np.array_equal(Sa.astype(np.float64), tr["aScores"])
            np.testing.assert_allclose(Ya, tr["Y_all"], rtol=1e-6, atol=1e-4)             # decode: f32-exp ulps (px)
            idx = np.argsort(-tr["aScores"], kind="stable")[:300]
            assert np.array_equal(Y, Ya[idx]) and np.array_equal(S, Sa[idx])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _zero_head(C, n6, n71, n72):
    z = lambda *s: np.zeros(s, np.float32)          # noqa: E731
    return {"W6": z(n6, C * 49), "b6": z(n6), "W71": z(n71, n6), "b71": z(n71), "W72": z(n72, n6), "b72": z(n72),
            "Was": z(11, n71), "bas": z(11), "Wab": z(44, n71), "bab": z(44), "Wz": z(1, n72), "bz": z(1)}


def test_refused_sizes_leave_the_loaded_head_alone(env):
    """n71 + n72 past the tail kernel's LDS tile and a non-multiple of 4 in each of the four sizes: AZ_ERR_INVALID, and the head
    loaded before answers with the same bits.  The same for the detection head's n7 and ncls."""
    ffi, orc, ctxs = env
    c = az_rand((12, 132, 68, 36))
    for m in MODES:
        ctx = ctxs[m]
        ctx.load_head(c["head"])
        ctx.set_feature_map(c["fmap"])
        want = ctx.head_forward(c["rois"][:48])
        for bad in (H.AZ_REFUSED_LDS, (6, 132, 68, 36), (12, 130, 68, 36), (12, 132, 66, 36), (12, 132, 68, 34)):
            with pytest.raises(ffi.AzError) as e:
                ctx.load_head(_zero_head(*bad))
            assert e.value.code == ffi.AZ_ERR_INVALID, bad
            for x, y in zip(ctx.head_forward(c["rois"][:48]), want):
                assert np.array_equal(x, y), bad
    d = det_rand((12, 132, 100, 21))
    ctx = ctxs[0]
    ctx.load_det_head(d["head"])
    ctx.set_feature_map(d["fmap"])
    want = ctx.det_forward(d["rois"][:48])
    z = lambda *s: np.zeros(s, np.float32)          # noqa: E731
    for n7, ncls in ((98, 21), (100, 1), (100, 257)):
        with pytest.raises(ffi.AzError) as e:
            ctx.load_det_head({"W6": z(132, 588), "b6": z(132), "W7": z(n7, 132), "b7": z(n7), "Wc": z(ncls, n7), "bc": z(ncls),
                               "Wb": z(4 * ncls, n7), "bb": z(4 * ncls)})
        assert e.value.code == ffi.AZ_ERR_INVALID, (n7, ncls)
        for x, y in zip(ctx.det_forward(d["rois"][:48]), want):
            assert np.array_equal(x, y), (n7, ncls)
