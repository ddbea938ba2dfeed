"""GPU: final selection and box decoding at their handovers and edges (DESIGN, "Selection edges") -- both top-k
implementations (the chip-wide counting kernels through az_topk up to 65536 scores, the single-workgroup radix select
through az_topk_radix at every size, az_topk itself across the handover and up to the context's capacity), the threshold
selection and the fused gathers through whole searches, and az_decode_filter, against the plain references and on the cases
of tests/select_ref.py (each checked on the CPU by test_select_edges_host.py).  Index vectors, scores and the exact decode
cases compare with np.array_equal; only the decode cases with general log-size deltas use the box tolerance of
test_decode_filter_golden (the f32 exp differs from NumPy's by an ulp)."""
import ctypes

import numpy as np
import pytest

import select_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipAZNet
    return ffi, synth, HipAZNet


@pytest.fixture(scope="module")
def small(mods):
    ffi, synth, HipAZNet = mods
    head = synth.make_head(seed=77, **synth.SMALL_DIMS)
    net = HipAZNet(head, name="small")
    assert net.ctx.max_candidates == S.DEFAULT_MAX_CANDIDATES and net.ctx.max_regions == S.DEFAULT_MAX_REGIONS
    return net, head


# ------------------------------------------------------------------------------------------------------------- top-k
def _topk_both(ctx, s, k, what, want=None):
    """az_topk (counting kernels up to 65536 scores, the radix select above) and az_topk_radix (the radix select alone)
    against the reference -- and so against each other."""
    if want is None:
        want = S.topk_ref(s, k)
    plain = ctx.topk(s, k)
    radix = ctx.topk_radix(s, k)
    assert plain.dtype == np.int32 and np.array_equal(plain, want), ("az_topk",) + what
    assert np.array_equal(radix, want), ("az_topk_radix",) + what


@pytest.mark.parametrize("n", S.topk_sizes())
def test_topk_sizes(small, n):
    """Every size, the three around the handover and the context's capacity among them, at every k (k > n: all n)."""
    ctx = small[0].ctx
    for i, pattern in enumerate(S.SIZE_PATTERNS):
        s = S.topk_scores(pattern, n, 300, 2000 + i)
        ref = S.topk_ref(s, max(S.TOPK_KS))                       # (the reference of a smaller k is its head)
        for k in S.TOPK_KS:
            _topk_both(ctx, s, k, (pattern, n, k), ref[:k])


@pytest.mark.parametrize("pattern", S.TOPK_PATTERNS)
def test_topk_patterns(small, pattern):
    ctx = small[0].ctx
    cases = S.pattern_cases(pattern)
    assert cases
    for n, k, seed in cases:
        _topk_both(ctx, S.topk_scores(pattern, n, k, seed), k, (pattern, n, k))


def test_topk_all_selected_near_the_largest_k(small):
    """ksel == n (everything is selected, no radix pass runs) at and around the largest k."""
    ctx = small[0].ctx
    for n in (4095, 4096):
        for pattern in ("uniform_ties", "all_equal", "negative_inf"):
            s = S.topk_scores(pattern, n, 4096, 31)
            for k in (n, 4096):
                _topk_both(ctx, s, k, (pattern, n, k))
                assert ctx.topk_radix(s, k).shape == (n,)


def test_topk_refusals_leave_the_context_working(small, mods):
    ffi = mods[0]
    ctx = small[0].ctx
    s = S.topk_scores("uniform_ties", ctx.max_candidates + 1, 300, 3)
    for fn in (ctx.topk, ctx.topk_radix):
        with pytest.raises(ffi.AzError) as e:
            fn(s, 300)                                            # one score more than the context holds
        assert e.value.code == ffi.AZ_ERR_CAPACITY
        _topk_both(ctx, s[:-1], 300, ("after n refusal",))
        with pytest.raises(ffi.AzError) as e:
            fn(s[:5000], 4097)
        assert e.value.code == ffi.AZ_ERR_CAPACITY
        with pytest.raises(ffi.AzError) as e:
            fn(s[:5000], 0)
        assert e.value.code == ffi.AZ_ERR_INVALID
        _topk_both(ctx, s[:5000], 4096, ("after k refusal",))
        assert fn(s[:0], 300).shape == (0,)                       # no scores: nothing selected, no error


# ------------------------------------------------------------------------------------------- through a whole search
@pytest.fixture(scope="module")
def searched(small, mods):
    """One 600 x 1000 search on one small map: its candidates (the same for every selection mode)."""
    ffi, synth, HipAZNet = mods
    net = small[0]
    net.set_conv(synth.make_feature_map(5, synth.SMALL_DIMS["C"], 38, 63))
    net.propose(ffi.AzContext.make_params(600, 1000, 1.0, 0.0))
    Yall, Sall = net.ctx.last_candidates()
    assert Sall.shape[0] > 4096 + 1024 and Yall.shape == (Sall.shape[0], 4)
    assert not np.isnan(Sall).any() and (Sall > 0).all()
    return net, Yall, Sall


SELECT_MODES = {"default": {}, "radix_select": dict(radix_select=True),
                "separate_kernels": dict(speculate=False, fused=False, fused_levels=False, static_tree=False, pair_spec=False,
                                         full_spec=False)}


@pytest.mark.parametrize("mode", sorted(SELECT_MODES))
@pytest.mark.parametrize("k", [1, 300, 4096])
def test_search_fixed_count_gathers_the_reference_rows(searched, mods, k, mode):
    """Boxes and scores of a search == its candidates indexed by topk_ref: the fused Yout / Sout gather of the selection
    the search fuses into its last launch, of the radix select, and of the counting kernels (levels as separate launches)."""
    ffi = mods[0]
    net, Yall, Sall = searched
    Y, Sc = net.propose(ffi.AzContext.make_params(600, 1000, 1.0, 0.0, num_proposals=k, **SELECT_MODES[mode]), want_scores=True)
    Ya, Sa = net.ctx.last_candidates()
    assert np.array_equal(Ya, Yall) and np.array_equal(Sa, Sall)
    idx = S.topk_ref(Sall, k)
    assert Y.shape == (k, 4) and np.array_equal(Y, Yall[idx]) and np.array_equal(Sc, Sall[idx])


def _thresh(net, ffi, Tc):
    Y, Sc = net.propose(ffi.AzContext.make_params(600, 1000, 1.0, 0.0, fixed_num=False, Tc=Tc), want_scores=True)
    return Y, Sc


def test_search_threshold_on_a_candidate_score(searched, mods):
    """Tc exactly a candidate's score keeps it (>= in double); one double above drops it and keeps every higher one."""
    ffi = mods[0]
    net, Yall, Sall = searched
    u = np.unique(Sall)
    for sj in (u[0], u[u.shape[0] // 3], u[u.shape[0] // 2], u[-2], u[-1]):
        j = np.where(Sall == sj)[0]
        for Tc, j_in in ((np.float64(sj), True), (np.nextafter(np.float64(sj), np.inf), False)):
            Y, Sc = _thresh(net, ffi, Tc)
            keep = S.thresh_ref(Sall, Tc)
            assert np.array_equal(Y, Yall[keep]) and np.array_equal(Sc, Sall[keep]), (sj, j_in)
            assert np.isin(j, keep).all() == j_in and np.isin(j, keep).any() == j_in
            assert np.array_equal(keep, np.where(Sall >= sj)[0] if j_in else np.where(Sall > sj)[0])


def test_search_threshold_selects_everything_and_nothing(searched, mods):
    ffi = mods[0]
    net, Yall, Sall = searched
    Y, Sc = _thresh(net, ffi, 0.0)                                # everything, in original order, over many 1024-rounds
    assert Sall.shape[0] > 5 * 1024 and np.array_equal(Y, Yall) and np.array_equal(Sc, Sall)
    for Tc in (np.nextafter(np.float64(Sall.max()), np.inf), 2.0):
        Y, Sc = _thresh(net, ffi, Tc)                             # above the maximum: no proposal, and no error
        assert Y.shape == (0, 4) and Sc.shape == (0,)
    Y, Sc = _thresh(net, ffi, np.float64(Sall.max()))
    assert np.array_equal(Sc, Sall[Sall == Sall.max()]) and Y.shape[0] >= 1


# ------------------------------------------------------------------------------------------------- decode + filter
def _decode(ctx, case):
    return ctx.decode_filter(case["anchors"], case["deltas"], case["scores"], case["im_h"], case["im_w"], eps=case["eps"],
                             min_side=case["min_side"])


def _exact(ctx, case, what):
    b, s = _decode(ctx, case)
    rb, rs, _ = S.case_ref(case)
    assert b.shape == rb.shape, what
    assert np.array_equal(s, rs), what                            # the survivors, in r*11+s order
    assert np.array_equal(b, rb), what
    return s


@pytest.mark.parametrize("im", S.IMAGES)
def test_decode_clips(small, im):
    """Each clip alone, all four, boxes wholly outside the image -- exactly, at every eps and min_side."""
    ctx = small[0].ctx
    for eps in S.EPSS:
        for ms in S.MIN_SIDES:
            _exact(ctx, S.clip_case(im[0], im[1], eps, ms), (im, eps, ms))


@pytest.mark.parametrize("min_side", S.MIN_SIDES)
def test_decode_side_equal_to_min_side(small, min_side):
    """A side exactly min_side is kept, the double below it dropped, whichever of width and height is the smaller."""
    ctx = small[0].ctx
    case, eq, below = S.min_side_case(min_side)
    s = _exact(ctx, case, min_side)
    assert np.array_equal(S.survivors(s), eq)


@pytest.mark.parametrize("R", S.DECODE_ROWS)
def test_decode_row_counts_and_keep_patterns(small, R):
    """0 ... max_regions rows around the 256-candidate blocks of the flag / compaction kernels, every keep pattern."""
    ctx = small[0].ctx
    i = S.DECODE_ROWS.index(R)
    for pattern in S.KEEP_PATTERNS:
        s = _exact(ctx, S.rows_case(R, pattern, *S.rows_settings(i)), (R, pattern))
        assert np.array_equal(S.survivors(s), np.where(S.keep_flags(pattern, R * S.NSUB))[0])


def test_decode_refuses_more_rows_than_the_context_holds(small, mods):
    ffi = mods[0]
    ctx = small[0].ctx
    with pytest.raises(ffi.AzError) as e:
        _decode(ctx, S.rows_case(ctx.max_regions + 1, "all", 600, 1000, 0.0, 10.0))
    assert e.value.code == ffi.AZ_ERR_CAPACITY
    _exact(ctx, S.rows_case(24, "alternating", 600, 1000, 0.0, 10.0), "after the refusal")


@pytest.mark.parametrize("spec", S.RANDOM_CASES)
def test_decode_general_deltas(small, spec):
    """Log-size deltas in [-2, 2]: boxes at rtol 1e-6 / atol 1e-4 (f32-exp ulps times the box size); the keep / drop
    decision for every candidate whose reference margin is more than 1e-3 px from the threshold (at most 1 % are nearer:
    test_select_edges_host.py), where the surviving index set must be the reference's."""
    ctx = small[0].ctx
    case = S.random_case(*spec)
    b, s = _decode(ctx, case)
    margin = S.case_ref(case)[2]
    allb = S.decode_clipped(case["anchors"], case["deltas"], case["im_h"], case["im_w"], case["eps"])
    got = S.survivors(s)
    assert (np.diff(got) > 0).all() and got.min() >= 0 and got.max() < margin.shape[0]     # r*11+s order
    sure = np.abs(margin) > S.MARGIN_BAND
    kept = np.zeros(margin.shape[0], dtype=bool)
    kept[got] = True
    print("candidates %d, inside the band %d, kept %d" % (margin.shape[0], int((~sure).sum()), got.shape[0]))
    assert np.array_equal(np.where(kept & sure)[0], np.where((margin >= 0) & sure)[0])
    np.testing.assert_allclose(b, allb[got], rtol=S.BOX_RTOL, atol=S.BOX_ATOL)


def test_decode_capacity_clamp(mods):
    """A context at the smallest limits az_set_limits takes (64 regions, 64 candidates): 64 rows hold up to 704 kept
    candidates.  Exactly 64 kept: no error.  More: k_compact clamps the count -- az_decode_filter reports 64, has written
    the reference's first 64, and returns AZ_ERR_CAPACITY (the flag the search reports the same way); the context works on."""
    ffi = mods[0]
    ctx = ffi.AzContext(0, max_regions=64, max_candidates=64)
    try:
        def run(case):
            R = case["anchors"].shape[0]
            a, d, sc = ffi._f64(case["anchors"]), ffi._f32(case["deltas"]), ffi._f32(case["scores"])
            ob = np.full((R * S.NSUB, 4), -1.0, dtype=np.float64)
            os_ = np.full((R * S.NSUB,), -1.0, dtype=np.float32)
            n = ctypes.c_int(-1)
            rc = ctx.L.az_decode_filter(ctx.h, ffi._p(a, ctypes.c_double), ffi._p(d, ctypes.c_float), ffi._p(sc, ctypes.c_float), R,
                                        case["im_h"], case["im_w"], case["eps"], case["min_side"], ffi._p(ob, ctypes.c_double),
                                        ffi._p(os_, ctypes.c_float), R * S.NSUB, ctypes.byref(n))
            return rc, n.value, ob, os_

        fits = S.rows_case(64, "alternating", 600, 1000, 0.0, 10.0)
        fits["deltas"].reshape(-1, 4)[128:, 0] = 128.0                     # candidates 0, 2, ..., 126: exactly 64 kept
        rb, rs, _ = S.case_ref(fits)
        assert rb.shape[0] == 64
        rc, n, ob, os_ = run(fits)
        assert rc == ffi.AZ_OK, ctx.L.az_last_error(ctx.h)
        assert n == 64 and np.array_equal(ob[:64], rb) and np.array_equal(os_[:64], rs)
        for pattern, total in (("alternating", 352), ("all", 704)):
            case = S.rows_case(64, pattern, 600, 1000, 0.0, 10.0)
            rb, rs, _ = S.case_ref(case)
            assert rb.shape[0] == total
            rc, n, ob, os_ = run(case)
            assert rc == ffi.AZ_ERR_CAPACITY and b"capacity" in ctx.L.az_last_error(ctx.h)
            assert n == 64 and np.array_equal(ob[:64], rb[:64]) and np.array_equal(os_[:64], rs[:64])
            assert (os_[64:] == -1.0).all() and (ob[64:] == -1.0).all()    # nothing behind the capacity is written
        one_more = S.rows_case(64, "alternating", 600, 1000, 0.0, 10.0)
        one_more["deltas"].reshape(-1, 4)[130:, 0] = 128.0                 # 65 kept
        assert S.case_ref(one_more)[0].shape[0] == 65
        assert run(one_more)[:2] == (ffi.AZ_ERR_CAPACITY, 64)
        rc, n, ob, os_ = run(fits)                                         # the context still works
        assert rc == ffi.AZ_OK and n == 64 and np.array_equal(os_[:64], S.case_ref(fits)[1])
        with pytest.raises(ffi.AzError) as e:
            ctx.topk(np.zeros(65, dtype=np.float32), 10)                   # the same capacity bounds az_topk
        assert e.value.code == ffi.AZ_ERR_CAPACITY
        s = S.topk_scores("uniform_ties", 64, 10, 1)
        assert np.array_equal(ctx.topk(s, 10), S.topk_ref(s, 10)) and np.array_equal(ctx.topk_radix(s, 10), S.topk_ref(s, 10))
    finally:
        ctx.close()


def test_set_limits_smallest_accepted_values(mods):
    ffi = mods[0]
    for mr, mc in ((63, 64), (64, 63)):
        with pytest.raises(ffi.AzError) as e:
            ffi.AzContext(0, max_regions=mr, max_candidates=mc)
        assert e.value.code == ffi.AZ_ERR_INVALID
