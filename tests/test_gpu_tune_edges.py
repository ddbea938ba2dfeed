"""The zoom-threshold tuner at its edges ("Tuner edges"; cases and restatements: tests/tune_edges_ref.py,
proved on the CPU by tests/test_tune_edges_host.py).  A: the score pool and its radix select through the push API, against
np.sort / a stable sort on the bit key and the reference's heap (orc.tune_thresh).  B: the tuner-variant search and its
anchor history against the oracle's tuner loop run on the same device head (orc.im_propose_tune).  C: the front door
(detect.tune.tune_thresh, tools/set_thresh.py).  Every comparison is exact."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import search_limits_ref as R
import tune_edges_ref as T

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
VALUE = T.value_cases()


@pytest.fixture(scope="module")
def mods():
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipAZNet
    from oracle import az_oracle as orc
    return ffi, synth, HipAZNet, orc


@pytest.fixture(scope="module")
def small(mods):
    ffi, synth, HipAZNet, orc = mods
    return HipAZNet(synth.make_head(seed=77, **synth.SMALL_DIMS), name="tune_edges")


@pytest.fixture(scope="module")
def planted(mods):
    """The planted head on a context of 64 regions (capHis = 128 rows); candidates are given room so that the history is
    the only thing the frozen trees outgrow."""
    ffi, synth, HipAZNet, orc = mods
    head = R.case_inputs(T.cap_cases()["his_at"])[0]
    ctx = ffi.AzContext(0, max_regions=T.MIN_REGIONS, max_candidates=4096)
    return HipAZNet(head, name="tune_edges_planted", ctx=ctx)


def bits_of(x):
    return T.bits(np.asarray(x, dtype=np.float32))


def same_bits(a, b):
    return np.array_equal(bits_of(a), bits_of(b))


def kth(ctx, k):
    v, n = ctx.tune_kth_largest(k)
    return np.float32(v), n


def top_sorted(ctx, k):
    return T.sorted_desc_by_key(ctx.tune_top(k))


def fill(ctx, a, pieces=1, capacity=None):
    ctx.tune_begin(capacity or max(1, a.size))
    cuts = np.linspace(0, a.size, pieces + 1).astype(np.int64)
    for i in range(pieces):
        ctx.tune_push(a[cuts[i]:cuts[i + 1]])


def code_of(ffi, fn, *args):
    with pytest.raises(ffi.AzError) as e:
        fn(*args)
    return e.value.code, str(e.value)


# ================================================================================================= A. pool and select
@pytest.mark.parametrize("n", T.GRID_SIZES)
def test_select_and_keep_around_one_turn_of_the_grid(small, n):
    ctx = small.ctx
    a, ks = T.size_case(n)
    fill(ctx, a, pieces=3)
    ctx.tune_push(np.zeros(0, np.float32))                                  # a zero-length push changes nothing
    s = T.sorted_desc_by_key(a)
    for k in ks:
        v, cnt = kth(ctx, k)
        assert cnt == n and same_bits(v, T.ref_kth(a, k)), (n, k)
        assert v == T.ref_kth_by_value(a, k)
    for k in ks:
        got = top_sorted(ctx, k)
        want = s if n <= k else s[T.fkey(s) >= T.fkey(s[k - 1:k])[0]]
        assert same_bits(got, want), (n, k)
    ctx.tune_end()


@pytest.mark.parametrize("name", sorted(VALUE))
def test_select_over_key_bytes_signs_zeros_denormals_infinities(small, name):
    ctx = small.ctx
    a, ks = VALUE[name]
    fill(ctx, a, pieces=2)
    for k in ks:
        v, cnt = kth(ctx, k)
        assert cnt == a.size and same_bits(v, T.ref_kth(a, k)), (name, k, v)
        assert v == T.ref_kth_by_value(a, k)
        assert same_bits(top_sorted(ctx, k), T.ref_top(a, k)), (name, k)
    ctx.tune_end()


def test_n_le_k_is_the_heaps_answer(small, mods):
    ffi, synth, HipAZNet, orc = mods
    ctx = small.ctx
    answers = []
    for lists, k in T.nk_cases():
        ctx.tune_begin(64)
        for l in lists:
            ctx.tune_push(l)
        v, n = ctx.tune_kth_largest(k)
        assert n == sum(l.size for l in lists)
        assert v == float(orc.tune_thresh(lists, k))                        # the heap's answer, not only the sort's
        a = np.concatenate(lists)
        assert same_bits(top_sorted(ctx, k), T.ref_top(a, k))
        if n <= k:
            assert ctx.tune_top(k).size == n                                # everything
        answers.append(v)
        ctx.tune_end()
    assert answers[0] == answers[1] == float("-inf") and np.isfinite(answers[2])


def test_ties_at_the_cut_and_the_grow_and_retry_of_tune_top(small):
    ctx = small.ctx
    for name, (a, k, run) in T.tie_cases().items():
        fill(ctx, a)
        assert kth(ctx, k)[0] == np.float32(0.5)
        got = top_sorted(ctx, k)
        assert same_bits(got, np.sort(a[a >= np.float32(0.5)])[::-1])       # every score >= the k-th, as a multiset
        assert (got.size > k) == (name != "last")
        ctx.tune_end()
    a, k = T.grow_case()
    fill(ctx, a)
    n = ctypes.c_longlong(0)
    out = np.empty(k + T.TOP_SLACK, dtype=np.float32)
    rc = ctx.L.az_tune_top(ctx.h, k, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size, ctypes.byref(n))
    assert rc == -3 and n.value == a.size > out.size                        # the first cap is too small: AZ_ERR_CAPACITY, m
    got = ctx.tune_top(k)
    assert got.size == a.size and same_bits(got, a)
    ctx.tune_end()


def test_pool_capacity_and_state(small, mods):
    ffi, synth, HipAZNet, orc = mods
    ctx = small.ctx
    rng = np.random.RandomState(51)
    a = rng.uniform(-1, 1, 1000).astype(np.float32)
    fill(ctx, a, pieces=7)                                                  # exactly the capacity
    before = [kth(ctx, k) for k in (1, 500, 999)]
    assert [same_bits(v, T.ref_kth(a, k)) for (v, n), k in zip(before, (1, 500, 999))] == [True] * 3
    assert code_of(ffi, ctx.tune_push, np.zeros(1, np.float32))[0] == ffi.AZ_ERR_CAPACITY
    ctx.tune_push(np.zeros(0, np.float32))                                  # nothing more still fits
    assert [kth(ctx, k) for k in (1, 500, 999)] == before                   # the pool answers as before
    for k in (0, -1):
        assert code_of(ffi, ctx.tune_kth_largest, k)[0] == ffi.AZ_ERR_INVALID
        assert code_of(ffi, ctx.tune_top, k)[0] == ffi.AZ_ERR_INVALID
    assert code_of(ffi, ctx.tune_begin, 0)[0] == ffi.AZ_ERR_INVALID
    ctx.tune_begin(1000)                                                    # begin again: the count starts over
    assert ctx.tune_kth_largest(1) == (float("-inf"), 0) and ctx.tune_top(1).size == 0
    ctx.tune_push(a[:10])
    assert kth(ctx, 3) == (T.ref_kth(a[:10], 3), 10)
    ctx.tune_begin(10)                                                      # a smaller pool after a larger one takes 10
    ctx.tune_push(a[20:30])
    assert code_of(ffi, ctx.tune_push, a[:1])[0] == ffi.AZ_ERR_CAPACITY
    assert kth(ctx, 3) == (T.ref_kth(a[20:30], 3), 10)
    ctx.tune_begin(2000)                                                    # ... and a larger one after it 2000
    ctx.tune_push(np.concatenate([a, a]))
    assert kth(ctx, 1000) == (T.ref_kth(np.concatenate([a, a]), 1000), 2000)
    ctx.tune_end()
    for fn, arg in ((ctx.tune_push, a[:1]), (ctx.tune_kth_largest, 1), (ctx.tune_top, 1)):
        assert code_of(ffi, fn, arg)[0] == ffi.AZ_ERR_STATE
    ctx.tune_end()                                                          # a second end is harmless


def test_multi_rank_merge_equals_the_unsplit_select(small, mods):
    ffi, synth, HipAZNet, orc = mods
    ctx = small.ctx
    a, k, splits = T.shard_cases()
    fill(ctx, a)
    whole = kth(ctx, k)[0]
    ctx.tune_end()
    assert same_bits(whole, T.ref_kth(a, k))
    for shards in splits:
        tops = []
        for s in shards:                                                    # every rank: its shard's top scores
            ctx.tune_begin(max(1, s.size))
            ctx.tune_push(s)
            tops.append(ctx.tune_top(k))
            ctx.tune_end()
            assert same_bits(T.sorted_desc_by_key(tops[-1]), T.ref_top(s, k))
        ctx.tune_begin(max(1, sum(t.size for t in tops)))                   # rank 0: detect.tune.tune_thresh(gather=)
        for t in tops:
            ctx.tune_push(t)
        merged = kth(ctx, k)[0]
        ctx.tune_end()
        assert same_bits(merged, whole), len(shards)
        assert float(merged) == float(orc.tune_thresh(shards, k))


# ================================================================================================ B. the tuner's search
def injected(net, fmap):
    class Injected(object):          # pycaffe-shaped view of the HIP head: the oracle's loop on the device's own scores
        name = "inj"
        blobs = net.blobs

        def forward(self, blobs=None, **kw):
            kw.pop("data", None)
            kw["conv5_3"] = fmap
            return net.forward(blobs=blobs, **kw)
    inj = Injected()
    return {"full": inj, "fc": inj}


PLAIN = dict(speculate=False, fused=False, fused_levels=False, static_tree=False, pair_spec=False, full_spec=False,
             early_end=False)


def tparams(ffi, H, W, scale, Tz, batch=10000, nprop=2000, **kw):
    return ffi.AzContext.make_params(H, W, scale, Tz, num_proposals=nprop, batch_size=batch, tune=True, **kw)


def tuner_run(ffi, net, H, W, scale, Tz, batch=10000, nprop=2000):
    Y, S, st = net.propose(tparams(ffi, H, W, scale, Tz, batch, nprop), want_scores=True, want_stats=True)
    regions, zoom = net.ctx.last_anchors()
    return dict(Y=Y, S=S, st=st, regions=regions, zoom=zoom)


def check_vs_oracle(orc, net, fmap, got, H, W, scale, Tz, batch=10000, nprop=2000):
    """Regions and zoom scores bit for bit, num_eval, per-level rows, proposals as tests/test_gpu_next.py compares them.
    Tz goes to the oracle as the Python float it is: its comparison is float64 (tests/test_tune_edges_host.py)."""
    cfg = orc.OracleCfg(Tz=Tz, BATCH_SIZE=batch, NUM_PROPOSALS=nprop)
    Y5, Bhis = orc.im_propose_tune(injected(net, fmap), (H, W), scale, cfg)
    assert np.array_equal(got["regions"], Bhis[:, :4])
    assert np.array_equal(got["zoom"].astype(np.float64), Bhis[:, 4])
    st = got["st"]
    sizes = T.level_sizes(Bhis, Tz)
    assert st.num_eval == Bhis.shape[0] and st.n_levels == orc.num_levels(H, W)
    assert list(st.level_regions[:st.n_levels]) == sizes + [0] * (st.n_levels - len(sizes))
    assert got["Y"].shape == Y5[:, :4].shape
    assert np.array_equal(np.sort(got["S"].astype(np.float64)), np.sort(Y5[:, 4]))
    return Bhis, sizes


def small_map(synth, H, W, scale, seed=6):
    fh, fw = R.map_size(H, W, scale)
    return synth.make_feature_map(seed, synth.SMALL_DIMS["C"], fh, fw)


@pytest.mark.parametrize("H,W", T.LEVEL_SHAPES + [T.THRESH_SHAPE])
def test_level_counts_one_two_and_the_deepest_that_fits(small, mods, H, W):
    ffi, synth, HipAZNet, orc = mods
    scale = T.shape_scale(H, W)
    fmap = small_map(synth, H, W, scale)
    small.set_conv(fmap)
    got = tuner_run(ffi, small, H, W, scale, 0.0)
    Bhis, sizes = check_vs_oracle(orc, small, fmap, got, H, W, scale, 0.0)
    full = T.full_tree(H, W)
    assert sizes == full["P"] and got["st"].n_levels == full["K"] == len(sizes)
    if full["K"] == 1:
        assert got["regions"].shape == (1, 4)                               # Bhis is the root alone
        with pytest.raises(ffi.AzError):                                    # ... and the plain search has no level at all
            small.propose(ffi.AzContext.make_params(H, W, scale, 0.0))
    else:
        st2 = small.propose(ffi.AzContext.make_params(H, W, scale, 0.0), want_stats=True)[1]
        assert got["st"].n_levels == st2.n_levels + 1
    if (H, W) == T.LEVEL_SHAPES[-1]:
        assert max(full["P"]) <= T.DEFAULT_REGIONS < max(T.full_tree(*T.TOO_DEEP)["P"])


def test_root_below_tz_divides_in_the_tuner_and_is_forced_in_the_plain_search(planted, mods):
    ffi, synth, HipAZNet, orc = mods
    c = dict(T.cap_cases()["his_at"], runs=[])
    H, W, scale = c["H"], c["W"], c["scale"]
    _, fmap, mask = R.case_inputs(c)
    planted.set_conv(fmap)
    got = tuner_run(ffi, planted, H, W, scale, R.TZ)
    Bhis, sizes = check_vs_oracle(orc, planted, fmap, got, H, W, scale, R.TZ)
    assert sizes == [1, 5] and (got["zoom"] < R.TZ).all()                   # the root, below Tz, divided: judged against 0
    assert list(got["st"].level_zoomed[:3]) == [1, 0, 0]
    Y, st = planted.propose(ffi.AzContext.make_params(H, W, scale, R.TZ, **PLAIN), want_stats=True)
    Ya, Sa = planted.ctx.last_candidates()
    tr = orc.im_propose(injected(planted, fmap), (H, W), scale, orc.OracleCfg(Tz=R.TZ), return_trace=True)[1]
    assert [l["B"].shape[0] for l in tr["levels"]] == [1, 5] == list(st.level_regions[:2])
    assert st.n_levels == got["st"].n_levels - 1 and list(st.level_zoomed[:2]) == [1, 0]
    assert tr["levels"][0]["zoom"][0] == 1.0 and got["zoom"][0] < R.TZ      # forced there, recorded raw here
    assert np.array_equal(Sa.astype(np.float64), tr["aScores"])


PLAIN_FORMS = ({}, dict(speculate=False, fused=False, fused_levels=False))


def test_a_score_on_the_threshold_compares_in_double(small, mods):
    """Tz = float(z_j) keeps anchor j, the next double above it drops it -- in the tuner's search, in the plain search in
    two forms, and in the oracle, whose comparison is float64 as well."""
    ffi, synth, HipAZNet, orc = mods
    H, W = T.THRESH_SHAPE
    scale = T.shape_scale(H, W)
    fmap = small_map(synth, H, W, scale)
    small.set_conv(fmap)
    got0 = tuner_run(ffi, small, H, W, scale, 0.0)
    sizes0 = list(got0["st"].level_regions[:got0["st"].n_levels])
    j, zj = T.pick_anchor(got0["zoom"], sizes0)
    at, past = T.thresholds_at(zj)
    kids = orc.divide_region(got0["regions"][j:j + 1], 10)
    assert kids.shape[0] > 0 and np.float32(past) == zj and past > float(zj)
    g_at = tuner_run(ffi, small, H, W, scale, at)
    B_at, s_at = check_vs_oracle(orc, small, fmap, g_at, H, W, scale, at)
    assert s_at[:3] == [1, sizes0[1], kids.shape[0]]
    assert np.array_equal(g_at["regions"][1 + sizes0[1]:1 + sizes0[1] + kids.shape[0]], kids)   # j's children are there
    g_past = tuner_run(ffi, small, H, W, scale, past)
    B_past, s_past = check_vs_oracle(orc, small, fmap, g_past, H, W, scale, past)
    assert s_past == [1, sizes0[1]]                                         # ... and one double higher they are not
    for Tz, n2 in ((at, kids.shape[0]), (past, 0)):
        tr = orc.im_propose(injected(small, fmap), (H, W), scale, orc.OracleCfg(Tz=Tz), return_trace=True)[1]
        for form in PLAIN_FORMS:
            Y, S, st = small.propose(ffi.AzContext.make_params(H, W, scale, Tz, **form), want_scores=True, want_stats=True)
            Ya, Sa = small.ctx.last_candidates()
            assert list(st.level_regions[:3]) == [1, sizes0[1], n2], (Tz, form)
            assert st.num_eval == tr["num_eval"] and np.array_equal(Sa.astype(np.float64), tr["aScores"])


@pytest.mark.parametrize("H,W,scale,tzq", [(375, 500, 1.6, None), (375, 500, 1.6, 0.5), (300, 500, 0.4, None), (240, 320, 0.5, 0.4)])
def test_chunks_and_shared_rois(small, mods, H, W, scale, tzq):
    """batch_size 1, 7 and one below / at / above a level's region count, each against the oracle chunked the same way (its
    np.unique per chunk); down-scaled images, where many regions of a level share a roi (the zoom_u[inv[r]] indirection
    of k_record_anchors).  Regions that share a dedup key take the key's FIRST region's roi, and which one that is depends
    on the chunking: only where no level shares a roi are the scores those of the unchunked search."""
    ffi, synth, HipAZNet, orc = mods
    fmap = small_map(synth, H, W, scale, seed=9)
    small.set_conv(fmap)
    base = tuner_run(ffi, small, H, W, scale, 0.0)
    Tz = 0.0 if tzq is None else float(np.quantile(base["zoom"].astype(np.float64), tzq))
    ref = tuner_run(ffi, small, H, W, scale, Tz)
    st = ref["st"]
    sizes = [int(x) for x in st.level_regions[:st.n_levels] if x > 0]
    shared = any(st.level_unique[l] < st.level_regions[l] for l in range(st.n_levels))
    assert shared or scale >= 1                                             # down-scaled: regions do share rois
    P = sizes[-2]
    assert P > 2
    for batch in (1, 7, P - 1, P, P + 1):
        got = tuner_run(ffi, small, H, W, scale, Tz, batch=batch)
        check_vs_oracle(orc, small, fmap, got, H, W, scale, Tz, batch=batch)
        if not shared:
            assert np.array_equal(got["regions"], ref["regions"]) and same_bits(got["zoom"], ref["zoom"]), batch
        if batch == 1:
            assert list(got["st"].level_unique[:st.n_levels]) == list(got["st"].level_regions[:st.n_levels])


# ------------------------------------------------------------------------------------------------ capHis = 2 * max_regions
def test_history_at_its_capacity_and_past_it(planted, mods):
    ffi, synth, HipAZNet, orc = mods
    cases = T.cap_cases()
    ctx = planted.ctx
    at, past = cases["his_at"], cases["his_past"]
    H, W, scale = at["H"], at["W"], at["scale"]
    f_at, f_past = R.case_inputs(at)[1], R.case_inputs(past)[1]
    # at the capacity the search is right
    planted.set_conv(f_at)
    g_at = tuner_run(ffi, planted, H, W, scale, R.TZ)
    Bhis, sizes = check_vs_oracle(orc, planted, f_at, g_at, H, W, scale, R.TZ)
    assert sizes == at["P"] and Bhis.shape[0] == T.HIS_FACTOR * T.MIN_REGIONS == 2 * ctx.max_regions
    assert list(g_at["st"].level_zoomed[:5]) == at["PZ"][:5]
    # past it: a clean refusal that names the limit; the history and (with a pool open) the pool answer nothing
    ctx.tune_begin(4096)
    planted.propose(tparams(ffi, H, W, scale, R.TZ))                        # 128 scores pooled
    assert ctx.tune_kth_largest(10 ** 6) == (float("-inf"), 128)
    planted.set_conv(f_past)
    code, msg = code_of(ffi, planted.propose, tparams(ffi, H, W, scale, R.TZ))
    assert code == ffi.AZ_ERR_CAPACITY and "az_set_limits" in msg and "flags 16" in msg
    assert code_of(ffi, ctx.last_anchors)[0] == ffi.AZ_ERR_STATE
    for fn in (ctx.tune_kth_largest, ctx.tune_top):
        code, msg = code_of(ffi, fn, 5)
        assert code == ffi.AZ_ERR_CAPACITY and "az_tune_begin" in msg
    assert code_of(ffi, ctx.tune_push, np.zeros(1, np.float32))[0] == ffi.AZ_ERR_CAPACITY
    # the next, smaller tuner search on the context is right, and the pool is good again after the next begin
    c2 = dict(at, runs=at["runs"][:3])
    f2 = R.case_inputs(c2)[1]
    planted.set_conv(f2)
    ctx.tune_begin(4096)
    g2 = tuner_run(ffi, planted, H, W, scale, R.TZ)
    B2, s2 = check_vs_oracle(orc, planted, f2, g2, H, W, scale, R.TZ)
    assert s2 == T.tuner_populations(H, W, scale, T.mask_of_case(c2))["P"][:len(s2)] and 6 < B2.shape[0] < 128
    assert same_bits(top_sorted(ctx, 10 ** 6), T.sorted_desc_by_key(g2["zoom"]))
    ctx.tune_end()
    # ... and without a pool the refused search leaves the next one alone as well
    planted.set_conv(f_past)
    assert code_of(ffi, planted.propose, tparams(ffi, H, W, scale, R.TZ))[0] == ffi.AZ_ERR_CAPACITY
    planted.set_conv(f_at)
    g3 = tuner_run(ffi, planted, H, W, scale, R.TZ)
    assert np.array_equal(g3["regions"], g_at["regions"]) and same_bits(g3["zoom"], g_at["zoom"])


# ------------------------------------------------------------------------------------------------ the pool fed by searches
FEED = [(375, 500, 1.6, None), (100, 64, 6.0, 0.5), (120, 200, 5.0, None), (375, 500, 1.6, 0.6), (30, 37, 20.0, None)]


@pytest.fixture(scope="module")
def feed(small, mods):
    """The searches that feed the pool (mixed shapes, some at Tz > 0): maps, thresholds, and each search's history and
    result on a context in its default state, computed once."""
    ffi, synth, HipAZNet, orc = mods
    runs = []
    for i, (H, W, scale, tzq) in enumerate(FEED):
        fmap = small_map(synth, H, W, scale, seed=20 + i)
        small.set_conv(fmap)
        Tz = 0.0
        if tzq is not None:
            Tz = float(np.quantile(tuner_run(ffi, small, H, W, scale, 0.0)["zoom"].astype(np.float64), tzq))
        runs.append(dict(H=H, W=W, scale=scale, Tz=Tz, fmap=fmap, ref=tuner_run(ffi, small, H, W, scale, Tz)))
    return runs


def feed_pool(ffi, net, runs, between=None):
    got = []
    for r in runs:
        net.set_conv(r["fmap"])
        got.append(tuner_run(ffi, net, r["H"], r["W"], r["scale"], r["Tz"]))
        if between is not None:
            between(r)
    return got


def assert_feed(ctx, got, runs):
    for g, r in zip(got, runs):
        for key in ("Y", "S", "regions", "zoom"):
            assert g[key].shape == r["ref"][key].shape and np.array_equal(bits64(g[key]), bits64(r["ref"][key])), key
    want = np.concatenate([g["zoom"] for g in got])
    assert same_bits(top_sorted(ctx, 10 ** 7), T.sorted_desc_by_key(want))  # the pool is the histories' scores, no more


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_pool_fed_by_searches_and_its_overflow(small, mods, feed):
    ffi, synth, HipAZNet, orc = mods
    ctx = small.ctx
    total = sum(r["ref"]["zoom"].size for r in feed)
    ctx.tune_begin(total)                                                   # exactly what the searches append
    got = feed_pool(ffi, small, feed)
    assert ctx.tune_kth_largest(10 ** 7) == (float("-inf"), total)
    assert_feed(ctx, got, feed)
    allz = np.concatenate([g["zoom"] for g in got])
    for k in (1, 100, total - 1):
        assert same_bits(kth(ctx, k)[0], T.ref_kth(allz, k))
    ctx.tune_end()
    # a pool smaller than what the searches append: the device counts what it dropped
    cap = total - 7
    ctx.tune_begin(cap)
    feed_pool(ffi, small, feed)
    v, n = ctypes.c_float(1.0), ctypes.c_longlong(-1)
    rc = ctx.L.az_tune_kth_largest(ctx.h, 5, ctypes.byref(v), ctypes.byref(n))
    assert rc == ffi.AZ_ERR_CAPACITY and n.value == cap
    assert "raise az_tune_begin's capacity" in ctx.L.az_last_error(ctx.h).decode()
    assert code_of(ffi, ctx.tune_top, 5)[0] == ffi.AZ_ERR_CAPACITY
    ctx.tune_begin(total)                                                   # the next begin starts clean
    assert ctx.tune_kth_largest(1) == (float("-inf"), 0)
    ctx.tune_end()


def test_pool_feeding_under_graphs_and_on_two_lanes(mods, feed):
    """The same bits with az_set_graphs(1) -- the search with a pool open is not captured, the one without is -- and on a
    two-lane context with plain searches queued in between (the tuner's search always runs on the first lane)."""
    ffi, synth, HipAZNet, orc = mods
    head = synth.make_head(seed=77, **synth.SMALL_DIMS)
    total = sum(r["ref"]["zoom"].size for r in feed)
    net = HipAZNet(head, name="tune_edges_graphs")
    net.ctx.set_graphs(1)
    for rep in range(2):                                                    # without a pool: captured, then replayed
        got = feed_pool(ffi, net, feed)
        for g, r in zip(got, feed):
            assert np.array_equal(g["regions"], r["ref"]["regions"]) and same_bits(g["zoom"], r["ref"]["zoom"])
            assert np.array_equal(g["Y"], r["ref"]["Y"]) and same_bits(g["S"], r["ref"]["S"])
    net.ctx.tune_begin(total)
    assert_feed(net.ctx, feed_pool(ffi, net, feed), feed)
    net.ctx.tune_end()
    net.ctx.close()

    net = HipAZNet(head, name="tune_edges_lanes")
    ctx = net.ctx
    ctx.set_lanes(2)
    plain = {}

    def between(r):                                                         # two plain searches of the same map, queued
        p = ffi.AzContext.make_params(r["H"], r["W"], r["scale"], r["Tz"])
        if orc.num_levels(r["H"], r["W"]) < 2:
            return
        ctx.propose_launch(p)
        ctx.propose_launch(p)
        a, b = ctx.propose_fetch(), ctx.propose_fetch()
        assert np.array_equal(a, b)
        plain[(r["H"], r["W"], r["Tz"])] = a

    ctx.tune_begin(total)
    assert_feed(ctx, feed_pool(ffi, net, feed, between=between), feed)
    ctx.tune_end()
    assert len(plain) >= 3
    ctx.close()


def test_two_tuner_searches_queued_back_to_back(small, mods, feed):
    """launch, launch, fetch, fetch: both results right, the pool holds both, and the anchor history -- one buffer per
    context -- is refused between the fetches (the second search has overwritten it), as az_last_candidates refuses."""
    ffi, synth, HipAZNet, orc = mods
    ctx = small.ctx
    r0, r1 = feed[0], feed[3]                                               # one shape and map, Tz = 0 and Tz > 0
    assert (r0["H"], r0["W"]) == (r1["H"], r1["W"]) and r0["Tz"] != r1["Tz"]
    small.set_conv(r0["fmap"])
    refs = [tuner_run(ffi, small, r["H"], r["W"], r["scale"], r["Tz"]) for r in (r0, r1)]
    assert refs[0]["zoom"].size != refs[1]["zoom"].size
    ctx.tune_begin(refs[0]["zoom"].size + refs[1]["zoom"].size)
    for r in (r0, r1):
        ctx.propose_launch(tparams(ffi, r["H"], r["W"], r["scale"], r["Tz"]))
    Y0, S0 = ctx.propose_fetch(want_scores=True)
    code, msg = code_of(ffi, ctx.last_anchors)
    assert code == ffi.AZ_ERR_STATE and "later tuner search" in msg
    assert code_of(ffi, ctx.last_candidates)[0] == ffi.AZ_ERR_STATE
    Y1, S1 = ctx.propose_fetch(want_scores=True)
    regions, zoom = ctx.last_anchors()                                      # after the second fetch: the second's
    assert np.array_equal(regions, refs[1]["regions"]) and same_bits(zoom, refs[1]["zoom"])
    for (Y, S), ref in (((Y0, S0), refs[0]), ((Y1, S1), refs[1])):
        assert np.array_equal(Y, ref["Y"]) and same_bits(S, ref["S"])
    want = np.concatenate([refs[0]["zoom"], refs[1]["zoom"]])
    assert same_bits(top_sorted(ctx, 10 ** 7), T.sorted_desc_by_key(want))
    ctx.tune_end()
    # a tuner search launched behind a FETCHED one takes the history as well, until it is fetched itself
    small.propose(tparams(ffi, r0["H"], r0["W"], r0["scale"], r0["Tz"]))
    ctx.propose_launch(tparams(ffi, r1["H"], r1["W"], r1["scale"], r1["Tz"]))
    assert code_of(ffi, ctx.last_anchors)[0] == ffi.AZ_ERR_STATE
    ctx.propose_fetch()
    assert same_bits(ctx.last_anchors()[1], refs[1]["zoom"])
    # ... and a plain search queued behind a tuner search leaves the history alone
    ctx.propose_launch(tparams(ffi, r0["H"], r0["W"], r0["scale"], r0["Tz"]))
    ctx.propose_launch(ffi.AzContext.make_params(r0["H"], r0["W"], r0["scale"], 0.0))
    ctx.propose_fetch()
    assert same_bits(ctx.last_anchors()[1], refs[0]["zoom"])
    ctx.propose_fetch()


# ======================================================================================================= C. front door
class FakeBackbone(object):
    """conv5_3 as a function of the image blob's size (tests/test_gpu_next.py)."""
    device = "cuda:0"

    def __init__(self, synth):
        self.synth, self.fmaps = synth, {}

    def __call__(self, blob):
        import torch
        key = tuple(blob.shape[2:])
        if key not in self.fmaps:
            s = self.synth
            self.fmaps[key] = s.make_feature_map(60 + len(self.fmaps), s.SMALL_DIMS["C"], s.conv_out_size(key[0]),
                                                 s.conv_out_size(key[1]))
        return torch.from_numpy(self.fmaps[key]).to("cuda:0")


def test_tune_thresh_minus_infinity_and_the_property_it_exists_for(small, mods, tmp_path):
    ffi, synth, HipAZNet, orc = mods
    from detect import tune as U
    from detect.config import cfg, cfg_set_mode, cfg_set_path, cfg_load_thresh
    import detect.config as C
    from datasets.factory import get_imdb
    old = (cfg.SEAR.get("Tz", 0.0), cfg.SEAR.get("NUM_PROPOSALS", 300), cfg.ROOT_DIR, cfg.TRAIN.ANCHORS_PER_IMG,
           cfg.TEST.MAX_SIZE)
    cfg_set_mode("Train")
    cfg_set_path("pytest_tune_edges")
    cfg.ROOT_DIR = str(tmp_path)
    cfg.TEST.MAX_SIZE = 1000
    net = small
    try:
        db = get_imdb("synthetic_120x200_3")
        n_img = len(db.image_index)
        net.backbone = FakeBackbone(synth)
        nets = {"full": net, "fc": net}
        hist = [U.im_propose(net, db.image_at(i))[1] for i in range(n_img)]   # the anchors of the Tz = 0 runs
        scores = np.concatenate([h[:, 4] for h in hist])
        pkl = os.path.join(C.get_output_dir(db, net), "thresh.pkl")
        # at most k anchors in the set: the threshold is -inf, pickled and read back as such
        cfg.TRAIN.ANCHORS_PER_IMG = -(-scores.size // n_img)
        assert n_img * cfg.TRAIN.ANCHORS_PER_IMG >= scores.size
        got = U.tune_thresh(nets, db)
        assert got == -np.inf and cfg_load_thresh(pkl) == -np.inf
        assert got == orc.tune_thresh([h[:, 4] for h in hist], n_img * cfg.TRAIN.ANCHORS_PER_IMG)
        # a search at Tz = -inf has the bits of the search at Tz = 0
        im = db.image_at(0)
        runs = {}
        for Tz in (0.0, float(got)):
            cfg.SEAR.Tz = Tz
            Y5, Bhis = U.im_propose(net, im)
            runs[Tz] = (Y5, Bhis)
            H, W = im.shape[:2]
            scale = U._im_scale(im.shape)[0]
            Y, S = net.propose(ffi.AzContext.make_params(H, W, scale, Tz), want_scores=True)
            runs[(Tz, "plain")] = (Y, S.astype(np.float64))
        cfg.SEAR.Tz = 0.0
        for a, b in ((0.0, float(got)), ((0.0, "plain"), (float(got), "plain"))):
            assert np.array_equal(runs[a][0], runs[b][0]) and np.array_equal(runs[a][1], runs[b][1])
        # an ordinary k: at least k anchors score >= the threshold and fewer than k score above it
        for per_img in (1, 7, 40):
            cfg.TRAIN.ANCHORS_PER_IMG = per_img
            k = n_img * per_img
            assert k < scores.size
            t = U.tune_thresh(nets, db)
            assert (scores >= t).sum() >= k > (scores > t).sum()
            assert t == orc.tune_thresh([h[:, 4] for h in hist], k) and cfg_load_thresh(pkl) == t
            assert isinstance(t, np.float64) and np.float64(np.float32(t)) == t     # a tuned threshold is a widened float32
    finally:
        net.backbone = None
        cfg.SEAR.Tz, cfg.SEAR.NUM_PROPOSALS, cfg.ROOT_DIR, cfg.TRAIN.ANCHORS_PER_IMG, cfg.TEST.MAX_SIZE = old
        cfg_set_path(None)


def test_set_thresh_cli_without_a_pyramid(mods, tmp_path):
    """tools/set_thresh.py in a fresh child process on a synthetic imdb: the pickled value is tune_thresh's in-process value
    on the same set with the same net (both with PyTorch's own convolutions: the same bits in every process)."""
    import shutil
    import torch
    from detect import config as C
    from detect import tune as U
    from datasets.factory import get_imdb
    cfg = C.cfg
    imdb_name, per_img = "synthetic_120x200_2", 9
    exp = "tune_edges_cli_%d" % os.getpid()
    out_root = os.path.join(cfg.ROOT_DIR, "output", exp)
    yml = os.path.join(str(tmp_path), "tune.yml")
    with open(yml, "w") as f:
        f.write("TRAIN:\n  ANCHORS_PER_IMG: %d\n" % per_img)
    env = dict(os.environ)
    env["AZ_BACKBONE_DETERMINISTIC"] = "2"
    env["PYTHONPATH"] = os.pathsep.join([TOOLS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    old = (cfg.SEAR.get("Tz", 0.0), cfg.SEAR.get("NUM_PROPOSALS", 300), cfg.TRAIN.ANCHORS_PER_IMG, cfg.EXP_DIR,
           torch.backends.cudnn.deterministic, os.environ.get("AZ_BACKBONE_DETERMINISTIC"), torch.backends.cudnn.enabled)
    try:
        r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(TOOLS, "set_thresh.py"), "--gpu", "0",
                            "--net", "synthetic", "--imdb", imdb_name, "--exp", exp, "--cfg", yml],
                           env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        assert "the threshold is set to" in r.stdout and r.stdout.count("im_tune: ") == 2
        pf = os.path.join(out_root, imdb_name, "vgg16_az_net_synthetic_1234", "thresh.pkl")
        cli = C.cfg_load_thresh(pf)
        sys.path.insert(0, TOOLS)
        import prop_az
        os.environ["AZ_BACKBONE_DETERMINISTIC"] = "2"
        net = prop_az.load_net("synthetic", 0)
        C.cfg_set_mode("Train")
        C.cfg_set_path(exp)
        cfg.TRAIN.ANCHORS_PER_IMG = per_img
        mine = U.tune_thresh({"full": net, "fc": net}, get_imdb(imdb_name))
        net.ctx.close()
        assert isinstance(cli, np.float64) and np.isfinite(cli) and 0.0 <= cli <= 1.0
        assert cli == mine
    finally:
        cfg.SEAR.Tz, cfg.SEAR.NUM_PROPOSALS, cfg.TRAIN.ANCHORS_PER_IMG = old[:3]
        C.cfg_set_path(None if old[3] == "default" else old[3])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.enabled = old[4], old[6]
        if old[5] is None:
            os.environ.pop("AZ_BACKBONE_DETERMINISTIC", None)
        else:
            os.environ["AZ_BACKBONE_DETERMINISTIC"] = old[5]
        shutil.rmtree(out_root, ignore_errors=True)
