"""CPU: the cases of tests/tune_edges_ref.py reach the edges their names say, and its restatements tell right from wrong.
The key-byte sets agree outside their byte, the ties tie where stated, the grid sizes straddle one turn of the grid-stride
loops, the frozen planted trees have the history sizes tests/tune_edges_cases.py records (recomputed, and walked by the
oracle's own tuner loop with the planted head), and three wrong restatements -- a select that skips a byte pass, `>` for
`>=` in the keep, a signed comparison of raw bits -- each disagree with np.sort somewhere in the table.  Also what the
threshold comparison of the reference is ("Tuner edges", item 3): float64 on both sides."""
import numpy as np
import pytest

import search_limits_ref as R
import tune_edges_ref as T
from oracle import az_oracle as orc

VALUE = T.value_cases()


def _same_bits(a, b):
    return np.array_equal(T.bits(np.asarray(a, dtype=np.float32)), T.bits(np.asarray(b, dtype=np.float32)))


# ---------------------------------------------------------------------------------------------------------------- keys
@pytest.mark.parametrize("byte,neg", [(3, False), (2, False), (1, False), (0, False), (2, True), (1, True), (0, True)])
def test_byte_sets_differ_in_their_byte_only(byte, neg):
    s = T.byte_set(byte, neg)
    k = T.fkey(s)
    mask = np.uint32(~(0xff << (8 * byte)) & 0xffffffff)
    assert s.size == 256 and np.unique(k).size == 256 and not T.has_nan(s)
    assert np.unique(k & mask).size == 1                                   # every other byte agrees
    assert np.array_equal(np.sort((k >> np.uint32(8 * byte)) & np.uint32(255)), np.arange(256))
    assert _same_bits(T.key_to_float(k), s)
    if byte != 3:
        assert bool((s < 0).all()) == neg and bool((s > 0).all()) == (not neg)
    else:
        assert s.min() == -np.inf and s.max() == np.finfo(np.float32).max
    a, ks = T.byte_case(byte, neg)
    bucket = np.isin(T.bits(T.sorted_desc_by_key(a)), T.bits(s))
    first = int(np.argmax(bucket)) + 1
    assert {first, first + 127, first + 255} <= set(ks)                    # k at both ends of the bucket and inside it
    assert bucket[first - 1:first + 255].all() and bucket.sum() == (257 if byte == 3 else 256)


def test_key_order_is_value_order_and_splits_the_zeros():
    a = T.random_bits(5000, 3)
    assert not T.has_nan(a)
    assert (np.abs(a[np.isfinite(a)]) < 1e-38).any() and (a < 0).any() and (a > 0).any()
    s = T.sorted_desc_by_key(a)
    assert np.array_equal(s, np.sort(a)[::-1])                             # same values (== does not see the zeros' sign)
    z = np.array([-0.0, 0.0], dtype=np.float32)
    assert z[0] == z[1] and int(T.fkey(z)[1]) - int(T.fkey(z)[0]) == 1       # equal as values, adjacent keys
    zs, ks = VALUE["zeros"]
    got = [T.ref_kth(zs, k) for k in ks]
    assert [np.signbit(v) for v in got[2:7]] == [False, False, True, True, True]
    assert all(v == 0 for v in got[2:7])


def test_sizes_straddle_one_turn_of_the_grid():
    assert T.GRID == 524288 and T.GRID_SIZES == (1, 255, 256, 257, 524287, 524288, 524289, 1048577)
    assert max(T.GRID_SIZES) * 4 < 5 * 2 ** 20                             # the largest pool: 4 MB


# ---------------------------------------------------------------------------------------------- restatements vs np.sort
def _table():
    for name, (a, ks) in VALUE.items():
        yield name, a, ks
    for n in T.GRID_SIZES[:5]:
        a, ks = T.size_case(n)
        yield "n%d" % n, a, ks


def test_restated_select_and_keep_equal_the_sort():
    for name, a, ks in _table():
        for k in ks:
            want = T.ref_kth(a, k)
            got = T.dev_kth(a, k)
            assert _same_bits(got, want), (name, k)
            assert got == T.ref_kth_by_value(a, k), (name, k)
            top = T.dev_top(a, k)
            assert _same_bits(top, T.ref_top(a, k)), (name, k)
            if a.size > k:
                assert np.array_equal(top, np.sort(a[a >= want])[::-1]) or want == 0, (name, k)   # (a cut between -0.0 and +0.0: only the keys tell)
                assert top.size >= k and _same_bits(top[-1:], [want])


def test_wrong_restatements_disagree_with_the_sort():
    skipped = {24: 0, 16: 0, 8: 0, 0: 0}
    strict = signed = 0
    for name, a, ks in _table():
        for k in ks:
            if a.size <= k:
                continue
            want = T.ref_kth_by_value(a, k)
            for sh in skipped:
                skipped[sh] += int(not (T.dev_kth(a, k, skip_shift=sh) == want))
            strict += int(not np.array_equal(T.dev_top(a, k, strict=True), np.sort(a[a >= want])[::-1]))
            signed += int(not (T.signed_bits_kth(a, k) == want))
    assert all(v > 0 for v in skipped.values()), skipped
    assert strict > 0 and signed > 0
    # ... and the signed order is wrong exactly where negatives meet: right on an all-positive set
    a, ks = T.byte_case(1)
    pos = a[a > 0]
    assert all(T.signed_bits_kth(pos, k) == T.ref_kth_by_value(pos, k) for k in (1, 2, pos.size - 1))


# ------------------------------------------------------------------------------------------------------- n <= k, ties
def test_n_le_k_is_the_heaps_answer():
    (l0, k), (l1, _), (l2, _) = T.nk_cases()
    assert [sum(x.size for x in l) for l in (l0, l1, l2)] == [k - 1, k, k + 1]
    for lists, want_inf in ((l0, True), (l1, True), (l2, False)):
        a = np.concatenate(lists)
        h = T.heap_thresh(lists, k)
        assert (h == -np.inf) == want_inf
        assert float(T.dev_kth(a, k)) == h
        if not want_inf:
            assert h == float(np.sort(a)[1]) and np.sort(a)[1] == np.sort(a)[::-1][:k].min()   # the minimum of the k kept
        else:
            assert T.dev_top(a, k).size == a.size                          # tune_top at n <= k returns everything


def test_tie_cases_tie_where_stated():
    for name, (a, k, run) in T.tie_cases().items():
        s = np.sort(a)[::-1]
        assert s[k - 1] == np.float32(0.5) and (a == np.float32(0.5)).sum() == run
        first = int(np.argmax(s == np.float32(0.5))) + 1
        assert k == {"first": first, "middle": first + 16, "last": first + run - 1}[name]
        top = T.ref_top(a, k)
        assert top.size == first + run - 1 and (top.size > k) == (name != "last")
        assert _same_bits(T.dev_top(a, k), top) and T.dev_kth(a, k) == np.float32(0.5)
    a, k = T.grow_case()
    assert T.ref_top(a, k).size == a.size > k + T.TOP_SLACK


def test_shard_merge_equals_the_unsplit_select_and_the_heap():
    a, k, splits = T.shard_cases()
    want = T.ref_kth(a, k)
    assert (a == want).sum() >= 5                                          # ties at the cut ...
    assert [len(s) for s in splits] == [1, 2, 3, 8]
    seen = dict(empty=0, fewer=0, more=0, tie_shards=0)
    for shards in splits:
        assert _same_bits(np.concatenate(shards), a)
        seen["empty"] += sum(s.size == 0 for s in shards)
        seen["fewer"] += sum(0 < s.size < k for s in shards)
        seen["more"] += sum(s.size > k for s in shards)
        seen["tie_shards"] = max(seen["tie_shards"], sum(bool((s == want).any()) for s in shards))
        assert _same_bits(T.merged_thresh(shards, k), want)
        assert T.heap_thresh(shards, k) == float(want)
    assert seen["empty"] >= 2 and seen["fewer"] >= 2 and seen["more"] >= 3 and seen["tie_shards"] >= 4   # ... across shards


# ---------------------------------------------------------------------------------------------- planted history trees
def _cpu_net(head, fmap):
    onet = orc.OracleNet(head, feat_fn=lambda d: fmap)
    return {"full": onet, "fc": onet}


@pytest.fixture(scope="module")
def cap_runs():
    out = {}
    for name, c in T.cap_cases().items():
        head, fmap, mask = R.case_inputs(c)
        cfg = orc.OracleCfg(Tz=R.TZ, BATCH_SIZE=10000, NUM_PROPOSALS=300)
        out[name] = (orc.im_propose_tune(_cpu_net(head, fmap), (c["H"], c["W"]), c["scale"], cfg)[1], mask)
    return out


def test_history_cases_have_the_sizes_they_record(cap_runs):
    cases = T.cap_cases()
    cap = T.HIS_FACTOR * T.MIN_REGIONS
    for name, c in cases.items():
        assert c["scale"] == R.default_scale(c["H"], c["W"])
        p = T.tuner_populations(c["H"], c["W"], c["scale"], cap_runs[name][1])
        assert p["K"] == 6 and p["P"] == c["P"] and p["PZ"] == c["PZ"] and p["CH"][:5] == c["CH"] and p["his"] == c["his"]
        assert max(p["P"]) <= T.MIN_REGIONS and max(p["CH"]) <= 4 * T.MIN_REGIONS       # every level fits the context ...
        # the oracle's own tuner loop with the planted head walks that tree, every score at least 0.1 from Tz
        Bhis = cap_runs[name][0]
        assert Bhis.shape[0] == c["his"]
        assert np.abs(Bhis[1:, 4] - R.TZ).min() >= 0.1
        off = np.cumsum([0] + c["P"])
        for l in range(1, 6):
            assert int((Bhis[off[l]:off[l + 1], 4] >= R.TZ).sum()) == c["PZ"][l]
    assert cases["his_at"]["his"] == cap < cases["his_past"]["his"]                      # ... and only the history does not
    a, b = T.mask_of_case(cases["his_at"]), T.mask_of_case(cases["his_past"])
    assert (a != b).sum() == 1 and cases["his_at"]["P"][:5] == cases["his_past"]["P"][:5]


# -------------------------------------------------------------------------------------------- the tuner's loop on the CPU
def _small(H, W, scale, seed=6):
    from aznet_hip import synth
    head = synth.make_head(seed=77, **synth.SMALL_DIMS)
    fh, fw = R.map_size(H, W, scale)
    return _cpu_net(head, synth.make_feature_map(seed, synth.SMALL_DIMS["C"], fh, fw))


def test_level_counts_of_the_two_loops():
    assert [orc.num_levels(s, 999) for s in (10, 16, 19, 20, 39, 40)] == [1, 1, 1, 2, 2, 3]
    for (H, W) in T.LEVEL_SHAPES:
        K = orc.num_levels(H, W)
        net = _small(H, W, T.shape_scale(H, W))
        Bhis = orc.im_propose_tune(net, (H, W), T.shape_scale(H, W), orc.OracleCfg(Tz=0.0, NUM_PROPOSALS=300))[1]
        sizes = T.level_sizes(Bhis)
        assert len(sizes) == K and sizes[0] == 1 and all(s > 0 for s in sizes)
    assert [orc.num_levels(H, W) for H, W in T.LEVEL_SHAPES[:2]] == [1, 2]


def test_root_below_tz_still_divides_in_the_tuners_loop():
    """No planted cell: every score is below Tz = 0.5.  The tuner judges the root against 0 (it divides, its raw score is
    recorded), the plain search forces it (it divides, the trace holds 1.0): the same two levels by two different rules,
    and the tuner's loop has one level more to give."""
    c = dict(T.cap_cases()["his_at"], runs=[])
    head, fmap, mask = R.case_inputs(c)
    assert not mask.any()
    net = _cpu_net(head, fmap)
    cfg = orc.OracleCfg(Tz=R.TZ, BATCH_SIZE=10000, NUM_PROPOSALS=300)
    Bhis = orc.im_propose_tune(net, (c["H"], c["W"]), c["scale"], cfg)[1]
    tr = orc.im_propose(net, (c["H"], c["W"]), c["scale"], cfg, return_trace=True)[1]
    assert T.tuner_populations(c["H"], c["W"], c["scale"], mask)["P"] == [1, 5, 0, 0, 0, 0]
    assert Bhis.shape[0] == 6 and (Bhis[:, 4] < R.TZ - 0.1).all()
    assert [l["B"].shape[0] for l in tr["levels"]] == [1, 5] and tr["levels"][0]["zoom"][0] == 1.0
    assert np.array_equal(tr["levels"][1]["B"], Bhis[1:, :4])
    assert orc.num_levels(c["H"], c["W"]) == 6                              # the plain loop walks 5 of them


def test_threshold_comparison_is_float64_in_the_reference():
    """Item 3 of the issue, settled: az_forward's zoom scores are float64 (an hstack onto np.zeros((0,))), so
    `np.where(zoom >= Tz)` compares doubles, as the device's `(double)z >= Tz` does.  At Tz = nextafter(float(z_j), 1) the
    oracle drops anchor j -- called with the Python float, no cast -- although a float32 ARRAY compared with that float
    would keep it."""
    H, W = T.THRESH_SHAPE
    scale = T.shape_scale(H, W)
    net = _small(H, W, scale)
    zoom = orc.az_forward(net, (H, W), scale, np.array([[0, 0, W - 1.0, H - 1.0]]), None, orc.OracleCfg(Tz=0.0))[0]
    assert zoom.dtype == np.float64
    Bhis0 = orc.im_propose_tune(net, (H, W), scale, orc.OracleCfg(Tz=0.0, NUM_PROPOSALS=300))[1]
    sizes = T.level_sizes(Bhis0)
    j, zj = T.pick_anchor(Bhis0[:, 4].astype(np.float32), sizes)
    at, past = T.thresholds_at(zj)
    assert isinstance(at, float) and isinstance(past, float) and at < past and np.float32(past) == zj
    assert bool((np.array([zj]) >= past)[0]) and not (float(zj) >= past)     # float32 array vs float64 scalar
    B_at = orc.im_propose_tune(net, (H, W), scale, orc.OracleCfg(Tz=at, NUM_PROPOSALS=300))[1]
    B_past = orc.im_propose_tune(net, (H, W), scale, orc.OracleCfg(Tz=past, NUM_PROPOSALS=300))[1]
    kids = orc.divide_region(Bhis0[j:j + 1, :4], 10)
    assert kids.shape[0] > 0
    assert T.level_sizes(B_at, at)[:3] == [1, sizes[1], kids.shape[0]]
    assert np.array_equal(B_at[1 + sizes[1]:1 + sizes[1] + kids.shape[0], :4], kids)
    assert B_past.shape[0] == 1 + sizes[1]                                    # j no longer divides: the oracle compares doubles
    assert np.array_equal(B_past, Bhis0[:1 + sizes[1]])
