"""CPU: the references and case generators of tests/select_ref.py, which tests/test_gpu_select_edges.py holds the selection
and decode kernels against -- the references reproduce the g4 / g8 goldens and the oracle's own decode, and every generator
meets the conditions it states (no NaN, no -0.0, the bits and ties where it says, the near-threshold share under its cap)."""
import numpy as np
import pytest

import select_ref as S
from helpers import load


# ------------------------------------------------------------------------------------------------------- references
def test_topk_ref_reproduces_golden_g8():
    """Under the rules test_topk_golden_g8 states: NumPy's order inside a tie is unspecified, so the score sequence agrees,
    the index set above the last selected score agrees, and tie groups above the cut select the same boxes."""
    g = load("g8_topk.npz")
    for tag in [str(t) for t in g["runs"]]:
        neg, indA, Yall, Y = g[tag + "_neg_scores"], g[tag + "_indA"], g[tag + "_Y_all"], g[tag + "_Y"]
        k = int(g[tag + "_num_proposals"])
        sc = (-neg).astype(np.float32)
        assert np.array_equal(sc.astype(np.float64), -neg)
        idx = S.topk_ref(sc, k)
        n = min(k, sc.shape[0])
        assert idx.shape == (n,)
        assert np.array_equal(neg[idx], neg[indA[:n]]), tag
        cut = neg[indA[n - 1]]
        assert set(idx[neg[idx] < cut].tolist()) == set(indA[:n][neg[indA[:n]] < cut].tolist()), tag
        for v in np.unique(neg[indA[:n]]):
            if v == cut:
                continue
            a = Yall[idx[neg[idx] == v]]
            b = Y[neg[indA[:n]] == v]
            assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]), tag
        # the stated equivalence: no NaN, no -0.0 -> the stable sort of the negated values
        assert np.array_equal(idx, np.argsort(-sc.astype(np.float64), kind="stable")[:n])


def test_decode_filter_ref_reproduces_golden_g4():
    g = load("g4_decode.npz")
    b, s, margin = S.decode_filter_ref(g["boxes"], g["deltas"], g["scores"], 600, 1000, 1e-14, 10)
    assert np.array_equal(S.decode_raw(g["boxes"], g["deltas"], 1e-14).reshape(200, 44), g["pred"])
    assert np.array_equal(S.decode_clipped(g["boxes"], g["deltas"], 600, 1000, 1e-14).reshape(200, 44), g["clipped"])
    assert np.array_equal(b, g["unwrap_boxes"]) and np.array_equal(s, g["unwrap_scores"])
    assert margin.shape == (200 * 11,) and int((margin >= 0).sum()) == b.shape[0]


def _oracle_decode(case):
    from oracle import az_oracle as orc
    a, d = case["anchors"], case["deltas"]
    pred = orc.clip_boxes(orc.bbox_pred(a, d, case["eps"]), (case["im_h"], case["im_w"]))
    return orc.unwrap_adj_pred(pred, case["scores"], case["min_side"])


def _decode_cases():
    out = []
    for i, (h, w) in enumerate(S.IMAGES):
        for j, ms in enumerate(S.MIN_SIDES):
            out.append(S.clip_case(h, w, S.EPSS[(i + j) % 3], ms))
    out += [S.min_side_case(ms)[0] for ms in S.MIN_SIDES]
    for i, R in enumerate(S.DECODE_ROWS[1:-1]):
        out.append(S.rows_case(R, S.KEEP_PATTERNS[i % len(S.KEEP_PATTERNS)], *S.rows_settings(i)))
    out += [S.random_case(*c) for c in S.RANDOM_CASES]
    return out


def test_decode_filter_ref_agrees_with_the_oracle():
    for case in _decode_cases():
        b, s, _ = S.case_ref(case)
        ob, os_ = _oracle_decode(case)
        assert np.array_equal(b, ob) and np.array_equal(s, os_)


def test_thresh_ref_is_a_double_compare():
    s = np.array([0.1, 0.7, 0.7, 0.3], dtype=np.float32)
    t = np.float64(s[1])
    assert S.thresh_ref(s, t).tolist() == [1, 2]
    assert S.thresh_ref(s, np.nextafter(t, np.inf)).tolist() == []
    assert S.thresh_ref(s, 0.7).tolist() == []                  # 0.7 as a double lies above float32(0.7)
    assert S.thresh_ref(s, 0.0).tolist() == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------- top-k generators
def _all_topk_cases():
    for p in S.TOPK_PATTERNS:
        for n, k, seed in S.pattern_cases(p):
            yield p, n, k, seed
    for i, n in enumerate(S.topk_sizes()):
        if n > S.RANK_MAX_N + 1025:
            continue                                            # (the capacity-sized vectors: same generators, checked below)
        for p in S.SIZE_PATTERNS:
            yield p, n, 300, 2000 + i


def test_topk_patterns_hold_no_nan_and_no_negative_zero():
    count = 0
    for p, n, k, seed in _all_topk_cases():
        s = S.topk_scores(p, n, k, seed)
        assert s.dtype == np.float32 and s.shape == (n,)
        assert not np.isnan(s).any(), p
        assert not (s.view(np.uint32) == np.uint32(0x80000000)).any(), p
        assert np.array_equal(S.topk_ref(s, k), np.argsort(-s.astype(np.float64), kind="stable")[:min(k, n)]), (p, n, k)
        count += 1
    assert count > 300
    n = S.DEFAULT_MAX_CANDIDATES
    for p in S.SIZE_PATTERNS:
        s = S.topk_scores(p, n, 300, 7)
        assert not np.isnan(s).any() and not (s.view(np.uint32) == np.uint32(0x80000000)).any()
    assert set(p for p, _, _, _ in _all_topk_cases()) == set(S.TOPK_PATTERNS)


@pytest.mark.parametrize("pattern", sorted(S.KEY_BIT_RANGES))
def test_one_radix_pass_decides(pattern):
    """The keys of the pattern differ inside one pass's bits only, take many values there, and (for n above the number of
    values) tie -- so that pass alone finds the cut and the index order settles the rest."""
    lo, hi = S.KEY_BIT_RANGES[pattern]
    for n, k, seed in S.pattern_cases(pattern):
        key = S.score_key(S.topk_scores(pattern, n, k, seed))
        diff = np.bitwise_or.reduce(key ^ key[0])
        inside = np.uint32(((1 << hi) - 1) ^ ((1 << lo) - 1))
        assert diff & ~inside == 0 and diff != 0
        assert np.unique(key).shape[0] > min(n, 1 << (hi - lo)) // 4


def test_two_value_patterns_cut_where_they_say():
    for n, k, seed in S.pattern_cases("two_values_cut_in_lower"):
        s = S.topk_scores("two_values_cut_in_lower", n, k, seed)
        hi = int((s == 0.75).sum())
        assert set(np.unique(s).tolist()) <= {0.25, 0.75}
        if n > k:
            assert hi < k and s[S.topk_ref(s, k)[-1]] == 0.25
    for n, k, seed in S.pattern_cases("two_values_cut_in_upper"):
        s = S.topk_scores("two_values_cut_in_upper", n, k, seed)
        hi = int((s == 0.75).sum())
        if n > k:
            assert k < hi <= n and (hi < n or n == k + 1) and s[S.topk_ref(s, k)[-1]] == 0.75
            assert s[S.topk_ref(s, k)].min() == 0.75


def test_tie_run_straddles_a_per_thread_chunk():
    cases = S.pattern_cases("tie_straddle")
    assert len(cases) >= 12 and any(k == 4096 for _, k, _ in cases) and any(n > S.RANK_MAX_N for n, _, _ in cases)
    for n, k, seed in cases:
        s, start, end, b, g = S.tie_straddle(n, k)
        assert np.array_equal(s, S.topk_scores("tie_straddle", n, k, seed))
        per = S.per_thread_chunk(n)
        assert b % per == 0 and start < b < end and end - start > k            # longer than k, across a chunk boundary
        assert (s[start:end] == 0.5).all() and int((s == 0.5).sum()) == end - start
        assert int((s > 0.5).sum()) == g < k
        idx = S.topk_ref(s, k)
        assert s[idx[-1]] == 0.5 and idx.shape == (k,)                          # the cut is inside the run
        if k >= 4:
            assert idx[-1] >= b and idx[g] < b                                  # ... with selected elements on both sides
        assert np.array_equal(idx[g:], np.arange(start, start + k - g))


def test_special_value_patterns_hold_their_values():
    for n, k, seed in S.pattern_cases("zero_one"):
        s = S.topk_scores("zero_one", n, k, seed)
        assert (s == 0.0).any() and (s == 1.0).any() and s.min() == 0.0 and s.max() == 1.0
    tiny = np.finfo(np.float32).tiny
    for n, k, seed in S.pattern_cases("denormals"):
        s = S.topk_scores("denormals", n, k, seed)
        assert ((s > 0) & (s < tiny)).sum() > n // 2 and (s == 0.0).any() and (s >= tiny).any()
    for n, k, seed in S.pattern_cases("negative_inf"):
        s = S.topk_scores("negative_inf", n, k, seed)
        assert (s == np.inf).any() and (s == -np.inf).any() and (s < 0).sum() > n // 4 and ((s < 0) & (s > -tiny)).any()
    for p, at in (("max_first", 0), ("max_last", -1)):
        for n, k, seed in S.pattern_cases(p):
            s = S.topk_scores(p, n, k, seed)
            assert s[at] == 1.0 and int((s == 1.0).sum()) == 1 and S.topk_ref(s, k)[0] == (n + at) % n
    for n in (257, 70000):
        a = S.topk_scores("ascending", n, 300, 0)
        assert (np.diff(a) > 0).all() and (np.diff(S.topk_scores("descending", n, 300, 0)) < 0).all()


def test_sizes_cross_the_handover_and_reach_the_capacity():
    sizes = S.topk_sizes()
    for n in (S.RANK_MAX_N - 1, S.RANK_MAX_N, S.RANK_MAX_N + 1, S.RANK_MAX_N + 1025, S.DEFAULT_MAX_CANDIDATES, 1, 4096, 4097):
        assert n in sizes
    assert S.DEFAULT_MAX_CANDIDATES == 16384 * 11 and S.TOPK_KS == [1, 2, 300, 4095, 4096]


# --------------------------------------------------------------------------------------------------- decode generators
@pytest.mark.parametrize("im", S.IMAGES)
def test_clip_case_covers_every_clip(im):
    h, w = im
    for eps in S.EPSS:
        case = S.clip_case(h, w, eps, 10.0)
        assert (case["deltas"].reshape(-1, 4)[:, 2:] == 0).all()               # log-size deltas 0: exp is exact
        raw = S.decode_raw(case["anchors"], case["deltas"], eps)
        c = np.stack([raw[:, 0] < 0, raw[:, 1] < 0, raw[:, 2] > w - 1, raw[:, 3] > h - 1], axis=1)
        for q in range(4):                                                      # each clip alone
            only = np.zeros(4, dtype=bool)
            only[q] = True
            assert (c == only).all(axis=1).any(), (im, eps, q)
        assert c.all(axis=1).any() and (~c).all(axis=1).any()                   # all four at once; none
        b = S.decode_clipped(case["anchors"], case["deltas"], h, w, eps)
        assert (b[:, 2] - b[:, 0] + 1 <= 0).any() and (b[:, 3] - b[:, 1] + 1 <= 0).any()   # wholly outside, either axis
        for ms in S.MIN_SIDES:
            kept = S.case_ref(dict(case, min_side=ms))[0].shape[0]
            assert (0 < kept < b.shape[0]) if ms <= min(h, w) else kept == 0    # (no side of 16.5 in a 16 x 16 image)


@pytest.mark.parametrize("min_side", S.MIN_SIDES)
def test_min_side_case_sits_on_the_threshold(min_side):
    case, eq, below = S.min_side_case(min_side)
    b, s, margin = S.case_ref(case)
    side = margin + min_side
    assert (margin[eq] == 0).all() and eq.shape[0] == 22                        # equal on either axis: kept
    assert (side[below] == np.nextafter(np.float64(min_side), -np.inf)).all() and below.shape[0] == 22
    assert np.array_equal(S.survivors(s), eq)
    cl = S.decode_clipped(case["anchors"], case["deltas"], case["im_h"], case["im_w"], 0.0)
    w, h = cl[:, 2] - cl[:, 0] + 1, cl[:, 3] - cl[:, 1] + 1
    assert (w[eq[:11]] < h[eq[:11]]).all() and (h[eq[11:]] < w[eq[11:]]).all()  # the width decides, then the height


def test_rows_cases_keep_what_the_pattern_says():
    for i, R in enumerate(S.DECODE_ROWS):
        if R > 1000:
            continue
        for pattern in S.KEEP_PATTERNS:
            case = S.rows_case(R, pattern, *S.rows_settings(i))
            b, s, margin = S.case_ref(case)
            want = np.where(S.keep_flags(pattern, R * S.NSUB))[0]
            assert np.array_equal(S.survivors(s), want), (R, pattern)
            if R:
                assert np.abs(margin).min() > 0.4                                # far from the threshold on either side
    R = S.DEFAULT_MAX_REGIONS
    case = S.rows_case(R, "block_last", *S.rows_settings(7))
    assert S.case_ref(case)[0].shape[0] == (R * S.NSUB + S.BLOCK - 1) // S.BLOCK
    assert 24 * S.NSUB > S.BLOCK >= 23 * S.NSUB and 94 * S.NSUB > 4 * S.BLOCK >= 93 * S.NSUB
    seen = set(S.rows_settings(i) for i in range(len(S.DECODE_ROWS)))
    assert set(x[3] for x in seen) == set(S.MIN_SIDES) and set(x[2] for x in seen) == set(S.EPSS)
    assert set(x[:2] for x in seen) == set(S.IMAGES)


@pytest.mark.parametrize("spec", S.RANDOM_CASES)
def test_random_cases_stay_clear_of_the_threshold(spec):
    """The share of candidates whose keep / drop decision is not asserted on the GPU (reference margin within 1e-3 px of
    the threshold, where one ulp of the device's expf may decide) is at most 1 % -- by the choice of the seeds."""
    case = S.random_case(*spec)
    b, s, margin = S.case_ref(case)
    d = case["deltas"].reshape(-1, 4)
    assert np.abs(d[:, 2:]).max() > 1.9 and np.abs(d[:, 2:]).max() <= 2.0
    assert float((np.abs(margin) <= S.MARGIN_BAND).mean()) <= S.MARGIN_SHARE
    assert 0.2 < b.shape[0] / float(margin.shape[0]) < 0.98                     # both outcomes are common
    assert S.MARGIN_BAND == 10 * S.BOX_ATOL
