"""CPU: the case builders of tests/eval_edges_cases.py hold what their names promise (so no GPU case passes for the
wrong reason or quietly stops testing its edge), the ranking reference equals a brute-force sort, and both evaluation
restatements run over every case."""
import math

import numpy as np
import pytest

import coco_eval_ref as CR
import eval_edges_cases as E
import voc_eval_ref as VR


# ---------------------------------------------------------------------------------------------------- ranking
def _brute(C, N, score, det_off):
    seg = np.repeat(np.arange(C * N), np.diff(det_off)).tolist()
    key = [(1, 0.0) if math.isnan(v) else (0, -v) for v in score.tolist()]      # -0.0 == 0.0 as tuples compare
    idx = range(len(key))
    return (sorted(idx, key=lambda d: (seg[d], key[d], d)), sorted(idx, key=lambda d: (seg[d] // N, key[d], d)))


@pytest.mark.parametrize("seed", range(4))
def test_sort_chain_equals_brute_force(seed):
    C, N, D = 3, 4, 400
    score = E.special_scores(D, seed)
    assert np.isnan(score).sum() >= 3 and (score == 0).sum() >= 2 and np.signbit(score[score == 0]).any()
    det_off = E.random_offsets(C * N, D, seed)
    by_seg, by_class = E.rank_ref(C, N, score, det_off)
    want_seg, want_class = _brute(C, N, score, det_off)
    assert by_seg.tolist() == want_seg and by_class.tolist() == want_class
    # rank_unit's contract: both are permutations, NaN last within its group
    assert sorted(by_class.tolist()) == list(range(D))


def test_rank_sizes_sit_on_the_constants():
    assert E.RANK_SIZES == [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 10241]
    tiles = lambda D: -(-D // E.VTILE)
    chunks = lambda D: -(-tiles(D) * 256 // E.SCH)
    assert chunks(8192) == 1 and chunks(8193) == 2                       # 4 tiles fill one scan chunk
    assert E.RANK_BIG_D == 8388608 + 2049 and chunks(E.RANK_BIG_D - E.VTILE - 1) == 1024 and chunks(E.RANK_BIG_D) > 1024
    for D in E.RANK_SIZES:
        for p in E.RANK_PATTERNS:
            C, N, s, off = E.rank_size_case(D, p)
            assert s.shape == (D,) and off.shape == (C * N + 1,) and off[0] == 0 and off[-1] == D and (np.diff(off) >= 0).all()
    D = 8193
    assert np.unique(E.scores("distinct", D)).size == D
    assert np.unique(E.scores("quarters", D)).tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert np.unique(E.scores("equal", D)).size == 1
    m = E.scores("mixed_sign", D)
    assert (m < 0).sum() > D // 4 and (m > 0).sum() > D // 4 and np.unique(m).size < D      # both signs, ties


def test_one_byte_scores_differ_in_that_byte_only():
    for byte in range(8):
        s = E.one_byte_scores(byte)
        assert np.isfinite(s).all()
        x = s.view(np.uint64) ^ np.uint64(E.SCORE_BASE_BITS)
        assert (x & ~(np.uint64(255) << np.uint64(8 * byte))).max() == 0
        assert np.unique(s).size == 256                                 # every digit value; ties: the pass must be stable
    assert (E.one_byte_scores(7) < 0).any() and (E.one_byte_scores(7) > 0).any()


def test_special_scores_hold_every_special_value():
    s = E.special_scores()
    z = s[s == 0]
    assert np.signbit(z).sum() >= 6 and (~np.signbit(z)).sum() >= 6
    assert np.isposinf(s).sum() == 6 and np.isneginf(s).sum() == 6 and np.isnan(s).sum() == 18
    assert np.signbit(s[np.isnan(s)]).any() and (~np.signbit(s[np.isnan(s)])).any()
    den = s[(s != 0) & (np.abs(s) < 2.2250738585072014e-308)]
    assert (den > 0).sum() == 12 and (den < 0).sum() == 12


def test_rank_layouts_cross_the_digit_counts():
    nbytes = lambda v: (int(v).bit_length() + 7) // 8                   # bytes_for in az_voc.hip
    want = {(1, 1): (0, 0), (1, 2): (1, 0), (2, 1): (1, 1), (1, 256): (1, 0), (1, 257): (2, 0), (256, 1): (1, 1),
            (257, 1): (2, 2), (3, 100): (2, 1), (300, 3): (2, 2), (65537, 1): (3, 3), (1, 65537): (3, 0)}
    for C, N, D in E.RANK_LAYOUTS:
        assert (nbytes(C * N - 1), nbytes(C - 1)) == want[(C, N)]
        c, n, s, off = E.rank_layout_case(C, N, D)
        assert off.size == C * N + 1 and off[-1] == D == s.size and (np.diff(off) >= 0).all()
    e = E.rank_empty_segment_cases()
    cnt = {k: np.diff(v[3]) for k, v in e.items()}
    assert (cnt["head"][:12] == 0).all() and (cnt["head"][12:] > 0).all()
    assert (cnt["middle"][9:27] == 0).all() and (cnt["middle"][:9] > 0).all() and (cnt["middle"][27:] > 0).all()
    assert (cnt["tail"][22:] == 0).all() and (cnt["tail"][:22] > 0).all()
    assert (cnt["last_only"][:-1] == 0).all() and cnt["last_only"][-1] == 3000


# ---------------------------------------------------------------------------------------------------- VOC
@pytest.mark.parametrize("G", E.VOC_G)
def test_voc_tie_cases_attain_the_maximum_at_both_boxes(G):
    kinds = {"same_lane": False, "low_j_high_lane": False, "across_2048": False}
    for n in E.VOC_N:
        args = E.voc_gt_count_case(G, n)
        C, N, box, conf, doff, gb, gd, goff = args
        assert gb.shape == (G, 4) and box.shape == (n, 4) and (np.diff(conf) < 0).all()
        r = VR.evaluate_flat(*args)
        pairs = E.voc_tie_pairs(G)
        assert pairs
        for a, b in pairs:
            assert gd[a] != gd[b]
            hits = [d for d in range(n) if np.array_equal(box[d], gb[a])]
            assert len(hits) >= 2 and hits[0] < 64
            ov = E.voc_iou(box[hits[0]], gb)
            assert np.nonzero(ov == ov.max())[0].tolist() == [a, b]
            # the first box decides: difficult -> ignored every time; else a true positive, then claimed
            assert [r["match"][d] for d in hits[:2]] == ([0, 0] if gd[a] else [1, -1])
            if (n + 1) // 2 >= 64 and not gd[a]:                        # claimed in one chunk of detections, met in the next
                assert hits[-1] >= 64 and all(r["match"][d] == -1 for d in hits[1:])
            kinds["same_lane"] |= (b - a) % 64 == 0
            kinds["low_j_high_lane"] |= a % 64 > b % 64
            kinds["across_2048"] |= a < 2048 <= b
        if G > 2049:                                                    # a plain box past the register bits, met twice
            far = [j for j in range(2049, G) if not gd[j] and sum(np.array_equal(bx, gb[j]) for bx in box) >= 2
                   and all(j not in p for p in pairs)]
            assert far
            for j in far:
                assert [r["match"][d] for d in range(n) if np.array_equal(box[d], gb[j])][:2] == [1, -1]
    assert kinds["same_lane"] == (G > 64) and kinds["low_j_high_lane"] == (G > 66) and kinds["across_2048"] == (G > 2048)


def test_voc_claim_across_chunks_is_tp_then_fp():
    args = E.voc_claim_across_chunks_case()
    r = VR.evaluate_flat(*args)
    conf = args[3]
    assert (np.diff(conf) < 0).all()                                    # file order is rank order
    m = r["match"]
    assert m[10] == 1 and m[70] == -1 and m[100] == 1 and (np.delete(m, [10, 70, 100]) == -1).all()
    assert np.array_equal(args[2][10], args[2][70])


def test_voc_min_overlap_case_sits_on_the_thresholds():
    args = E.voc_min_overlap_case()
    box, gb = args[2], args[5]
    ov = np.array([E.voc_iou(box[i], gb[i:i + 1])[0] for i in range(len(box))])
    for m in (0.3, 0.5, 0.7, 1.0):
        assert (ov == m).sum() == 1                                     # ov == min_overlap occurs, exactly
    assert np.isneginf(ov).sum() == 1 and (ov == 0.29).sum() + (ov == 0.49).sum() + (ov == 0.69).sum() == 3
    tps = [int((VR.evaluate_flat(*args, min_overlap=m)["match"] == 1).sum()) for m in E.VOC_MIN_OVERLAPS]
    assert tps == [9, 7, 5, 3, 1]


def test_voc_score_edge_case_has_the_values():
    args = E.voc_score_edge_case()
    conf = args[3]
    assert np.isnan(conf).sum() == 1 and np.isposinf(conf).sum() == 1 and (conf < 0).sum() > 5
    z = conf[conf == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()
    for metric in (True, False):
        r = VR.evaluate_flat(*args, metric_07=metric)
        assert (r["match"] == 1).any() and (r["match"] == -1).any()


def test_voc_class_curve_case_has_the_counts_and_the_nans():
    args = E.voc_class_curve_case()
    C, N, box, conf, doff, gb, gd, goff = args
    assert C == len(E.VOC_CURVE_CLASSES)
    r = VR.evaluate_flat(*args)
    sl = {}
    for name, c in E.VOC_CURVE_CLASSES.items():
        lo, hi = int(doff[c * N]), int(doff[(c + 1) * N])
        assert hi - lo == E.VOC_CURVE_COUNTS[name], name
        sl[name] = slice(lo, hi)
        if name.startswith("empty"):
            assert goff[c * N] == goff[(c + 1) * N]
        else:
            assert goff[(c + 1) * N] - goff[c * N] > 0
    assert sorted(E.VOC_CURVE_COUNTS.values())[:8] == [0, 0, 0, 1, 40, 255, 256, 257] and E.VOC_CURVE_CLASSES["empty_end"] == C - 1
    p = r["prec"][sl["nan_lead_300"]]
    assert np.isnan(p[:300]).all() and not np.isnan(p[300:]).any()          # more than one chunk of 256 all NaN
    assert np.isnan(r["prec"][sl["all_difficult"]]).all() and r["npos"][E.VOC_CURVE_CLASSES["all_difficult"]] > 0
    assert (r["match"][sl["all_difficult"]] == 0).all()
    c0 = E.VOC_CURVE_CLASSES["npos0_300"]
    assert r["npos"][c0] == 0 and np.isnan(r["rec"][sl["npos0_300"]]).all() and math.isnan(r["ap_auc"][c0])
    for name in ("n255", "n256", "n257", "n513"):
        m = r["match"][sl[name]]
        assert (m == 1).any() and (m == -1).any() and (m == 0).any(), name


def test_voc_many_segments_exceed_one_pass_of_the_grid():
    C, N, box, conf, doff, gb, gd, goff = E.voc_many_segments_case()
    assert C * N == 20000 > 4096 * (E.VT // E.AZ_WAVE)
    assert 2500 < doff[-1] < 4500 and np.diff(doff)[-1] > 0 and np.diff(goff)[-1] > 0
    r = VR.evaluate_flat(C, N, box, conf, doff, gb, gd, goff)
    tail = r["match"][doff[16384]:]                                     # segments only the second pass reaches
    assert (tail == 1).any() and (tail == -1).any()


# ---------------------------------------------------------------------------------------------------- COCO
def _coco_ref(c):
    return CR.coco_eval(c["n_classes"], c["n_images"], c["det_box"], c["det_score"], c["det_off"], c["gt_box"],
                        c["gt_area"], c["gt_crowd"], c["gt_off"])


@pytest.fixture(scope="module")
def coco_refs():
    """Both restatements run over every COCO case once: a malformed case fails here, not on the GPU machine."""
    cases = E.coco_cases_all()
    assert sorted(cases) == sorted(E.COCO_CASE_NAMES)
    return cases, {k: _coco_ref(c) for k, c in cases.items()}


@pytest.mark.parametrize("G", E.COCO_G)
def test_coco_gt_count_cases(coco_refs, G):
    c, r = coco_refs[0]["gt_%d" % G], coco_refs[1]["gt_%d" % G]
    crowd, small, dups = E.coco_specials(G)
    assert c["gt_box"].shape == (G, 4) and c["det_off"][-1] <= E.MAXDET
    assert c["gt_crowd"].nonzero()[0].tolist() == sorted(crowd) and (c["gt_area"] == 500.0).nonzero()[0].tolist() == sorted(small)
    if G > 66:
        assert max(crowd) >= 64 and max(small) >= 64
    rank = np.argsort(-c["det_score"], kind="stable")
    m = r["dt_match"][0, 0]                                             # area 'all', IoU 0.5
    for a, b in dups:
        assert np.array_equal(c["gt_box"][a], c["gt_box"][b])
        on = [d for d in rank if np.array_equal(c["det_box"][d], c["gt_box"][a])]
        assert [m[d] for d in on] == [b, a, -1]                          # the last box of the highest IoU first
    assert ((63, 64) in dups) == (G >= 65)
    for j in crowd:
        if j >= 64 or G <= 64:
            on = [d for d in range(len(m)) if np.array_equal(c["det_box"][d], c["gt_box"][j])]
            if on:
                assert len(on) >= 3 and all(m[d] == j for d in on)       # a crowd box is matched again and again
                assert (r["dt_ignore"][0, 0][on] == 1).all()
    if G >= 128:
        assert any(j >= 64 and (m == j).sum() >= 3 for j in crowd)
        assert any(j >= 64 and (r["dt_match"][2, 0] == j).any() and
                   (r["dt_ignore"][2, 0][r["dt_match"][2, 0] == j] == 1).all() for j in small)   # ignored in 'medium'


def test_coco_segment_and_chunk_sizes(coco_refs):
    cases, refs = coco_refs
    assert np.diff(cases["segment_sizes"]["det_off"]).tolist() == [99, 100, 101, 164, 165]
    ig = refs["segment_sizes"]["dt_ignore"][0, 0]
    off = cases["segment_sizes"]["det_off"]
    assert [(ig[off[i]:off[i + 1]] == -1).sum() for i in range(5)] == [0, 0, 1, 64, 65]
    c = cases["acc_chunk"]
    N = c["n_images"]
    assert [int(c["det_off"][(k + 1) * N] - c["det_off"][k * N]) for k in range(4)] == [255, 256, 257, 600]
    assert np.diff(c["det_off"]).max() <= E.MAXDET
    p = refs["acc_chunk"]["precision"]
    assert (p > -1).all()
    assert not np.array_equal(p[..., 0], p[..., 1]) and not np.array_equal(p[..., 1], p[..., 2])   # maxDets matter


def test_coco_npig_case_puts_recall_on_thresholds(coco_refs):
    c, r = coco_refs[0]["npig"], coco_refs[1]["npig"]
    N = c["n_images"]
    for k, (npig, tp) in enumerate(sorted(E.COCO_NPIG.items())):
        assert c["gt_off"][(k + 1) * N] - c["gt_off"][k * N] == npig
        assert (r["recall"][:, k, 0, 2] == tp / float(npig)).all()       # every threshold: exact boxes
        assert any(j / float(npig) == t for j in range(1, tp + 1) for t in CR.REC_THRS), npig
        fp = (r["dt_match"][0, 0][c["det_off"][k * N]:c["det_off"][(k + 1) * N]] < 0).sum()
        assert fp == (tp + 1) // 3
    assert 57 / 100.0 < CR.REC_THRS[57]                                  # npig = 100 also ends a hair under a threshold


def test_coco_layout_cases(coco_refs):
    cases, refs = coco_refs
    p = refs["layout_mixed"]["precision"]
    assert (p[:, :, 1] == -1).all() and (p[:, :, 2] == -1).all() and (p[:, :, [0, 4], 0, 2] > -1).all()
    assert (p[:, :, 3, 0] == 0).all() and (refs["layout_mixed"]["recall"][:, 3, 0] == 0).all()   # boxes, no detections
    assert cases["layout_k1"]["n_classes"] == 1 and cases["layout_k257"]["n_classes"] == 257
    p = refs["layout_k257"]["precision"]
    live = [k for k in range(257) if (p[:, :, k] > -1).any()]
    assert live == [0, 1, 128, 255, 256]


# ---------------------------------------------------------------------------------------------------- recall matching
@pytest.mark.parametrize("K", E.RECALL_K)
def test_recall_cases_tie_their_column_maxima(K):
    from oracle import az_oracle as orc
    cand, gt = E.recall_case(K)
    assert gt.shape == (K, 4) and cand.shape[0] >= K
    ov = orc.bbox_overlaps(cand, gt)
    ties = E.recall_ties(K)
    assert (5, 200) in ties and ((2, 256) in ties) == (K > 256) and ((1, 257) in ties) == (K > 257)
    for a, b in ties:
        ca, cb = np.sort(ov[:, a])[::-1], np.sort(ov[:, b])[::-1]
        assert ca[0] == cb[0] == 400.0 / 1200.0 and ov[:, a].argmax() == ov[:, b].argmax()
        assert ca[1] == 0.25 and cb[1] == 0.2 and ca[2] == 0 and cb[2] == 0
    assert np.array_equal(gt[30], gt[31]) and (cand[0] == cand).all(1).sum() == 2
    got = orc.recall_gt_overlaps([cand], [gt])
    assert (got == 0.2).sum() == len(ties) and (got == 0.25).sum() == 0     # the first column of a pair is taken first
