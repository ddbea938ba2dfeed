"""GPU: the evaluation kernels on the edges of their constants (DESIGN, "Evaluation edges") -- az_rank_unit against a
chain of stable NumPy sorts, az_voc_eval / az_coco_eval / az_recall_match against their restatements, on the cases of
tests/eval_edges_cases.py (each checked on the CPU by test_eval_edges_host.py).  Every comparison is exact, but for
ap_auc and the VOC12-metric ap at the rtol = 1e-12 of test_gpu_voc_eval.py."""
import ctypes

import numpy as np
import pytest

import coco_eval_ref as CR
import eval_edges_cases as E
import voc_eval_ref as VR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- ranking
def _rank(ctx, C, N, score, det_off):
    got_seg, got_class = ctx.rank_unit(C, N, score, det_off)
    want_seg, want_class = E.rank_ref(C, N, score, det_off)
    assert np.array_equal(got_seg, want_seg)
    assert np.array_equal(got_class, want_class)


@pytest.mark.parametrize("D", E.RANK_SIZES)
def test_rank_sizes(ctx, D):
    for pattern in E.RANK_PATTERNS:
        _rank(ctx, *E.rank_size_case(D, pattern))


@pytest.mark.parametrize("byte", range(8))
def test_rank_one_key_pass_decides(ctx, byte):
    score = E.one_byte_scores(byte)
    _rank(ctx, 2, 3, score, E.random_offsets(6, score.size, seed=byte))


def test_rank_special_values(ctx):
    score = E.special_scores()
    _rank(ctx, 2, 3, score, E.random_offsets(6, score.size, seed=9))
    _rank(ctx, 1, 1, score, [0, score.size])


@pytest.mark.parametrize("C,N,D", E.RANK_LAYOUTS)
def test_rank_segment_layouts(ctx, C, N, D):
    _rank(ctx, *E.rank_layout_case(C, N, D))


@pytest.mark.parametrize("name", ["head", "middle", "tail", "last_only"])
def test_rank_empty_segments(ctx, name):
    _rank(ctx, *E.rank_empty_segment_cases()[name])


def test_rank_beyond_1024_chunk_sums(ctx):
    """D = 8 388 608 + 2049: 1025 chunk sums, the only size at which k_voc_scan gives a thread more than one."""
    _rank(ctx, *E.rank_big_case())


def test_rank_errors_and_empty(ctx):
    from aznet_hip import ffi
    L, h = ctx.L, ctx.h
    ip, up, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    score = np.array([0.5, 0.25, 0.75])
    a, b = np.full(3, 7, np.uint32), np.full(3, 7, np.uint32)

    def call(doff, C=1, N=2):
        doff = np.asarray(doff, np.int32)
        return L.az_rank_unit(h, C, N, score.ctypes.data_as(dp), doff.ctypes.data_as(ip), a.ctypes.data_as(up),
                              b.ctypes.data_as(up))
    assert call([0, 3, 1]) == ffi.AZ_ERR_INVALID                        # descends
    assert call([1, 2, 3]) == ffi.AZ_ERR_INVALID                        # does not start at 0
    assert call([0, 3, 3], C=-1) == ffi.AZ_ERR_INVALID
    assert call([0, 3, 3], C=65536, N=65536) == ffi.AZ_ERR_CAPACITY
    assert call([0, 0, 0]) == ffi.AZ_OK and (a == 7).all() and (b == 7).all()      # D = 0: nothing touched
    assert L.az_rank_unit(h, 1, 2, None, np.zeros(3, np.int32).ctypes.data_as(ip), None, None) == ffi.AZ_OK
    assert (a == 7).all() and (b == 7).all()
    assert call([0, 1, 3]) == ffi.AZ_OK                                 # the context works afterwards
    assert a.tolist() == [0, 2, 1] and b.tolist() == [2, 0, 1]


# ---------------------------------------------------------------------------------------------------- VOC
def _check(ctx, args, min_overlap=0.5, metric_07=True, rel=1e-12):
    """test_gpu_voc_eval.py's comparison, with min_overlap passed on."""
    got = ctx.voc_eval(*args, min_overlap=min_overlap, metric_07=metric_07)
    want = VR.evaluate_flat(*args, min_overlap=min_overlap, metric_07=metric_07)
    assert np.array_equal(got["match"], want["match"])
    assert np.array_equal(got["npos"], want["npos"])
    assert np.array_equal(got["rec"], want["rec"], equal_nan=True)
    assert np.array_equal(got["prec"], want["prec"], equal_nan=True)
    if metric_07:
        assert np.array_equal(got["ap"], want["ap"], equal_nan=True)
    else:
        np.testing.assert_allclose(got["ap"], want["ap"], rtol=rel, atol=0)
    np.testing.assert_allclose(got["ap_auc"], want["ap_auc"], rtol=rel, atol=0)
    return got


@pytest.mark.parametrize("G", E.VOC_G)
def test_voc_gt_counts_and_first_box_ties(ctx, G):
    for n in E.VOC_N:
        _check(ctx, E.voc_gt_count_case(G, n))


def test_voc_claim_across_detection_chunks(ctx):
    got = _check(ctx, E.voc_claim_across_chunks_case())
    assert got["match"][10] == 1 and got["match"][70] == -1


@pytest.mark.parametrize("min_overlap", E.VOC_MIN_OVERLAPS)
def test_voc_min_overlap(ctx, min_overlap):
    _check(ctx, E.voc_min_overlap_case(), min_overlap=min_overlap)


@pytest.mark.parametrize("metric_07", [True, False])
def test_voc_score_edge_values(ctx, metric_07):
    _check(ctx, E.voc_score_edge_case(), metric_07=metric_07)


@pytest.mark.parametrize("metric_07", [True, False])
def test_voc_class_curves(ctx, metric_07):
    _check(ctx, E.voc_class_curve_case(), metric_07=metric_07)


def test_voc_many_segments(ctx):
    _check(ctx, E.voc_many_segments_case())


def test_voc_arena_reuse(ctx):
    large, small = E.voc_gt_count_case(2112, 129), E.voc_min_overlap_case()
    first = ctx.voc_eval(*large)
    _check(ctx, small)
    third = ctx.voc_eval(*large)
    assert sorted(first) == sorted(third)
    for key in first:
        assert np.array_equal(first[key].view(np.uint8), third[key].view(np.uint8)), key


# ---------------------------------------------------------------------------------------------------- COCO
def _run(ctx, c):
    return ctx.coco_eval(c["n_classes"], c["n_images"], c["det_box"], c["det_score"], c["det_off"], c["gt_box"],
                         c["gt_area"], c["gt_crowd"], c["gt_off"], want_matches=True)


def _ref(c):
    return CR.coco_eval(c["n_classes"], c["n_images"], c["det_box"], c["det_score"], c["det_off"], c["gt_box"],
                        c["gt_area"], c["gt_crowd"], c["gt_off"])


def _same(got, ref, what):
    """test_gpu_coco_eval.py's comparison: every output, bit for bit."""
    for key in ("precision", "recall", "stats", "dt_match", "dt_ignore"):
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8) if a.dtype == np.float64 else a,
                              b.view(np.uint8) if b.dtype == np.float64 else b), (what, key)


@pytest.fixture(scope="module")
def coco_cases():
    return E.coco_cases_all()


@pytest.mark.parametrize("name", E.COCO_CASE_NAMES)
def test_coco_edges(ctx, coco_cases, name):
    _same(_run(ctx, coco_cases[name]), _ref(coco_cases[name]), name)


# ---------------------------------------------------------------------------------------------------- recall matching
@pytest.mark.parametrize("K", E.RECALL_K)
def test_recall_match_many_boxes(ctx, K):
    from oracle import az_oracle as orc
    cand, gt = E.recall_case(K)
    assert np.array_equal(ctx.recall_match([cand], [gt]), orc.recall_gt_overlaps([cand], [gt]))


def test_recall_match_images_of_every_size_in_one_call(ctx):
    from oracle import az_oracle as orc
    cands, gts = zip(*[E.recall_case(K) for K in E.RECALL_K])
    assert np.array_equal(ctx.recall_match(list(cands), list(gts)), orc.recall_gt_overlaps(list(cands), list(gts)))
