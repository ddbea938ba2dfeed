"""CPU twin of tests/test_gpu_det_infer_edges.py: every reference of tests/det_infer_ref.py against the oracle
(orc.frcnn_forward with the CPU detection head, orc.nms' C walk, pyramid_ref, the recorded g9 / g19 runs), and every case
family against the edge it names -- which clips fire, which chunks hold a duplicate, which levels are chosen, which
transport a total takes, which output sizes are ties."""
import numpy as np
import pytest

import det_infer_ref as D
import pyramid_ref as pr
from helpers import load

from oracle import az_oracle as orc


def _oracle_detect(head, fmap, boxes, scale, dedup, batch, im_hw, eps):
    cfg = orc.OracleCfg(BATCH_SIZE=batch, DEDUP_BOXES=dedup, EPS=eps)
    conv = {"conv5_3": fmap}
    return orc.frcnn_forward({"fc": orc.OracleDetNet(head)}, im_hw, scale, np.asarray(boxes, np.float64), head["Wc"].shape[0],
                             conv, cfg)


def _fmap(C=D.BIAS_DIMS["C"], hw=D.MAP_HW):
    return np.random.RandomState(1).rand(1, C, hw[0], hw[1]).astype(np.float32)


# ---- A --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,scale", D.IMAGES)
def test_clip_family_is_the_oracles_and_hits_every_clip_edge(H, W, scale):
    head = D.clip_head()
    anchors = D.clip_anchors(H, W)
    seen = set()
    for eps in D.EPS:
        s, b, info = D.detect_ref(anchors, scale, 1. / 16., 10000, (H, W), eps, D.bias_rows(head))
        assert len(info["index"]) == len(anchors)                      # no two anchors share a 1/16 cell
        so, bo = _oracle_detect(head, _fmap(), anchors, scale, 1. / 16., 10000, (H, W), eps)
        assert np.array_equal(b, bo) and np.array_equal(s, so.astype(np.float32))
        assert np.array_equal(s, np.full(s.shape, np.float32(1) / np.float32(s.shape[1])))
        raw = info["raw"].reshape(len(anchors), -1, 4)
        lo_x, lo_y, hi_x, hi_y = raw[..., 0] < 0, raw[..., 1] < 0, raw[..., 2] > W - 1, raw[..., 3] > H - 1
        pat = lo_x * 1 + lo_y * 2 + hi_x * 4 + hi_y * 8
        seen |= {("clips", int(p)) for p in np.unique(pat)}
        seen |= {("outside left", bool((raw[..., 2] < 0).any())), ("outside top", bool((raw[..., 3] < 0).any())),
                 ("outside right", bool((raw[..., 0] > W - 1).any())), ("outside bottom", bool((raw[..., 1] > H - 1).any()))}
        if eps == 0:
            seen |= {("on 0", bool((raw[..., 0] == 0).any() and (raw[..., 1] == 0).any())),
                     ("on max", bool((raw[..., 2] == W - 1).any() and (raw[..., 3] == H - 1).any()))}
            assert np.any(anchors[:, 2] == anchors[:, 0])               # width = eps
    for p in (0, 1, 2, 4, 8, 15):
        assert ("clips", p) in seen, p
    for k in ("outside left", "outside top", "outside right", "outside bottom", "on 0", "on max"):
        assert (k, True) in seen, k


@pytest.mark.parametrize("ncls", D.CLASS_COUNTS)
def test_class_family_is_the_oracles_with_distinct_columns(ncls):
    H, W, scale = D.IMAGES[0]
    anchors = D.class_anchors(H, W)
    for log_sizes in (False, True):
        head = D.class_head(ncls, log_sizes)
        s, b, info = D.detect_ref(anchors, scale, 1. / 16., 10000, (H, W), 1e-14, D.bias_rows(head))
        so, bo = _oracle_detect(head, _fmap(), anchors, scale, 1. / 16., 10000, (H, W), 1e-14)
        assert np.array_equal(b, bo)
        assert np.abs(s - so).max() <= 1e-6
        cols = info["raw"].reshape(len(anchors), ncls, 4)
        assert len({tuple(c) for c in cols[0]}) == ncls                 # every class column shows its own deltas
        p64 = np.exp(head["bc"].astype(np.float64) - head["bc"].max())
        assert np.abs(s - p64 / p64.sum()).max() <= 1e-6


def test_chunk_family_has_duplicates_inside_and_across_chunks():
    H, W, scale = D.IMAGES[0]
    kinds = set()
    for batch in D.BATCHES:
        for P in D.chunk_sizes(batch):
            boxes = D.chunk_boxes(P, H, W, scale)
            rois, index, inv = D.unique_rows(boxes, scale, 1. / 16., batch)
            _, ix, iv = D.unique_rows(boxes, scale, 1. / 16., 10 ** 6)
            chunk = np.arange(P) // batch
            for a in range(P):
                for b in range(a):
                    if iv[a] == iv[b]:                                   # one 1/16 cell
                        kinds.add("inside" if chunk[a] == chunk[b] else "across")
                        assert (inv[a] == inv[b]) == (chunk[a] == chunk[b])
                        kinds.add("own anchor" if not np.array_equal(boxes[a], boxes[b]) else "same box")
            oi, ov = [], []
            off = 0
            for s0 in range(0, P, batch):                                # the oracle's dedup, chunk by chunk
                i, v = orc.roi_dedup(orc.get_rois_blob(boxes[s0:s0 + batch], scale), 1. / 16.)
                oi.append(i + s0), ov.append(v + off)
                off += len(i)
            assert np.array_equal(index, np.concatenate(oi)) and np.array_equal(inv, np.concatenate(ov))
    assert kinds == {"inside", "across", "own anchor", "same box"}
    assert D.CAP in D.chunk_sizes(1) and D.chunk_sizes(10000) == [1, D.CAP]


def test_dedup_factor_family():
    boxes = D.overflow_boxes()
    rois, index, inv = D.unique_rows(boxes, 1.0, 1.0, 10000)
    keys = np.round(rois * 1.0).dot(np.array([1, 1e3, 1e6, 1e9, 1e12]))
    assert np.abs(keys).max() < 2.0 ** 53 and np.array_equal(keys, np.rint(keys))
    assert inv[0] == inv[1] and not np.array_equal(boxes[0], boxes[1])     # fields overlap: different boxes, one key
    assert inv[6] == inv[7] and not np.array_equal(boxes[6], boxes[7])     # ... also with a negative field
    assert inv[2] == inv[3] and inv[4] == inv[5]
    assert len(index) == len(boxes) - 4
    assert (keys < 0).sum() >= 2 and np.array_equal(keys[index], np.sort(keys[index]))
    for dd in (0.0, -1.0):
        r, i, v = D.unique_rows(boxes, 1.0, dd, 10000)
        assert np.array_equal(i, np.arange(len(boxes))) and np.array_equal(v, i)
        oi, ov = orc.roi_dedup(orc.get_rois_blob(boxes, 1.0), dd)
        assert np.array_equal(oi, i) and np.array_equal(ov, v)


def test_integer_head_reference_is_the_oracles():
    case = D.int_case(orc)
    assert case["k"] >= 1 and np.abs(case["deltas"]).max() <= 1.0 and np.abs(case["deltas"]).max() > 0.25
    assert np.array_equal(case["deltas"] * 2.0 ** case["k"], np.rint(case["deltas"] * 2.0 ** case["k"]))
    assert len(np.unique(case["deltas"], axis=0)) > 250                   # the deltas vary per roi
    for head, deltas, exact in ((case["zero_sizes"], case["zero_deltas"], True), (case["head"], case["deltas"], False)):
        fn = lambda index, rois_u: (case["p32"][index], deltas[index])    # noqa: E731
        for H, W in (case["im"], (16, 16)):
            s, b, info = D.detect_ref(case["boxes"], 1.0, 1. / 16., 64, (H, W), 1e-14, fn)
            so, bo = _oracle_detect(head, case["fmap"], case["boxes"], 1.0, 1. / 16., 64, (H, W), 1e-14)
            assert np.array_equal(b, bo)
            assert np.abs(so - case["p64"][info["index"]][info["inv"]]).max() <= 1e-6
            if exact:
                assert np.any(info["raw"][:, 0::4] < 0) and np.any(info["raw"][:, 2::4] > W - 1)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_detect_ref_replays_the_recorded_runs(tag):
    g = load("g9_detect_%s.npz" % tag)
    n = int(g["ndet"])
    prob = np.concatenate([g["d%d_cls_prob" % i] for i in range(n)])
    delt = np.concatenate([g["d%d_bbox_pred" % i] for i in range(n)])
    rois_rec = np.concatenate([g["d%d_rois" % i] for i in range(n)])

    def head(index, rois_u):
        assert np.array_equal(rois_u, rois_rec)
        return prob, delt
    s, b, _ = D.detect_ref(g["proposals"], float(g["scale"]), 1. / 16., int(g["batch"]), (int(g["H"]), int(g["W"])), 1e-14, head)
    assert np.array_equal(s, g["scores"])
    np.testing.assert_allclose(b, g["pred_boxes"], rtol=0, atol=1e-6)


# ---- B --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(D.SCALE_SETS))
def test_scale_sets_choose_every_level_and_straddle_every_switch_point(name):
    scales = np.array(D.SCALE_SETS[name])
    assert 1 < len(scales) <= 8
    lv = pr.rois_blob(D.spread_boxes(), scales)[:, 0].astype(int)
    first = sorted({int(np.where(scales == s)[0][0]) for s in scales})        # equal scales: the first wins
    assert sorted(set(lv)) == first
    sw = D.switch_boxes(scales)
    pts = D.switch_points(scales)
    if name == "all_equal":
        assert len(pts) == 0 and sw.shape == (0, 4)
        return
    areas = (sw[:, 2] - sw[:, 0] + 1) * (sw[:, 3] - sw[:, 1] + 1)
    got = pr.rois_blob(sw, scales)[:, 0].astype(int).reshape(len(pts), -1)
    areas = areas.reshape(len(pts), -1)
    for (a, b, A), row, ar in zip(pts, got, areas):
        assert ar[4] == A and np.all(np.diff(ar) > 0) and ar[3] == np.nextafter(A, 0) and ar[5] == np.nextafter(A, np.inf)
        d = np.abs(ar[:, None] * scales[None, :] ** 2 - 224 * 224)
        assert np.array_equal(row, d.argmin(1))
        da, db = d[:, a], d[:, b]
        assert (da < db).any() and (db < da).any()                            # the pair really changes order here
        if min(da.min(), db.min()) == d.min():                                # ... and is the nearest pair: two levels chosen
            assert len(set(row)) >= 2
    adjacent = np.argsort(scales, kind="stable")
    hit = {tuple(sorted((int(x), int(y)))) for row in got for x, y in zip(row[:-1], row[1:]) if x != y}
    for x, y in zip(adjacent[:-1], adjacent[1:]):
        if scales[x] != scales[y]:
            fx, fy = int(np.where(scales == scales[x])[0][0]), int(np.where(scales == scales[y])[0][0])
            assert tuple(sorted((fx, fy))) in hit, (x, y)


def test_recorded_pyramid_cases_and_the_degenerate_areas():
    g = load("g19_pyramid.npz")
    for i in range(int(g["n_cases"])):
        rois, index, inv = D.unique_rows(g["c%d_boxes" % i], g["c%d_scales" % i], float(g["c%d_dedup" % i]), int(g["c%d_batch" % i]))
        assert np.array_equal(rois, g["c%d_rois" % i]) and np.array_equal(index, g["c%d_index" % i])
        assert np.array_equal(inv, g["c%d_inv" % i])
    boxes = D.degenerate_boxes()
    with np.errstate(all="ignore"):
        w, h = boxes[:, 2] - boxes[:, 0] + 1, boxes[:, 3] - boxes[:, 1] + 1
        area = w * h
        assert (area < 0).sum() >= 2 and np.isinf(area).sum() == 1 and np.isnan(area).sum() == 3
        for name in ("three", "descending", "unsorted"):
            scales = np.array(D.SCALE_SETS[name])
            lv = pr.rois_blob(boxes, scales)[:, 0].astype(int)
            # a negative area is nearest 224^2 at the smallest scale; an infinite or NaN area leaves every distance equal
            # (inf) or unordered (NaN): np.argmin gives the first, the kernel's `d < best` never fires -- level 0 both ways
            assert np.all(lv[area < 0] == int(np.argmin(scales)))
            assert np.all(lv[~np.isfinite(area)] == 0)


def test_merge_pair_merges_at_a_sixteenth_and_not_at_one():
    boxes, scales = D.merge_pair(), [1.0, 2.0]
    rois = pr.rois_blob(boxes, scales)
    assert list(rois[:, 0]) == [0, 1, 0, 1]
    assert np.array_equal(rois[0, 1:], rois[1, 1:]) and np.array_equal(rois[2, 1:], rois[3, 1:])
    assert len(D.unique_rows(boxes, scales, 1. / 16., 10000)[1]) == 2
    assert len(D.unique_rows(boxes, scales, 1.0, 10000)[1]) == 4
    assert len(D.unique_rows(boxes, scales, 0.0, 10000)[1]) == 4


# ---- C --------------------------------------------------------------------------------------------------------------------
def test_nms_walk_is_the_oracles_walk():
    rng = np.random.RandomState(7)
    for n in (1, 2, 63, 64, 65, 256, 257, 300):
        for kind in range(5):
            dets = D.nms_case(rng, n, kind)
            assert np.isfinite(dets).all()
            for thresh in (0.0, 0.3, 0.5, 1.0, 1.5):
                assert D.nms_walk(dets, thresh) == D.reference_keep(orc, dets, thresh), (n, kind, thresh)
    d = D.nms_case(np.random.RandomState(8), 100, 0)
    d[:, 4] = np.random.RandomState(8).permutation(100)                        # distinct scores: orc.nms' own order
    assert D.nms_walk(d, 0.4) == orc.nms(d, 0.4)
    assert D.reference_keep(orc, D.nms_none_suppressed(), 0.5) == D.nms_walk(D.nms_none_suppressed(), 0.5)
    assert len(D.nms_walk(D.nms_none_suppressed(), 0.5)) == 256
    assert len(np.unique(D.nms_none_suppressed()[:, 4])) < 256                 # with ties among the kept
    assert len(D.nms_walk(D.nms_all_but_first(), 0.5)) == 1


def test_nms_table_takes_the_transport_it_names():
    tot = {k: D.nms_total(v[0]) for k, v in D.NMS_TABLE.items()}
    assert tot["largest_mapped"] == D.NMS_MAPPED_MAX and tot["one_more"] == D.NMS_MAPPED_MAX + 1
    assert tot["copy_back"] > D.NMS_MAPPED_MAX + 1000 and tot["edges"] < D.NMS_MAPPED_MAX
    assert tot["all_empty"] == 0 and tot["many_small"] < D.NMS_MAPPED_MAX and len(D.NMS_TABLE["many_small"][0]) == 2000
    sizes = [n[1] if isinstance(n, tuple) else n for n in D.EDGE_SIZES]
    assert {0, 1, 2, 63, 64, 65, 128, 255, 256, 257, 300} <= set(sizes) and sizes[0] == 0 and sizes[-1] == 0
    groups = D.nms_groups(*D.NMS_TABLE["edges"])
    assert [g.shape[0] for g in groups] == sizes and all(g.dtype == np.float32 and np.isfinite(g).all() for g in groups)


# ---- D --------------------------------------------------------------------------------------------------------------------
def test_blob_cases_hit_the_sizes_they_name():
    sizes = {(h, w, s): orc.image_blob_size(h, w, s) for h, w, s, _ in D.BLOB_CASES}
    ows = {v[1] for v in sizes.values()}
    assert {255, 256, 257, 512, 513, 1} <= ows and 1 in {v[0] for v in sizes.values()}
    assert sizes[(5, 9, 0.5)] == (2, 4) and sizes[(7, 11, 0.5)] == (4, 6)      # x.5 both ways: to the even neighbour
    assert all((d * 0.5) % 1 == 0.5 for d in (5, 9, 7, 11))
    for h, w, s, _ in D.BLOB_CASES:
        assert sizes[(h, w, s)][0] >= 1 and sizes[(h, w, s)][1] >= 1
    im = D.blob_image(37, 53, "random")
    assert np.array_equal(orc.image_blob(im, D.MEANS, 1.0)[0], (im.astype(np.float32) - D.MEANS).transpose(2, 0, 1))
    # scale 2 and 3: the last taps sit on s == n - 1 with a fraction, which the clamp turns into the edge pixel alone
    for n, s in ((19, 2.0), (13, 3.0)):
        s0, s1, w0, w1 = orc._linear_taps(int(np.rint(n * s)), n, s)
        f = ((np.arange(int(np.rint(n * s))) + 0.5) / s - 0.5).astype(np.float32)
        edge = np.floor(f) == n - 1
        assert np.any(f[edge] > n - 1) and np.all(w1[edge] == 0) and np.all(s0[edge] == n - 1)
        assert np.any(f < 0) and np.all(w1[f < 0] == 0)
    assert set(np.unique(D.blob_image(4, 4, "checker"))) == {0, 255}
