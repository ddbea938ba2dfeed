"""CPU: the conditions that tests/test_gpu_det_edges.py relies on, asserted on the references alone (the cases are built in
tests/det_edges_ref.py), and the restatement tests/det_train_ref.py against what the REFERENCE recorded for the new target
and statistics cases (tests/golden/g22_train_det_edges.npz, written by tests/gen_golden_train_det.py --edges).

1. The exact softmax rows: exp(-203.5) is 0 in float32, p is 1 / k or 0 and sums to exactly 1, d = (p - onehot) / R has no
   rounding, the k columns reach every lane group, the labels every lane group; the random rows span +-30 with float32 gates
   equal to float64's.
2. The size case: every partial sum below 2^24, the float32 restatement equal to float64, bbox_pred's product the slab size.
3. The restatement off its defaults: a zero ratio ignores its mask, lr_mult 0 freezes a blob AND keeps its history zero
   whatever its decay_mult (Caffe multiplies the decayed gradient by the local rate), RefTrajectory carries both; the edited
   train nets read back as written.
5. The hostile target set: offsets, the tie at the threshold and the boxes next to it, the first maximum among three
   identical objects, degenerate boxes, large coordinates; the statistics cases: nan, tiny and positive stds where the GPU
   test expects them."""
import os

import numpy as np
import pytest

import det_edges_ref as E
import det_step_ref as D
import det_train_ref as DR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g22_train_det_edges.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. softmax ------------------------------------------------------------------------------------------------------------
def test_exact_rows_are_exact():
    assert np.exp(np.float32(-203.5)) == 0 and np.exp(np.float32(-203.5)).dtype == np.float32
    assert E.COLD - E.HOT == np.float32(-203.5)
    cases = E.exact_cases()
    assert len(cases) == 35 and (2, 4) not in cases
    seen_labels, seen_rows, kinds = set(), set(), set()
    for ncls, k in cases:
        bias, labels, p, d = E.exact_case(ncls, k)
        hot = E.hot_columns(ncls, k)
        R = labels.size
        x = np.tile(bias, (R, 1))
        l32, d32, p32 = D.softmax_loss(x, labels, np.float32(R))
        l64, d64, p64 = D.softmax_loss(x.astype(np.float64), labels, float(R))
        assert p32.dtype == np.float32 and same(p32, p) and same(d32, d), (ncls, k)
        assert np.all(p32.sum(axis=1) == 1) and np.all(p32.astype(np.float64).sum(axis=1) == 1.0)
        assert set(np.unique(p32)) <= {np.float32(0), np.float32(1) / np.float32(k)}
        assert np.abs(d64 - d).max() < 1e-80 and np.abs(p64 - p).max() < 1e-80       # (float64 keeps exp(-203.5) = 4e-89)
        assert np.isfinite(l32) and abs(l32 - l64) <= 1e-5 * max(1.0, abs(l64))
        groups = set(c // 64 for c in hot)
        if k == 4:                                                   # one column in every lane group that exists
            assert groups == set(range(E.lane_groups(ncls))), (ncls, hot)
        if k == 2 and ncls > 64:                                     # either side of the highest boundary
            assert hot[0] % 64 == 63 and hot[1] == hot[0] + 1
        if k == 1:
            assert hot == [ncls - 1]
        for l in labels.astype(int):
            kinds.add(("hot" if l in hot else "cold", l // 64))
        seen_labels |= set(labels.astype(int).tolist())
        seen_rows.add(R)
    for ncls in E.SM_NCLS:                                           # over the k of an ncls: every group that exists
        cols = set(c // 64 for k in E.SM_K if k <= ncls for c in E.hot_columns(ncls, k))
        assert cols == set(range(E.lane_groups(ncls))), ncls
    assert seen_rows == set(E.SM_ROWS)
    for q in range(4):                                               # labels in every lane group, on a 3.5 and on a -200 column
        assert ("hot", q) in kinds and ("cold", q) in kinds, (q, sorted(kinds))
    assert {0, 255, 64, 128, 192} <= seen_labels and any(64 <= l < 128 for l in seen_labels)
    # two placements spelled out
    assert E.hot_columns(256, 4) == [0, 127, 128, 255] and set(E.hot_columns(65, 4)) >= {0, 63, 64}


@pytest.mark.parametrize("ncls", E.SMR_NCLS)
def test_random_rows_span_and_gates(ncls):
    for rows in E.SMR_ROWS:
        head, fmap, blobs, pool, seed = E.random_case(ncls, rows)
        assert pool.shape == (rows, 196) and fmap.shape == E.SMR_MAP and blobs["labels"].shape == (rows,)
        r64 = D.step(head, pool, blobs, None, want_dpool=False)
        r32 = D.step(head, pool, blobs, None, dtype=np.float32, want_dpool=False)
        for t, _, _ in D.LAYERS:
            assert D.gate_mismatch(r32["pre%d" % t], r64["pre%d" % t]) == 0.0, (ncls, rows, t)
        span = float(np.abs(r64["cls_score"] - head["bc"]).max())
        print("ncls %d, R %d: seed %d, logits in [%.2f, %.2f]" % (ncls, rows, seed, r64["cls_score"].min(), r64["cls_score"].max()))
        assert abs(span - E.SMR_SPAN) < 0.01
        # the GPU test's 1e-6 on p is on the SAME float32 logits: NumPy's float32 arithmetic keeps it
        x = r32["cls_score"]
        p32, p64 = D.softmax_loss(x, blobs["labels"], np.float32(rows))[2], D.softmax_loss(x.astype(np.float64), blobs["labels"], float(rows))[2]
        assert np.abs(p32 - p64).max() <= 1e-6
        if rows > 1:
            assert blobs["labels"][0] == ncls - 1 and blobs["labels"][-1] == 0


# ---- 2. the size contract ----------------------------------------------------------------------------------------------------
def test_size_case_is_exact_in_float32():
    head, fmap, blobs, pool = E.size_case()
    S = E.SIZE
    assert pool.shape == (4096, 196) and S["R"] * 4 * S["ncls"] == 4 << 20 and fmap.shape == (2, 4, 12, 16)
    assert blobs["bbox_targets"].shape == (4096, 1024) and set(blobs["rois"][:, 0]) == {0.0, 1.0}
    r64 = D.step(head, pool, blobs, None, want_dpool=False)
    for nm, worst in E.partial_sum_bounds(head, pool, r64):
        print("  %s: largest possible |partial sum| %.0f (2^24 = %d)" % (nm, worst, 2 ** 24))
        assert worst < 2 ** 24
    r32 = D.step(head, pool, blobs, None, dtype=np.float32, want_dpool=False)
    for nm in ("pre6", "pre7", "cls_score", "bbox_pred"):
        assert r32[nm].dtype == np.float32 and np.array_equal(r32[nm], r64[nm]), nm
    assert np.abs(r64["cls_score"]).max() > 8 and np.abs(r64["bbox_pred"]).max() > 8
    assert len(set(blobs["labels"].tolist())) > 200 and blobs["labels"].max() == 255


# ---- 3. hyper-parameters -----------------------------------------------------------------------------------------------------
def test_dropout_scale_of_the_float32_ratio():
    for r in (0.3, 0.6, 0.25, 0.9, 0.8, 0.5):
        assert np.float32(1.0 / (1.0 - float(np.float32(r)))) == E.f32_scale(r), r
    x = np.array([[1.0, 3.0] + [0.0] * 194], np.float32)
    head = D.filler_head(1, 4, 4, 4, 2)
    head["W6"][:] = 0
    head["W6"][0, 0] = head["W6"][1, 1] = 1
    head["b6"][:] = 0
    blobs = dict(labels=np.zeros(1), bbox_targets=np.zeros((1, 8)), bbox_loss_weights=np.zeros((1, 8)))
    keep = {t: np.ones((1, 4), np.uint8) for t in (6, 7)}
    for dt in (np.float32, np.float64):
        a6 = D.step(head, x, blobs, keep, dtype=dt, ratios=(0.3, 0.5))["a6"]
        assert np.array_equal(a6.astype(np.float32)[0, :2], x[0, :2] * E.f32_scale(0.3))


@pytest.mark.parametrize("name", E.HYPER_HEADS)
@pytest.mark.parametrize("ratios", E.RATIO_SETS, ids=lambda r: "-".join("%g" % x for x in r))
def test_restatement_with_other_hyper_parameters(ratios, name):
    head, fmap, blobs = D.case(name)
    pool, _ = D.roi_pool(fmap, blobs["rois"])
    n = pool.shape[0]
    masks = D.step_masks(3, 1, n, head, ratios)
    assert sorted(masks) == [t for t, l, _ in D.LAYERS if ratios[l] > 0]
    r64 = D.step(head, pool, blobs, masks, ratios=ratios, want_dpool=False)
    r32 = D.step(head, pool, blobs, masks, dtype=np.float32, ratios=ratios, want_dpool=False)
    for t, l, _ in D.LAYERS:
        frac = D.gate_mismatch(r32["pre%d" % t], r64["pre%d" % t])
        print("%s, ratios %s, layer %d: %.3g of the float32 gates differ from float64" % (name, ratios, t, frac))
        assert frac <= 1e-4
        relu = np.maximum(r64["pre%d" % t], 0)
        if ratios[l] == 0:
            assert np.array_equal(r64["a%d" % t], relu)
        else:
            sc = 1.0 / (1.0 - float(np.float32(ratios[l])))
            assert np.array_equal(r64["a%d" % t], np.where(masks[t] > 0, relu * sc, 0))
    junk = dict(masks)
    junk.update({t: np.zeros_like(r64["pre%d" % t], dtype=np.uint8) for t, l, _ in D.LAYERS if ratios[l] == 0})
    again = D.step(head, pool, blobs, junk, ratios=ratios, want_dpool=False)
    assert all(np.array_equal(again["grads"][k], r64["grads"][k]) for k in D.KEYS)
    if ratios[0] > 0 and ratios[1] > 0:                             # the same masks with the two scales swapped: told apart
        swapped = D.step(head, pool, blobs, masks, ratios=ratios[::-1], want_dpool=False)
        assert not np.array_equal(swapped["d_pre7"], r64["d_pre7"])
    assert np.all(r64["losses"] > 0) and all(np.abs(r64["grads"][k]).max() > 0 for k in D.KEYS)


def test_multipliers_and_the_frozen_layer():
    """fc7 with lr_mult 0 / 0 and its decay_mult left at 1 / 0: in Caffe's rule h = momentum h + (rate lr_mult) (clip g +
    decay w) the local rate multiplies the decay too, so the history stays zero and no bit of W7 or b7 moves -- computed
    here, not assumed."""
    head, fmap, blobs = D.case("voc")
    pool, _ = D.roi_pool(fmap, blobs["rois"])
    r64 = D.step(head, pool, blobs, D.step_masks(3, 0, pool.shape[0], head), want_dpool=False)
    lr, dc = E.hyper_multipliers()
    assert lr["Wc"] == float(np.float32(0.1)) and lr["W7"] == lr["b7"] == 0 and lr["bb"] == 3 and dc["b6"] == 1 and dc["Wb"] == 0
    assert dc["W7"] == 1 and dc["b7"] == 0
    zeros = {k: np.zeros_like(v) for k, v in head.items()}
    for dt in (np.float32, np.float64):
        p, h = D.sgd(head, r64["grads"], zeros, 0.001, 0.9, 0.0005, 0.5, dtype=dt, lr_mult=lr, decay_mult=dc)
        p, h = D.sgd(p, r64["grads"], h, 0.001, 0.9, 0.0005, 1.0, dtype=dt, lr_mult=lr, decay_mult=dc)
        for k in ("W7", "b7"):
            assert np.array_equal(p[k], head[k]) and not h[k].any()
        assert all(not np.array_equal(p[k], head[k]) for k in D.KEYS if k not in ("W7", "b7"))
    q, _ = D.sgd(head, r64["grads"], zeros, 0.001, 0.9, 0.0005, 0.5, lr_mult=D.LR_MULT, decay_mult=D.DECAY_MULT)
    p, _ = D.sgd(head, r64["grads"], zeros, 0.001, 0.9, 0.0005, 0.5, lr_mult=lr, decay_mult=dc)
    assert not np.array_equal(p["b6"], q["b6"]) and not np.array_equal(p["Wb"], q["Wb"]) and np.array_equal(p["W6"], q["W6"])
    assert not np.array_equal(p["Wc"], q["Wc"]) and not np.array_equal(p["bb"], q["bb"])


def test_front_door_rows_and_trajectory(tmp_path):
    from detect import prototxt as P
    D.traj_solver_files(str(tmp_path), True, E.front_door_rows)
    net = P.read_det_train_net(str(tmp_path / "train_det.prototxt"))
    assert [net[k]["dropout_ratio"] for k in P.DET_HEAD_LAYERS] == [0.3, None, None, None]
    assert net["fc7"]["lr_mult"] == [0.0, 0.0] and net["fc6"]["lr_mult"] == [1.0, 2.0] and net["fc7"]["decay_mult"] == [1.0, 0.0]
    assert all(net[k]["lr_mult"] == [0.0, 0.0] for k in P.CONV_LAYERS)
    # the net of the run with training convolutions: conv1_1 .. conv2_2 frozen, the rest 1 / 2
    D.traj_solver_files(str(tmp_path), False)
    net = P.read_det_train_net(str(tmp_path / "train_det.prototxt"))
    assert [k for k in P.CONV_LAYERS if max(net[k]["lr_mult"]) > 0] == list(P.CONV_LAYERS[4:])
    assert [net[k]["dropout_ratio"] for k in P.DET_HEAD_LAYERS] == [0.5, 0.5, None, None]
    # RefTrajectory carries the ratios and the multipliers
    head, fmap, blobs = D.case("voc")
    lr, dc = E.front_door_multipliers()
    ref = D.RefTrajectory(head, np.float64, D.TRAJ["solver"], ratios=E.FRONT_DOOR["ratios"], lr_mult=lr, decay_mult=dc)
    base = D.RefTrajectory(head, np.float64, D.TRAJ["solver"])
    for _ in range(2):
        r, b = ref.step(fmap, blobs, 3), base.step(fmap, blobs, 3)
    assert np.array_equal(r["a7"], np.maximum(r["pre7"], 0)) and not np.array_equal(b["a7"], np.maximum(b["pre7"], 0))
    assert np.array_equal(ref.p["W7"], head["W7"]) and np.array_equal(ref.p["b7"], head["b7"]) and ref.it == 2
    assert all(not np.array_equal(ref.p[k], head[k]) for k in D.KEYS if k not in ("W7", "b7"))
    assert not np.array_equal(base.p["W7"], head["W7"])


# ---- 5. targets and statistics -------------------------------------------------------------------------------------------------
def test_offsets_case_is_hostile():
    ex, gt, lab = E.offsets_case()
    off = E.offsets_of(ex)
    assert off.tolist() == [0, 0, 3, 3, 3, 258, 259, 516, 516] and E.offsets_of(gt).tolist() == [0, 2, 2, 3, 6, 76, 77, 82, 82]
    assert off[4] < 256 < off[5] and off[6] < 512 < off[7]           # block boundaries inside images 4 and 6
    e4, g4, l4 = ex[4], gt[4], lab[4]
    ov = DR.iou_matrix(e4, g4)
    assert tuple(e4[0]) == E.TIE_BOX and tuple(g4[0]) == E.TIE_OBJECT and ov[0, 0] == 0.25 and ov[0].max() == 0.25
    assert 0.2499 < ov[1].max() < 0.25 < ov[2].max() < 0.2501 and ov[1].argmax() == 0 and ov[2].argmax() == 0
    a = E.TWIN_AT
    assert np.array_equal(g4[a], g4[a + 1]) and np.array_equal(g4[a], g4[a + 2]) and tuple(l4[a:a + 3]) == E.TWIN_CLASSES
    twins = np.where((ov[:, a] == ov.max(axis=1)) & (ov[:, a] >= 0.25))[0]
    assert twins.size >= 10 and ov[3, a] == 1.0
    for key, s in E.TARGET_SETTINGS.items():
        ref = E.reference_targets(key)
        t4, mo4 = ref[4]
        assert [r[0].shape[0] for r in ref] == list(E.EX_COUNTS)
        assert not ref[1][0].any() and np.all(ref[1][1] == float(np.float32(s["bg_lo"])))          # boxes without objects
        if s["bbox_thresh"] == 0.25:
            assert set(t4[twins, 0]) == {float(E.TWIN_CLASSES[0])}                               # the FIRST maximum's class
            assert t4[0, 0] == 2 and t4[1, 0] == 0 and t4[2, 0] == 2                               # at, below and above the tie
            pos = t4[:, 0] > 0
            thin_ex = (e4[:, 2] - e4[:, 0] < 1) | (e4[:, 3] - e4[:, 1] < 1)
            assert (pos & thin_ex).sum() >= 4 and set(t4[pos & thin_ex, 0]) >= {3.0, 7.0}
            assert (pos & (e4[:, 0] > 9000)).sum() >= 3 and set(t4[pos & (e4[:, 0] > 9000), 0]) >= {6.0, 8.0}
            assert (ref[6][0][:, 0] > 0).sum() > 50 and ref[5][0][0, 0] == 11
        else:
            assert 0 < (t4[:, 0] > 0).sum() < 40
    ta, tb = E.reference_targets("a")[4][0], E.reference_targets("b")[4][0]
    assert np.array_equal(ta[:, 0], tb[:, 0])
    print("eps 0 against 1e-14: %d of %d target values differ" % (int((ta != tb).sum()), ta.size))


def test_target_restatement_equals_reference(g):
    """Every image of the set under every setting, images without example boxes included: the reference ran all of them."""
    for key in E.TARGET_SETTINGS:
        for i, (t, mo) in enumerate(E.reference_targets(key)):
            assert same(t, g["t%s%d_targets" % (key, i)]), (key, i)
            want = g["t%s%d_max_overlaps" % (key, i)]
            assert want.dtype == (np.float32 if E.GT_COUNTS[i] == 0 else np.float64)
            assert same(mo, want.astype(np.float64)), (key, i)


@pytest.mark.parametrize("ncls", E.STATS_NCLS)
def test_stats_cases_and_reference(g, ncls):
    raw = E.stats_case(ncls)
    counts, means, stds, norm = E.reference_stats(ncls)
    assert len(raw) == E.STATS_IMAGES[ncls] and raw[-2].shape[0] == 0 and stds.shape == (ncls, 4)
    assert E.same_or_both_nan(means.ravel(), g["s%d_means" % ncls]) and E.same_or_both_nan(stds.ravel(), g["s%d_stds" % ncls])
    assert E.same_or_both_nan(norm, g["s%d_norm" % ncls])
    allr = np.vstack(raw)
    labels = allr[:, 0]
    assert (labels >= ncls).sum() >= 3 and (labels == 2.5).sum() == 1 and (labels == -1).sum() == 1 and (labels == 0).sum() >= 10
    ignored = ~((labels >= 1) & (labels < ncls) & (labels == np.floor(labels)))
    assert same(norm[ignored], allr[ignored])                        # rows of no class come back untouched
    S = E.STAT_CLASS
    per_image = lambda c: [int((t[:, 0] == c).sum()) for t in raw]
    assert all(n > 0 for i, n in enumerate(per_image(S["spread"])) if i != len(raw) - 2)
    print("%d classes: %d nan stds, %d finite stds below 1e-6, %d classes without a row"
          % (ncls, int(np.isnan(stds).sum()), int((stds < 1e-6).sum()), int((counts[1:] < 0.5).sum())))
    assert np.all(np.isfinite(stds[S["spread"]])) and np.all(stds[S["spread"]] > 0.05)
    if ncls == 2:
        return
    assert sum(per_image(S["one_row"])) == 1 and max(per_image(S["four_same"])) == 4 and sum(per_image(S["no_row"])) == 0
    assert sorted(per_image(S["two_and_two"]))[-2:] == [2, 2] and sorted(per_image(S["one_image"]))[-2:] == [0, 10]
    assert counts[S["no_row"]] == DR.EPS and not means[S["no_row"]].any() and not stds[S["no_row"]].any()
    assert np.isnan(stds).any(), "no nan std"
    tiny = np.isfinite(stds[1:]) & (stds[1:] < 1e-6) & (counts[1:, None] > 0.5)
    assert tiny.any(), "no zero or tiny std"
    for c in (S["one_dyadic"], S["four_dyadic"]):                    # no rounding in sums or squares: a tiny positive variance
        assert np.all(stds[c] > 0) and np.all(stds[c] < 1e-6)
        assert np.all(np.isfinite(norm[allr[:, 0] == c, 1:]) | np.isinf(norm[allr[:, 0] == c, 1:]))
    for c in range(1, ncls):                                         # two or more distinct rows: a finite std > 0
        rows = allr[labels == c, 1:]
        if np.unique(rows, axis=0).shape[0] >= 2:
            assert np.all(np.isfinite(stds[c])) and np.all(stds[c] > 0), c
    single = [c for c in range(9, ncls) if (labels == c).sum() == 1]
    nan_single = sum(bool(np.isnan(stds[c]).any()) for c in single)
    print("  %d of %d single-row classes from 9 on have a nan std" % (nan_single, len(single)))
    # a second run of the yardstick gives the same bits (it is the GPU test's reference, computed once there)
    again = E.reference_stats(ncls)
    assert all(E.same_or_both_nan(a, b) for a, b in zip((counts, means, stds, norm), again))
