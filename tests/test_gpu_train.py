"""GPU: the training data layer's kernels (csrc/az_train.hip) against what the REFERENCE's own az_data_layer/roidb.py
and minibatch.py recorded (tests/golden/g20_train_roidb.npz) and against the NumPy restatement tests/train_ref.py.

Bounds.  Integer / boolean / index outputs, ex_boxes, the noise consumed, row order, dx, dy and the IoU column: bit-exact
(f64 in the reference's operation order, no FMA).  dw, dh: 4 ulp (f64) -- device log and glibc log are each documented
to <= 1 ulp, so they differ by <= 2; 2 more for a rounding of log near a tie.  means: 1e-12 relative-or-absolute (f64
sums taken in another order); stds: 1e-12 * max(1, E[x^2] / var), the amplification of that error by the subtraction
E[x^2] - mean^2; normalised targets: what those two imply for (x - mean) / std."""
import os

import numpy as np
import pytest

import train_ref as tr
from train_edges_ref import check_stats, check_targets, stat_bounds, ulp_diff      # noqa: F401  (derived above)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_train_roidb.npz")
C = tr.TrainCfg()
TP = dict(C.__dict__)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def case_noise(g, i, extra=0):
    np.random.seed(int(g["c%d_seed" % i]))
    return np.random.random(int(g["c%d_used" % i]) + extra)


def test_zoom_labels_golden(ctx, g):
    for i in range(int(g["n_cases"])):
        got = ctx.zoom_labels(g["c%d_ex_boxes" % i], g["c%d_gt" % i], C.emb_reg_thresh, C.emb_obj_thresh)
        assert np.array_equal(got, g["c%d_zoom_of_ex" % i]), i


def test_ex_rois_golden(ctx, g):
    for i in range(int(g["n_cases"])):
        size = tuple(int(v) for v in g["c%d_size" % i])
        ex, zoom, off, used = ctx.train_ex_rois(TP, [size], [g["c%d_gt" % i]], case_noise(g, i, 7))
        assert int(used[0]) == int(g["c%d_used" % i]), i
        assert np.array_equal(ex, g["c%d_ex_boxes" % i].astype(np.float32)), i
        assert np.array_equal(zoom.astype(bool), g["c%d_zoom_gt" % i]), i
        assert off.tolist() == [0, ex.shape[0]]


def test_adj_targets_golden(ctx, g):
    worst = 0.0
    for i in range(int(g["n_cases"])):
        ex = g["c%d_ex_boxes" % i].astype(np.float32)
        t, toff = ctx.train_adj_targets(TP, ex, [0, ex.shape[0]], [g["c%d_gt" % i].astype(np.float32)])
        assert toff.tolist() == [0, int(g["c%d_ntargets" % i])]
        worst = max(worst, check_targets(t, g["c%d_targets" % i], "case %d" % i))
    print("max |dw, dh| difference to the reference: %.2f ulp" % worst)


def test_target_stats_golden(ctx, g):
    raw = np.ascontiguousarray(np.vstack([g["c%d_targets" % i] for i in range(int(g["n_cases"]))]))
    t = raw.copy()
    m, s = ctx.train_target_stats(11, C.eps, t, True)
    check_stats(m, s, t, g["set_means"].reshape(11, 4), g["set_stds"].reshape(11, 4), raw, g["set_targets"])
    t2 = raw.copy()
    m2, s2 = ctx.train_target_stats(11, C.eps, t2, False)
    assert np.array_equal(t2, raw) and np.array_equal(m2, m) and np.array_equal(s2, s)
    m0, s0 = ctx.train_target_stats(11, C.eps, np.zeros((0, 7)), True)
    assert not m0.any() and not s0.any()


def test_two_images_share_one_stream(ctx, g):
    sizes = [tuple(int(v) for v in g["c%d_size" % i]) for i in (0, 2, 3, 1)]
    gts = [g["c%d_gt" % i] for i in (0, 2, 3, 1)]
    noise = np.random.RandomState(77).random_sample(40000)
    ex, zoom, off, used = ctx.train_ex_rois(TP, sizes, gts, noise)
    at = 0
    for j in range(4):
        e1, z1, o1, u1 = ctx.train_ex_rois(TP, [sizes[j]], [gts[j]], noise[at:])
        assert int(u1[0]) == int(used[j])
        assert np.array_equal(e1, ex[off[j]:off[j + 1]]) and np.array_equal(z1, zoom[off[j]:off[j + 1]])
        at += int(u1[0])
    # ... and the same as the restatement walking one stream
    at = 0
    for j in range(4):
        b, z, u = tr.compute_ex_rois(sizes[j], gts[j], noise[at:], C)
        assert u == int(used[j]) and np.array_equal(b.astype(np.float32), ex[off[j]:off[j + 1]])
        assert np.array_equal(z, zoom[off[j]:off[j + 1]].astype(bool))
        at += u


def test_short_noise_and_cap_are_errors(ctx, g):
    from aznet_hip import ffi
    size, gt = tuple(int(v) for v in g["c0_size"]), g["c0_gt"]
    used, E = int(g["c0_used"]), g["c0_ex_boxes"].shape[0]
    ex, _, _, u = ctx.train_ex_rois(TP, [size], [gt], case_noise(g, 0), cap=E)         # exactly enough of both
    assert ex.shape[0] == E and int(u[0]) == used
    with pytest.raises(ffi.AzError) as e:
        ctx.train_ex_rois(TP, [size], [gt], case_noise(g, 0)[:used - 1])
    assert e.value.code == ffi.AZ_ERR_CAPACITY and e.value.needed == used
    with pytest.raises(ffi.AzError) as e:
        ctx.train_ex_rois(TP, [size], [gt], case_noise(g, 0), cap=E - 1)
    assert e.value.code == ffi.AZ_ERR_CAPACITY and e.value.needed_cap == E
    ex32 = g["c0_ex_boxes"].astype(np.float32)
    T = int(g["c0_ntargets"])
    t, _ = ctx.train_adj_targets(TP, ex32, [0, E], [gt.astype(np.float32)], cap=T)
    assert t.shape[0] == T
    with pytest.raises(ffi.AzError) as e:
        ctx.train_adj_targets(TP, ex32, [0, E], [gt.astype(np.float32)], cap=T - 1)
    assert e.value.code == ffi.AZ_ERR_CAPACITY and e.value.needed_cap == T


def random_image(rng):
    h, w = (int(v) for v in rng.randint(120, 801, 2))
    n = int(rng.randint(0, 41))
    bw = rng.uniform(0.01, 0.45, n) * w
    bh = rng.uniform(0.01, 0.45, n) * h
    x1 = rng.uniform(0, w - 1 - bw)
    y1 = rng.uniform(0, h - 1 - bh)
    gt = np.floor(np.stack([x1, y1, x1 + bw, y1 + bh], 1)).reshape(-1, 4)
    if n >= 4:
        gt[n - 1] = gt[0]                                   # a duplicate
        gt[n - 2, 2:] = gt[n - 2, :2]                        # a 1-px object
        gt[n - 3, 2] = gt[n - 3, 0]                          # a 1-px-wide object
    return (h, w), gt


def test_random_cross_check(ctx):
    rng = np.random.RandomState(2024)
    n_images, chunk, worst, n_t = 200, 25, 0.0, 0
    for s in range(0, n_images, chunk):
        ims = [random_image(rng) for _ in range(chunk)]
        sizes, gts = [a for a, _ in ims], [b for _, b in ims]
        noise = rng.random_sample(12000 * chunk)
        ex, zoom, off, used = ctx.train_ex_rois(TP, sizes, gts, noise)
        t, toff = ctx.train_adj_targets(TP, ex, off, [b.astype(np.float32) for b in gts])
        at = 0
        for j in range(chunk):
            b, z, u = tr.compute_ex_rois(sizes[j], gts[j], noise[at:], C)
            at += u
            what = "image %d %s N=%d" % (s + j, sizes[j], gts[j].shape[0])
            assert u == int(used[j]), what
            assert np.array_equal(b.astype(np.float32), ex[off[j]:off[j + 1]]), what
            assert np.array_equal(z, zoom[off[j]:off[j + 1]].astype(bool)), what
            ref = tr.compute_targets(gts[j], ex[off[j]:off[j + 1]], C)
            worst = max(worst, check_targets(t[toff[j]:toff[j + 1]], ref, what))
            n_t += ref.shape[0]
    print("%d images, %d targets compared; max |dw, dh| difference %.2f ulp" % (n_images, n_t, worst))


def set_state(g, prefix):
    return ("MT19937", g[prefix + "_keys"], int(g[prefix + "_pos"][0]), int(g[prefix + "_pos"][1]), float(g[prefix + "_gauss"]))


def same_state(g, prefix):
    st = np.random.get_state()
    return np.array_equal(st[1], g[prefix + "_keys"]) and int(st[2]) == int(g[prefix + "_pos"][0])


def build_synthetic(ctx):
    from az_data_layer import roidb as rdl
    from datasets.synthetic import SyntheticImdb
    from detect.config import cfg
    assert not cfg.TRAIN.USE_CACHE
    from aznet_hip import ffi
    ffi.set_default_context(ctx)
    imdb = SyntheticImdb(375, 500, 8)
    imdb.append_flipped_images()
    np.random.seed(3)
    rdl.prepare_roidb(imdb)
    state = np.random.get_state()
    means, stds = rdl.add_adjacent_prediction_targets(imdb)
    return imdb, state, means, stds


def test_synthetic_roidb_and_minibatches(ctx, g):
    from az_data_layer.minibatch import get_minibatch
    from detect.config import cfg
    imdb, state, means, stds = build_synthetic(ctx)
    assert np.array_equal(state[1], g["syn_state_keys"]) and int(state[2]) == int(g["syn_state_pos"][0])
    n = int(g["syn_n"])
    assert len(imdb.roidb) == n == 16
    raw = []
    for i, e in enumerate(imdb.roidb):
        assert e["flipped"] == bool(g["syn%d_flipped" % i])
        for k in ("ex_boxes", "zoom_gt", "gt_boxes"):
            assert e[k].dtype == g["syn%d_%s" % (i, k)].dtype and np.array_equal(e[k], g["syn%d_%s" % (i, k)]), (i, k)
        assert e["bbox_targets"].dtype == np.float64 and e["bbox_targets"].shape == g["syn%d_bbox_targets" % i].shape
        raw.append(tr.compute_targets(e["gt_boxes"], e["ex_boxes"], C))
    raw = np.vstack(raw)
    got = np.vstack([e["bbox_targets"] for e in imdb.roidb])
    ref = np.vstack([g["syn%d_bbox_targets" % i] for i in range(n)])
    gm, gs = g["syn_means"].reshape(11, 4), g["syn_stds"].reshape(11, 4)
    # (dw, dh enter the sums with the device's log: within 4 ulp of the reference's each)
    in_err = 4 * np.finfo(np.float64).eps * max(1.0, float(np.abs(raw[:, 2:4]).max()))
    check_stats(means.reshape(11, 4), stds.reshape(11, 4), got, gm, gs, raw, ref, in_err)
    # minibatches: the reference's samples (its RNG call order), blobs without `data`
    for b in range(int(g["n_batches"])):
        cfg.SEAR.SCALE_ADJ_CONF = bool(g["mb%d_conf" % b])
        try:
            np.random.seed(int(g["mb%d_seed" % b]))
            blobs = get_minibatch([imdb.roidb[i] for i in g["mb%d_inds" % b]], 11, ctx)
        finally:
            cfg.SEAR.SCALE_ADJ_CONF = False
        assert same_state(g, "mb%d_state" % b), b
        assert blobs["data"].shape == (len(g["mb%d_inds" % b]), 3, 600, 800) and blobs["data"].dtype == np.float32
        assert np.array_equal(blobs["rois"].astype(np.float32), g["mb%d_rois" % b]), b
        assert np.array_equal(blobs["zoom_labels"].astype(np.float32), g["mb%d_zoom_labels" % b]), b
        assert np.array_equal(blobs["adj_loss_weights"], g["mb%d_adj_loss_weights" % b]), b
        assert np.array_equal(blobs["adj_labels"].astype(np.float32), g["mb%d_adj_labels" % b]), b
        # (normalised targets within ~1e-12 of the reference's in f64, far below an f32 step: the f32 casts differ by at
        #  most one f32 ulp, where the two f64 values straddle a rounding boundary)
        ref_t = g["mb%d_adj_targets" % b]
        assert np.all(np.abs(blobs["adj_targets"] - ref_t) <= np.spacing(np.abs(ref_t))), b


def test_short_noise_block_is_retried(ctx, g, monkeypatch):
    """prepare_roidb's first block of uniforms too small for the chunk: the device says so, the chunk runs again with
    a larger block; same regions, np.random left in the same state."""
    from az_data_layer import roidb as rdl
    monkeypatch.setattr(rdl, "NOISE_PER_IMAGE", 16)
    monkeypatch.setattr(rdl, "CHUNK", 5)
    imdb, state, _, _ = build_synthetic(ctx)
    assert np.array_equal(state[1], g["syn_state_keys"]) and int(state[2]) == int(g["syn_state_pos"][0])
    for i, e in enumerate(imdb.roidb):
        assert np.array_equal(e["ex_boxes"], g["syn%d_ex_boxes" % i]) and np.array_equal(e["zoom_gt"], g["syn%d_zoom_gt" % i])


def test_runs_are_identical(ctx):
    a = build_synthetic(ctx)
    b = build_synthetic(ctx)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    for x, y in zip(a[0].roidb, b[0].roidb):
        for k in ("ex_boxes", "zoom_gt", "gt_boxes", "bbox_targets"):
            assert x[k].tobytes() == y[k].tobytes()
