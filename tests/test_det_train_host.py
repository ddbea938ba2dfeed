"""CPU: the detection net's training data layer and head step without a GPU.

1. The NumPy restatement tests/det_train_ref.py against what the REFERENCE's own roi_data_layer/roidb.py and minibatch.py
   recorded (tests/golden/g21_train_det.npz): bit for bit, dw / dh included (both sides use NumPy's log).  It then stands in
   for the two device entry points, so that roi_data_layer's prepare_roidb (proposals cache, flips), add_bbox_regression_targets,
   the sampler and RoIDataLayer's index logic run here against the same goldens, np.random's state included.
2. The float64 / float32 restatement of the head step tests/det_step_ref.py: its softmax loss and every gradient against
   central finite differences, and its float32 run's ReLU gates against float64's on the GPU tests' cases.
3. detect/prototxt.py: read_det_train_net on frcnn/train.prototxt's values as the new writer states them; read_train_net
   still refuses that net."""
import os
import pickle

import numpy as np
import pytest

import det_step_ref as D
import det_train_ref as DR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g21_train_det.npz")
K = 21


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. the data layer -----------------------------------------------------------------------------------------------------
def test_restatement_equals_reference(g):
    views = []
    for i in range(int(g["n_cases"])):
        t, mo = DR.compute_targets(g["c%d_ex" % i], g["c%d_gt" % i], g["c%d_labels" % i])
        assert same(t, g["c%d_targets" % i]), "targets of case %d" % i
        assert same(mo, g["c%d_max_overlaps" % i]), "max_overlaps of case %d" % i
        views.append(t)
    counts, means, stds = DR.target_stats(views, K)
    assert same(means.ravel(), g["set_means"]) and same(stds.ravel(), g["set_stds"])
    for i, t in enumerate(views):
        assert same(t, g["c%d_norm" % i]), "normalised targets of case %d" % i
    assert counts[0] == DR.EPS and counts[3] > 2


def test_goldens_hold_the_cases(g):
    """What the issue lists: no objects; a first-maximum tie; IoU exactly 0.5; max(1, .) binding; and, in the synthetic set,
    an image with an empty background band and one with fewer foreground boxes than the quota; stds > 0, nothing nan."""
    assert g["c1_gt"].shape[0] == 0 and not g["c1_targets"].any() and g["c1_max_overlaps"].dtype == np.float32
    assert np.all(g["c1_max_overlaps"] == np.float32(0.1))
    ov = DR.iou_matrix(g["c2_ex"], g["c2_gt"])
    tie = (ov[:, 0] == ov[:, 1]) & (ov[:, 0] >= 0.5)
    assert tie.sum() >= 5 and set(g["c2_targets"][tie, 0].tolist()) == {float(g["c2_labels"][0])}
    assert tuple(g["c3_ex"][0]) == (0, 0, 9, 9) and tuple(g["c3_gt"][0]) == (0, 0, 9, 19)
    assert g["c3_max_overlaps"][0] == 0.5 and g["c3_targets"][0, 0] == g["c3_labels"][0]
    assert g["c3_max_overlaps"][1] < 0.5 and g["c3_targets"][1, 0] == 0
    thin = (g["c3_targets"][:, 0] > 0) & ((g["c3_ex"][:, 2] - g["c3_ex"][:, 0] < 1) | (g["c3_ex"][:, 3] - g["c3_ex"][:, 1] < 1))
    assert thin.sum() >= 4
    mo2, mo4 = g["syn2_max_overlaps"], g["syn4_max_overlaps"]
    assert not np.any((mo2 >= 0.1) & (mo2 < 0.5)) and 0 < (mo4 >= 0.5).sum() < 16
    for name in g.files:
        if g[name].dtype.kind == "f":
            assert np.all(np.isfinite(g[name])), name
    for pre, n in (("c", int(g["n_cases"])), ("syn", int(g["syn_n"]))):
        stds = (g["set_stds"] if pre == "c" else g["syn_stds"]).reshape(K, 4)
        seen = set()
        for i in range(n):
            t = g["c%d_targets" % i] if pre == "c" else g["syn%d_bbox_targets" % i]
            seen |= set(int(c) for c in t[:, 0] if c > 0)
        assert len(seen) >= 10 and all(np.all(stds[c] > 0) for c in seen)


@pytest.fixture()
def det_rdl():
    from roi_data_layer import roidb as rdl
    rdl.set_backend(DR.RefBackend())
    yield rdl
    rdl.set_backend(None)


synthetic_roidb = DR.synthetic_roidb
FakeNet = DR.FakeNet


def check_synthetic(imdb, means, stds, g, dw_ulp=0):
    """dw_ulp: the float32 steps the un-normalised dw / dh may be off (0 on the CPU; the device's log: 1) -- the
    normalised targets are then compared through the golden's own means and stds."""
    assert same(means, g["syn_means"]) or dw_ulp
    for i, e in enumerate(imdb.roidb):
        assert bool(e["flipped"]) == bool(g["syn%d_flipped" % i])
        for k in ("ex_boxes", "gt_boxes", "max_overlaps"):
            assert same(e[k], g["syn%d_%s" % (i, k)]), (i, k)
        assert np.array_equal(e["gt_labels"], g["syn%d_gt_labels" % i])
        if not dw_ulp:
            assert same(e["bbox_targets"], g["syn%d_bbox_targets" % i]), i
    if not dw_ulp:
        assert same(stds, g["syn_stds"])


def test_roidb_on_the_restatement(det_rdl, g, tmp_path, monkeypatch):
    imdb, means, stds = synthetic_roidb(det_rdl, g, tmp_path, monkeypatch)
    check_synthetic(imdb, means, stds, g)
    # flipped entries mirror their originals
    for i in range(8):
        a, b = imdb.roidb[i]["ex_boxes"], imdb.roidb[8 + i]["ex_boxes"]
        assert np.array_equal(b[:, 0], 500 - a[:, 2] - 1) and np.array_equal(b[:, 2], 500 - a[:, 0] - 1)
        assert imdb.roidb[8 + i]["gt_labels"] is imdb.roidb[i]["gt_labels"]
    # without a cache the net is asked, and the pickle is written
    from roi_data_layer import roidb as rdl
    from datasets.synthetic import SyntheticImdb
    from detect import config
    asked = []

    def fake_propose(net, entry):
        asked.append(entry["image"])
        return g["syn_prop%d" % (len(asked) - 1)].astype(np.float64)
    monkeypatch.setattr(rdl, "_propose", fake_propose)
    monkeypatch.setattr(config.cfg, "EXP_DIR", "det_host_2")
    imdb2 = SyntheticImdb(375, 500, 8)
    imdb2.append_flipped_images()
    net = FakeNet()
    rdl.prepare_roidb(imdb2, net)
    assert asked == ["synthetic://%d" % i for i in range(8)]
    with open(os.path.join(config.get_output_dir(imdb2, net), "proposals.pkl"), "rb") as f:
        saved = pickle.load(f)
    assert len(saved) == 8 and all(same(saved[i], g["syn_prop%d" % i]) for i in range(8))
    assert all(same(imdb2.roidb[i]["ex_boxes"], g["syn%d_ex_boxes" % i]) for i in range(16))


def check_minibatches(imdb, g, ctx=None):
    """get_minibatch on the golden's image indices and seeds: every blob and np.random's state afterwards."""
    from roi_data_layer.minibatch import get_minibatch
    import train_step_ref as R
    for b in range(int(g["n_batches"])):
        inds = [int(i) for i in g["mb%d_inds" % b]]
        np.random.seed(int(g["mb%d_seed" % b]))
        blobs = get_minibatch([imdb.roidb[i] for i in inds], K, ctx or R.ShapeOnlyBlobCtx())
        for k in ("rois", "labels", "bbox_targets", "bbox_loss_weights"):
            assert same(np.asarray(blobs[k]).astype(np.float32), g["mb%d_%s" % (b, k)]), (b, k)
        st = np.random.get_state()
        assert np.array_equal(st[1], g["mb%d_state_keys" % b]) and int(st[2]) == int(g["mb%d_state_pos" % b][0]), b
        assert blobs["data"].shape == (len(inds), 3, 600, 800)


def test_minibatches_equal_reference(det_rdl, g, tmp_path, monkeypatch):
    imdb, _, _ = synthetic_roidb(det_rdl, g, tmp_path, monkeypatch)
    check_minibatches(imdb, g)
    # the restatement's sampler draws the same
    for b in range(int(g["n_batches"])):
        inds = [int(i) for i in g["mb%d_inds" % b]]
        np.random.seed(int(g["mb%d_seed" % b]))
        blobs = DR.minibatch([imdb.roidb[i] for i in inds], K, [float(g["mb_im_scale"])] * len(inds))
        assert all(same(blobs[k], g["mb%d_%s" % (b, k)]) for k in blobs), b
    # fallback pool and short foreground, as recorded
    assert (g["mb0_labels"] > 0).sum() == 32 and g["mb0_rois"].shape[0] < 128
    assert 0 < (g["mb2_labels"] > 0).sum() < 32


def test_layer_cursor_and_prefetch(det_rdl, g, tmp_path, monkeypatch):
    import train_step_ref as R
    from detect.config import cfg
    from roi_data_layer.layer import BLOB_NAMES, RoIDataLayer
    imdb, _, _ = synthetic_roidb(det_rdl, g, tmp_path, monkeypatch)
    for per_batch in (1, 2):
        monkeypatch.setattr(cfg.TRAIN, "IMS_PER_BATCH", per_batch)
        np.random.seed(5)
        layer = RoIDataLayer(K, ctx=R.ShapeOnlyBlobCtx())
        layer.set_roidb(imdb.roidb)
        np.random.seed(5)
        perm = np.random.permutation(np.arange(16))
        assert np.array_equal(layer._perm, perm)
        steps = 16 // per_batch - 1                      # the reshuffle comes when cur + IMS_PER_BATCH >= len
        for s in range(steps):
            blobs = layer.forward()
            assert set(blobs) == set(BLOB_NAMES) and all(v.dtype == np.float32 for v in blobs.values())
            assert np.array_equal(layer._perm, perm) and layer._cur == (s + 1) * per_batch
            assert blobs["rois"].shape[0] == blobs["labels"].shape[0] == blobs["bbox_targets"].shape[0] <= 128
            assert blobs["bbox_targets"].shape[1] == 4 * K and int(blobs["rois"][:, 0].max()) == per_batch - 1
            fg = blobs["labels"] > 0
            assert np.array_equal(blobs["bbox_loss_weights"].sum(axis=1), 4.0 * fg)
        layer.forward()
        assert layer._cur == per_batch and not np.array_equal(layer._perm, perm)
    monkeypatch.setattr(cfg.TRAIN, "USE_PREFETCH", True)
    with pytest.raises(NotImplementedError, match="USE_PREFETCH"):
        RoIDataLayer(K).set_roidb(imdb.roidb)


# ---- 2. the head step's restatement ------------------------------------------------------------------------------------------
def test_softmax_loss_matches_finite_differences():
    rng = np.random.Generator(np.random.PCG64(2))
    x = rng.standard_normal((5, 21)) * 3
    labels = np.array([0, 20, 7, 3, 20])
    loss, d, p = D.softmax_loss(x, labels, 5.0)
    assert np.allclose(p.sum(axis=1), 1) and abs(loss - np.mean(-np.log(p[np.arange(5), labels]))) < 1e-12
    num = np.zeros_like(x)
    h = 1e-6
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[i, j] += h
            xm[i, j] -= h
            num[i, j] = (D.softmax_loss(xp, labels, 5.0)[0] - D.softmax_loss(xm, labels, 5.0)[0]) / (2 * h)
    print("softmax: max |analytic - numeric| = %.3e" % np.abs(d - num).max())
    assert np.abs(d - num).max() < 1e-8
    # +-80 and a row of equal logits: finite, and the clamp at FLT_MIN
    x = np.full((3, 21), -80.0)
    x[0, 4] = 80.0
    x[1, :] = 1.25
    x[2, :] = 80.0
    x[2, 0] = -80.0
    loss, d, p = D.softmax_loss(x, np.array([4, 9, 0]), 3.0)
    assert np.isfinite(loss) and np.all(np.isfinite(d)) and np.allclose(p[1], 1 / 21.0)
    want = (0.0 + np.log(21.0) - np.log(float(np.finfo(np.float32).tiny))) / 3
    assert abs(loss - want) < 1e-9


def test_step_gradients_match_finite_differences():
    """The whole head, float64, smallest and an odd size: every parameter gradient and d pool5 against central differences
    of the summed loss (no dropout, so the loss is a function of the parameters alone; ReLU kinks are measure zero)."""
    for C, n6, n7, ncls, n in ((4, 4, 4, 2, 3), (4, 12, 8, 5, 7)):
        rng = np.random.Generator(np.random.PCG64(n))
        head = {k: v.astype(np.float64) for k, v in D.filler_head(3, C, n6, n7, ncls).items()}
        pool = np.abs(rng.standard_normal((n, C * 49)))
        blobs = D.random_blobs(4, n, 1, 12, 16, ncls)
        r = D.step(head, pool, blobs, None)
        f = lambda hd, pl: float(np.sum(D.step(hd, pl, blobs, None, want_dpool=False)["losses"]))
        worst = 0.0
        h = 1e-6
        for k in D.KEYS:
            flat = head[k].reshape(-1)
            for idx in rng.choice(flat.size, size=min(12, flat.size), replace=False):
                old = flat[idx]
                flat[idx] = old + h
                up = f(head, pool)
                flat[idx] = old - h
                dn = f(head, pool)
                flat[idx] = old
                worst = max(worst, abs((up - dn) / (2 * h) - np.asarray(r["grads"][k]).reshape(-1)[idx]))
        for idx in rng.choice(pool.size, size=12, replace=False):
            pp, pm = pool.copy(), pool.copy()
            pp.reshape(-1)[idx] += h
            pm.reshape(-1)[idx] -= h
            worst = max(worst, abs((f(head, pp) - f(head, pm)) / (2 * h) - r["d_pool5"].reshape(-1)[idx]))
        print("head %s: max |analytic - numeric| = %.3e" % ((C, n6, n7, ncls), worst))
        assert worst < 1e-7


@pytest.mark.parametrize("name", sorted(D.HEADS))
def test_float32_gates_equal_float64_on_the_gpu_cases(name):
    head, fmap, blobs = D.case(name)
    pool, arg = D.roi_pool(fmap, blobs["rois"])
    masks = D.step_masks(3, 0, pool.shape[0], head)
    r64 = D.step(head, pool, blobs, masks)
    r32 = D.step(head, pool, blobs, masks, dtype=np.float32)
    for t, _, _ in D.LAYERS:
        miss = D.gate_mismatch(r32["pre%d" % t], r64["pre%d" % t])
        print("%s layer %d: %.2e of the gates differ" % (name, t, miss))
        assert miss == 0.0
    assert np.all(np.isfinite(r64["losses"])) and r64["losses"][0] > 0
    if name != "small":
        assert r64["losses"][1] > 0 and (blobs["labels"] > 0).sum() >= 3
    assert D.rel_err(r32["grads"]["W6"], r64["grads"]["W6"]) < 1e-4


# ---- 3. prototxt -------------------------------------------------------------------------------------------------------------
def test_read_det_train_net_and_az_reader_refuses_it(tmp_path):
    from detect import prototxt as P
    path = str(tmp_path / "train_det.prototxt")
    P.write_train_prototxt(path, P.det_layer_table(), name="frcnn_train")
    net = P.read_det_train_net(path)
    assert set(net) == set(P.CONV_LAYERS + P.DET_HEAD_LAYERS)
    # models/Pascal/VGG16/frcnn/train.prototxt: conv1_1 .. conv2_2 frozen, the rest 1 / 2 and 1 / 0; dropout 0.5 on fc6, fc7;
    # gaussian 0.01 for cls_score, 0.001 for bbox_pred, no filler for fc6 / fc7
    for n in P.CONV_LAYERS[:4]:
        assert net[n]["lr_mult"] == [0.0, 0.0] and net[n]["decay_mult"] == [0.0, 0.0]
    for n in P.CONV_LAYERS[4:] + P.DET_HEAD_LAYERS:
        assert net[n]["lr_mult"] == [1.0, 2.0] and net[n]["decay_mult"] == [1.0, 0.0]
    assert [net[n]["dropout_ratio"] for n in P.DET_HEAD_LAYERS] == [0.5, 0.5, None, None]
    assert [net[n]["std"] for n in P.DET_HEAD_LAYERS] == [None, None, 0.01, 0.001]
    with pytest.raises(ValueError, match="not part of the AZ-net"):
        P.read_train_net(path)
    az = str(tmp_path / "train_az.prototxt")
    P.write_train_prototxt(az, P.layer_table())
    assert set(P.read_train_net(az)) == set(P.CONV_LAYERS + P.HEAD_LAYERS)
    with pytest.raises(ValueError, match="not part of the detection net"):
        P.read_det_train_net(az)
    rows = [r if r[0] != "cls_score" else r[:7] + (0.3,) for r in P.det_layer_table()]
    P.write_train_prototxt(path, rows)
    with pytest.raises(ValueError, match="Dropout on 'cls_score'"):
        P.read_det_train_net(path)


# ---- 4. SolverWrapper without a GPU ----------------------------------------------------------------------------------------
class StubTrainer(object):
    """AzDetSolver's parameter interface on host arrays."""

    def __init__(self, head):
        self.p = {k: np.array(v, dtype=np.float32) for k, v in head.items()}
        self.hyper = None

    def _shapes(self):
        return {k: v.shape for k, v in self.p.items()}

    def read(self):
        return {k: v.copy() for k, v in self.p.items()}

    def load(self, head):
        for k, v in head.items():
            self.p[k] = np.asarray(v, dtype=np.float32).reshape(self.p[k].shape)

    def set_hyper(self, lr, dc, drop):
        self.hyper = (list(lr), list(dc), list(drop))


def test_snapshot_unnormalises_and_restores(det_rdl, g, tmp_path, monkeypatch):
    from aznet_hip import caffemodel as cm
    from detect.config import cfg
    from detect.train_det import SolverWrapper
    imdb, means, stds = synthetic_roidb(det_rdl, g, tmp_path, monkeypatch)
    raw = [e["bbox_targets"].copy() for e in imdb.roidb]
    head = D.filler_head(9, 16, 128, 96, K)
    tr = StubTrainer(head)
    monkeypatch.setattr(cfg.TRAIN, "SNAPSHOT_INFIX", "t1")
    # (SolverWrapper computes the targets itself: hand it the roidb as prepare_roidb leaves it)
    for e in imdb.roidb:
        del e["bbox_targets"], e["max_overlaps"]
    sw = SolverWrapper(D.traj_solver_files(str(tmp_path)), imdb, str(tmp_path / "out"), trainer=tr)
    assert tr.hyper == ([1.0, 2.0] * 4, [1.0, 0.0] * 4, [0.5, 0.5])
    assert same(sw.bbox_means, means) and same(sw.bbox_stds, stds) and sw.bbox_means.shape == (4 * K,) and sw.conv_train == []
    assert all(same(e["bbox_targets"], r) for e, r in zip(imdb.roidb, raw))
    sw.iter = 12
    path = sw.snapshot()
    assert path == str(tmp_path / "out" / "frcnn_small_t1_iter_12.caffemodel")
    got = cm.det_head_from_layers(cm.load_caffemodel(path))
    for k in D.KEYS:
        want = head[k]
        if k == "Wb":
            want = (head[k] * stds[:, None]).astype(np.float32)
        elif k == "bb":
            want = (head[k] * stds + means).astype(np.float32)
        assert np.array_equal(got[k], want), k
    assert all(np.array_equal(tr.p[k], head[k]) for k in D.KEYS)                # the trainer keeps normalised weights
    # TRAIN.UN_NORMALIZE re-initialises bbox_pred of a pretrained (un-normalised) model, for the classes that have targets
    monkeypatch.setattr(cfg.TRAIN, "UN_NORMALIZE", True)
    for e in imdb.roidb:
        del e["bbox_targets"], e["max_overlaps"]
    tr2 = StubTrainer(got)
    sw2 = SolverWrapper(D.traj_solver_files(str(tmp_path)), imdb, str(tmp_path / "out2"), trainer=tr2)
    live = np.repeat(stds.reshape(K, 4).min(axis=1) > 0, 4)
    assert live.sum() >= 40
    assert np.allclose(tr2.p["Wb"][live], head["Wb"][live], rtol=1e-5, atol=1e-9)
    assert np.allclose(tr2.p["bb"][live], head["bb"][live], rtol=1e-4, atol=1e-6) and sw2.iter == 0


def test_train_tool_flags_and_header():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(REPO, "az-net_amd", "tools", "train_det_net.py"), "--help"],
                         capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--gpu", "--solver", "--iters", "--weights", "--cfg", "--imdb", "--rand", "--norm", "--def", "--def_fc", "--net",
                 "--exp", "--base-lr"):
        assert flag in out.stdout, flag
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    for name in ("az_det_targets", "az_det_target_stats", "az_det_solver_create", "az_det_solver_step", "az_det_solver_update",
                 "az_det_solver_forward_test", "az_det_solver_fetch", "roidb.py:", "train_det.py:"):
        assert name in src, name


def test_frozen_run_restatement_lowers_the_loss(det_rdl, g, tmp_path, monkeypatch):
    """The GPU front-door test requires the summed loss of the last five of 20 steps to lie below that of the first five.
    That must first hold, with room, for the float64 restatement at the recorded base_lr: here with the data layer answered
    by the NumPy restatement and the frozen backbone and the image front-end on the CPU."""
    import torch
    from detect import prototxt as P
    from roi_data_layer.layer import RoIDataLayer
    T = D.TRAJ
    imdb, _, _ = synthetic_roidb(det_rdl, g, tmp_path, monkeypatch)
    np.random.seed(T["np_seed"])
    layer = RoIDataLayer(K, ctx=D.TorchBlobCtx())
    layer.set_roidb(imdb.roidb)
    bb = D.traj_backbone("cpu")
    C = bb.out_channels
    rng = np.random.Generator(np.random.PCG64(T["solver_seed"]))
    shapes = {"W6": (T["n6"], C * 49), "W7": (T["n7"], T["n6"]), "Wc": (K, T["n7"]), "Wb": (4 * K, T["n7"])}
    std = {"W6": P.DET_FILLER_DEFAULT, "W7": P.DET_FILLER_DEFAULT, "Wc": 1e-2, "Wb": 1e-3}
    head = {}
    for k in D.KEYS:
        head[k] = (rng.standard_normal(shapes[k]) * std[k]).astype(np.float32) if k in shapes else np.zeros(shapes["W" + k[1:]][0], np.float32)
    ref = D.RefTrajectory(head, np.float64, T["solver"])
    tot = []
    for _ in range(T["steps"]):
        b = layer.forward()
        with torch.no_grad():
            conv = bb.forward_train(b["data"]).numpy()
        tot.append(float(ref.step(conv, b, T["solver_seed"])["losses"].sum()))
    first, last = sum(tot[:5]), sum(tot[-5:])
    print("float64 restatement, frozen run at base_lr %g: first five %.4f, last five %.4f" % (T["solver"]["base_lr"], first, last))
    print("  per step: " + " ".join("%.3f" % t for t in tot))
    assert last < 0.9 * first, (first, last)
