"""CPU: the yardstick of the training step (tests/train_step_ref.py) and the host side of training.  The restatement's
hand-written backward against torch.autograd in float64; the loss formulae where exp would overflow and with fractional
targets; the NumPy form of the dropout generator; the prototxt reader; learning-rate policy and gradient clipping; the
float32-CPU restatement's ReLU gates against float64 for every case the GPU tests use (the cap of 1e-4 is a condition on
the chosen seeds); SolverWrapper.snapshot with the trainer replaced by a stub; and that the float64 restatement of the
frozen 20-step run lowers the loss on the chosen seed and solver text."""
import os

import numpy as np
import pytest

import train_step_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_equals_autograd_f64():
    import torch
    from aznet_hip import ffi
    dims = dict(C=4, n6=12, n71=7, n72=5)
    head = R.filler_head(3, **dims)
    rng = np.random.Generator(np.random.PCG64(1))
    fmap = rng.standard_normal((2, 4, 9, 11)).astype(np.float32)
    blobs = R.random_blobs(2, 10, 2, 9, 11)
    pool, arg = R.roi_pool(fmap, blobs["rois"])
    masks = {t: ffi.dropout_mask(5, 3, l, 10 * n, 0.5).reshape(10, n) for t, l, n in ((6, 0, 12), (71, 1, 7), (72, 2, 5))}
    ref = R.step(head, pool, blobs, masks)
    dmap = R.roi_pool_backward(ref["d_pool5"], arg, blobs["rois"], fmap.shape)

    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    P = {k: t(v) for k, v in head.items()}
    fm = t(fmap)
    rows = []
    for r in range(10):                     # RoIPool as indexing by the restatement's arg-max (the map is the leaf)
        n = int(blobs["rois"][r, 0])
        flat = fm[n].reshape(4, -1)
        a = torch.tensor(arg[r].reshape(4, 49).astype(np.int64))
        rows.append(torch.where(a >= 0, torch.gather(flat, 1, a.clamp(min=0)), torch.zeros((), dtype=torch.float64)).reshape(-1))
    x = torch.stack(rows)
    m = {k: torch.tensor(v.astype(np.float64)) for k, v in masks.items()}
    a6 = torch.relu(x @ P["W6"].T + P["b6"]) * m[6] * 2
    a71 = torch.relu(a6 @ P["W71"].T + P["b71"]) * m[71] * 2
    a72 = torch.relu(a6 @ P["W72"].T + P["b72"]) * m[72] * 2
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    lz = bce((a72 @ P["Wz"].T + P["bz"]).reshape(-1), torch.tensor(blobs["zoom_labels"].astype(np.float64)), reduction="sum") / 10
    la = bce(a71 @ P["Was"].T + P["bas"], torch.tensor(blobs["adj_labels"].astype(np.float64)), reduction="sum") / 10
    w = torch.tensor(blobs["adj_loss_weights"].astype(np.float64))
    d = w * ((a71 @ P["Wab"].T + P["bab"]) - torch.tensor(blobs["adj_targets"].astype(np.float64)))
    lb = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum() / 10
    (lz + la + lb).backward()
    assert np.allclose(ref["losses"], [lz.item(), la.item(), lb.item()], rtol=1e-12, atol=0)
    for k in R.KEYS:
        assert np.allclose(ref["grads"][k], P[k].grad.numpy(), rtol=1e-10, atol=1e-14), k
    assert np.allclose(dmap, fm.grad.numpy(), rtol=1e-10, atol=1e-14)
    assert np.abs(dmap).max() > 0 and all(np.abs(ref["grads"][k]).max() > 0 for k in R.KEYS)


def test_roi_pool_first_maximum_and_empty_bins():
    fmap = np.zeros((1, 1, 6, 6), np.float32)
    fmap[0, 0, 1, 2] = fmap[0, 0, 3, 4] = 5.0                       # two equal maxima: the first in (h, w) order wins
    rois = np.array([[0, 0, 0, 95, 95], [0, 200, 200, 230, 230]], np.float32)   # the second lies outside the map
    pool, arg = R.roi_pool(fmap, rois)
    assert arg[1].max() == -1 and not pool[1].any()
    big = np.array([[0, 0, 0, 80, 80]], np.float32)                # 6 x 6 cells into 7 x 7 bins
    pool, arg = R.roi_pool(fmap, big)
    assert set(arg[0][pool[0] == 5.0]) == {1 * 6 + 2, 3 * 6 + 4}
    fmap[:] = 1.0
    pool, arg = R.roi_pool(fmap, np.array([[0, 0, 0, 95, 95]], np.float32))
    assert arg[0][0] == 0                                          # all equal: the window's first cell


def test_losses_large_x_and_fractional_targets():
    for dt in (np.float32, np.float64):
        x = np.array([-1e4, -90.0, -1.0, 0.0, 1.0, 90.0, 1e4], dtype=dt)
        for tv in (0.0, 1.0, 0.3):
            t = np.full_like(x, tv)
            loss, dx = R.sigmoid_ce(x, t, dt(7))
            assert np.isfinite(loss) and np.all(np.isfinite(dx))
            xe = x.astype(np.float64)
            exact = np.sum(np.maximum(xe, 0) - xe * tv + np.log1p(np.exp(-np.abs(xe)))) / 7
            assert abs(float(loss) - exact) <= 1e-6 * abs(exact)
            assert np.allclose(dx[[0, -1]] * 7, [0 - tv, 1 - tv], atol=1e-7)
        d = np.array([-3.0, -1.0, -0.5, 0.0, 0.5, 1.0, 3.0], dtype=dt)
        loss, dx = R.smooth_l1(d, np.zeros_like(d), np.ones_like(d), dt(1))
        assert np.isclose(float(loss), 2.5 + 0.5 + 0.125 + 0 + 0.125 + 0.5 + 2.5)
        assert np.array_equal(dx, np.array([-1, -1, -0.5, 0, 0.5, 1, 1], dtype=dt))
        loss, dx = R.smooth_l1(d, np.zeros_like(d), np.zeros_like(d), dt(1))
        assert float(loss) == 0 and not dx.any()


def test_dropout_generator_numpy_form():
    from aznet_hip import ffi
    n = 1 << 18
    a = ffi.dropout_mask(3, 0, 0, n)
    assert a.dtype == np.uint8 and set(np.unique(a)) == {0, 1}
    assert abs(a.mean() - 0.5) < 4 * 0.5 / np.sqrt(n)
    assert np.array_equal(a, ffi.dropout_mask(3, 0, 0, n))
    assert np.array_equal(a[:1000], ffi.dropout_mask(3, 0, 0, 1000))          # element e does not depend on n
    for other in (ffi.dropout_mask(4, 0, 0, n), ffi.dropout_mask(3, 1, 0, n), ffi.dropout_mask(3, 0, 1, n)):
        assert 0.45 < np.mean(other != a) < 0.55
    assert abs(ffi.dropout_mask(3, 0, 2, n, ratio=0.2).mean() - 0.8) < 4 * 0.4 / np.sqrt(n)
    assert ffi.dropout_mask(1, 2, 0, 64, ratio=0.0).all()
    # pinned words of the generator (the header's formula evaluated with Python integers)
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    G = 0x9E3779B97F4A7C15
    key = mix((mix((mix((7 + G) & M) + 9) & M) + 1) & M)
    want = [int((mix((key + G * (e + 1)) & M) >> 40) >= (1 << 23)) for e in range(64)]
    assert list(ffi.dropout_mask(7, 9, 1, 64)) == want


def test_prototxt_reader(tmp_path):
    from detect import prototxt as P
    net = str(tmp_path / "train.prototxt")
    P.write_train_prototxt(net, P.layer_table())
    n = P.read_train_net(net)
    assert n["conv2_2"]["lr_mult"] == [0.0, 0.0] and n["conv3_1"]["lr_mult"] == [1.0, 2.0] and n["conv3_1"]["decay_mult"] == [1.0, 0.0]
    assert n["int6"]["dropout_ratio"] == 0.5 and n["int7_2"]["dropout_ratio"] == 0.5 and n["adj_bbox"]["dropout_ratio"] is None
    assert [n[k]["std"] for k in P.HEAD_LAYERS] == [1e-4, 1e-4, 1e-3, 1e-2, 1e-3, 1e-2]
    P.write_train_prototxt(net, P.layer_table(frozen=P.CONV_LAYERS, dropout=0.25))          # the shared variant
    n = P.read_train_net(net)
    assert all(n[k]["lr_mult"] == [0.0, 0.0] for k in P.CONV_LAYERS) and n["int6"]["lr_mult"] == [1.0, 2.0]
    assert n["int7_1"]["dropout_ratio"] == 0.25
    sol = str(tmp_path / "solver.prototxt")
    P.write_solver_prototxt(sol, net, base_lr=0.01, stepsize=7, clip_gradients=20.0, snapshot_prefix="abc")
    s = P.read_solver(sol)
    assert (s["base_lr"], s["lr_policy"], s["gamma"], s["stepsize"], s["momentum"], s["weight_decay"], s["clip_gradients"],
            s["snapshot_prefix"], s["train_net"]) == (0.01, "step", 0.1, 7, 0.9, 0.0005, 20.0, "abc", net)
    assert P.resolve_train_net(sol, "elsewhere/train.prototxt") == net
    # hand-written text: comments, single quotes, no colon before a message, unknown fields
    with open(net, "w") as f:
        f.write("name: 'x' # comment\n" + "".join(
            "layer { name: '%s' type: \"%s\" bottom: 'a' param { lr_mult: 3 } convolution_param { num_output: 4 } }\n"
            % (k, "Convolution" if k in P.CONV_LAYERS else "InnerProduct") for k in P.CONV_LAYERS + P.HEAD_LAYERS))
    n = P.read_train_net(net)
    assert n["conv1_1"]["lr_mult"] == [3.0, 1.0] and n["zoom_score"]["decay_mult"] == [1.0, 1.0]
    # a net that is not the AZ head is refused
    rows = [r for r in P.layer_table() if r[0] != "int7_2"]
    P.write_train_prototxt(net, rows)
    with pytest.raises(ValueError):
        P.read_train_net(net)
    P.write_train_prototxt(net, P.layer_table() + [("fc8", "InnerProduct", 1.0, 2.0, 1.0, 0.0, 0.01, None)])
    with pytest.raises(ValueError):
        P.read_train_net(net)
    with open(sol, "w") as f:
        f.write('train_net: "x"\nlr_policy: "poly"\n')
    with pytest.raises(ValueError):
        P.read_solver(sol)
    with pytest.raises(ValueError):
        P.parse_text("layer { name: 'a' ")


def test_learning_rate_and_clip():
    from detect.train_az import learning_rate, clip_scale
    sp = dict(base_lr=0.001, lr_policy="step", gamma=0.1, stepsize=5)
    assert [learning_rate(sp, i) for i in (0, 4, 5, 9, 10)] == [0.001, 0.001, 0.001 * 0.1, 0.001 * 0.1, 0.001 * 0.1 ** 2]
    assert learning_rate(dict(sp, lr_policy="fixed"), 10 ** 6) == 0.001
    assert [R.learning_rate("step", 0.001, i, 0.1, 5) for i in (0, 5, 10)] == [learning_rate(sp, i) for i in (0, 5, 10)]
    assert clip_scale(399.0, 20.0) == 1.0 and clip_scale(400.0, 20.0) == 1.0          # norm <= clip: untouched
    assert clip_scale(1600.0, 20.0) == 0.5 and clip_scale(1600.0, -1.0) == 1.0 and clip_scale(1600.0, 0) == 1.0
    assert R.clip_scale(1600.0, 20.0) == 0.5 and R.clip_scale(100.0, 20.0) == 1.0
    # the update in float32 (the NumPy form of az_sgd_update) against the restatement run in float32
    from aznet_hip import ffi
    rng = np.random.Generator(np.random.PCG64(2))
    w, g, h = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    w2, h2 = ffi.sgd_update_numpy(w, g, h, 0.002, 0.9, 0.0005, 0.5)
    p, hh = R.sgd({"W6": w}, {"W6": g}, {"W6": h}, 0.002, 0.9, 0.0005, 0.5, dtype=np.float32)
    assert np.array_equal(w2, p["W6"]) and np.array_equal(h2, hh["W6"])
    p64, _ = R.sgd({"b6": w}, {"b6": g}, {"b6": h}, 0.001, 0.9, 0.0005, 1.0)          # biases: lr_mult 2, decay_mult 0
    assert np.allclose(p64["b6"], w - (0.9 * h.astype(np.float64) + 0.002 * g), rtol=1e-12)


@pytest.mark.parametrize("case", ["small", "small_R5", "full"])
def test_float32_gates_stay_under_the_cap(case):
    """The cap on ReLU gates that may differ between the device and float64 (1e-4 of a layer's units) is a condition on the
    seeds: the float32 CPU restatement must meet it for every layer of every case."""
    head, fmap, blobs = R.full_size_case() if case == "full" else R.small_case(R=5 if case == "small_R5" else 128)
    pool, _ = R.roi_pool(fmap, blobs["rois"])
    from aznet_hip import ffi
    n = pool.shape[0]
    masks = {t: ffi.dropout_mask(3, 0, l, n * head[k].shape[0]).reshape(n, -1) for t, l, k in ((6, 0, "b6"), (71, 1, "b71"), (72, 2, "b72"))}
    r64 = R.step(head, pool, blobs, masks, want_dpool=False)
    r32 = R.step(head, pool, blobs, masks, dtype=np.float32, want_dpool=False)
    for t in (6, 71, 72):
        frac = R.gate_mismatch(r32["pre%d" % t], r64["pre%d" % t])
        print("%s: layer %d: %.3g of the float32 gates differ from float64" % (case, t, frac))
        assert frac <= 1e-4, (case, t, frac)
    assert np.all(r64["losses"] > 0)


class StubTrainer(object):
    def __init__(self, head):
        self.p = {k: v.copy() for k, v in head.items()}
        self.loads = 0

    def read(self):
        return {k: v.copy() for k, v in self.p.items()}

    def load(self, d):
        self.loads += 1
        for k, v in d.items():
            self.p[k] = np.asarray(v, np.float32).reshape(self.p[k].shape)

    def set_hyper(self, lr, dc, drop):
        self.hyper = (list(lr), list(dc), list(drop))

    def _shapes(self):
        return {k: v.shape for k, v in self.p.items()}


def _solver_files(tmp_path, **kw):
    from detect import prototxt as P
    net = str(tmp_path / "train.prototxt")
    P.write_train_prototxt(net, P.layer_table(frozen=kw.pop("frozen", P.CONV_LAYERS)))
    sol = str(tmp_path / "solver.prototxt")
    P.write_solver_prototxt(sol, net, **kw)
    return sol


def test_snapshot_unnormalises_and_restores(tmp_path, monkeypatch):
    import train_ref
    from aznet_hip import synth, caffemodel as cm
    from az_data_layer import roidb as rdl
    from datasets.synthetic import SyntheticImdb
    from detect.config import cfg
    from detect.train_az import SolverWrapper, get_training_roidb
    rdl.set_backend(train_ref.RefBackend())
    try:
        imdb = SyntheticImdb(375, 500, 2)
        np.random.seed(3)
        get_training_roidb(imdb)
        head = R.filler_head(9, **synth.SMALL_DIMS)
        tr = StubTrainer(head)
        monkeypatch.setattr(cfg.TRAIN, "SNAPSHOT_INFIX", "t1")
        sw = SolverWrapper(_solver_files(tmp_path, snapshot_prefix="pre"), imdb, str(tmp_path / "out"), trainer=tr)
    finally:
        rdl.set_backend(None)
    assert tr.hyper == ([1.0, 2.0] * 6, [1.0, 0.0] * 6, [0.5, 0.5, 0.5])
    assert sw.bbox_means.shape == (44,) and np.all(sw.bbox_stds > 0) and sw.conv_train == []
    sw.iter = 12
    path = sw.snapshot()
    assert path == str(tmp_path / "out" / "pre_t1_iter_12.caffemodel")
    got = cm.az_head_from_layers(cm.load_caffemodel(path))
    for k in R.KEYS:
        if k == "Wab":
            assert np.array_equal(got[k], (head[k] * sw.bbox_stds[:, None]).astype(np.float32))
        elif k == "bab":
            assert np.array_equal(got[k], (head[k] * sw.bbox_stds + sw.bbox_means).astype(np.float32))
        else:
            assert np.array_equal(got[k], head[k]), k
    assert all(np.array_equal(tr.p[k], head[k]) for k in R.KEYS)               # the trainer keeps normalised weights
    # TRAIN.UN_NORMALIZE re-initialises adj_bbox of a pretrained (un-normalised) model
    monkeypatch.setattr(cfg.TRAIN, "UN_NORMALIZE", True)
    rdl.set_backend(train_ref.RefBackend())
    try:
        tr2 = StubTrainer(got)
        sw2 = SolverWrapper(_solver_files(tmp_path), imdb, str(tmp_path / "out2"), trainer=tr2)
    finally:
        rdl.set_backend(None)
    assert np.allclose(tr2.p["Wab"], head["Wab"], rtol=1e-5, atol=1e-9) and np.allclose(tr2.p["bab"], head["bab"], rtol=1e-4, atol=1e-6)
    assert sw2.iter == 0


def test_train_tool_flags():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(REPO, "az-net_amd", "tools", "train_az_net.py"), "--help"],
                         capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--gpu", "--solver", "--iters", "--weights", "--cfg", "--imdb", "--rand", "--norm", "--exp", "--net"):
        assert flag in out.stdout, flag


def test_header_describes_the_trainer():
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    for name in ("az_solver_create", "az_solver_step", "az_solver_update", "az_sgd_update", "az_solver_forward_test",
                 "az_solver_fetch", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert name in src, name


def test_frozen_run_restatement_lowers_the_loss():
    """The GPU trajectory test requires the summed loss of the last five of 20 steps to lie below that of the first five.
    That must first hold, with room, for the float64 restatement on the chosen seed and solver text: here with the data
    layer answered by the NumPy restatement and the frozen backbone and the image front-end on the CPU."""
    import torch
    from aznet_hip import synth
    T = R.TRAJ
    batches, imdb, _, _ = R.data_layer_blobs(T["height"], T["width"], T["n_images"], T["roidb_seed"], blob_ctx=R.TorchBlobCtx(),
                                             n_batches=T["steps"])
    bb = R.traj_backbone("cpu")
    d = {k: v for k, v in synth.SMALL_DIMS.items()}
    assert bb.out_channels == d["C"]
    rng = np.random.Generator(np.random.PCG64(T["solver_seed"]))
    from detect import prototxt as P
    shapes = {"W6": (d["n6"], d["C"] * 49), "W71": (d["n71"], d["n6"]), "W72": (d["n72"], d["n6"]), "Was": (11, d["n71"]),
              "Wab": (44, d["n71"]), "Wz": (1, d["n72"])}
    layer_of = {"W6": "int6", "W71": "int7_1", "W72": "int7_2", "Was": "adj_score", "Wab": "adj_bbox", "Wz": "zoom_score"}
    head = {}
    for k in R.KEYS:
        head[k] = (rng.standard_normal(shapes[k]) * P.FILLER_STD[layer_of[k]]).astype(np.float32) if k in shapes else \
            np.zeros(shapes["W" + k[1:]][0], np.float32)
    ref = R.RefTrajectory(head, np.float64)
    tot = []
    for b in batches:
        with torch.no_grad():
            conv = bb.forward_train(b["data"]).numpy()
        tot.append(float(ref.step(conv, b, T["solver_seed"])["losses"].sum()))
    first, last = sum(tot[:5]), sum(tot[-5:])
    print("float64 restatement, frozen run: first five %.4f, last five %.4f" % (first, last))
    assert last < 0.9 * first, (first, last)
