"""CPU: iter_size and the resumable solver state of detect.solver.SolverWrapper, on stub trainers that record their calls --
the solver file's key, the order of an accumulating iteration (flags, dropout iterations, the update's scale), the state
file's round trip and its refusals, and the two tools' flags."""
import os
import sys

import numpy as np
import pytest

import det_train_ref as DR
import train_step_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g21_train_det.npz")
AZ_DIMS = dict(C=16, n6=128, n71=64, n72=32)
SOLVER = dict(base_lr=0.01, lr_policy="step", gamma=0.5, stepsize=3, momentum=0.9, weight_decay=0.0005, clip_gradients=2.0,
              display=0, average_loss=3, snapshot_prefix="st")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


# ---- 1. the solver file ------------------------------------------------------------------------------------------------------
def test_iter_size_read_written_and_refused(tmp_path):
    from detect import prototxt as P
    net = str(tmp_path / "train.prototxt")
    P.write_train_prototxt(net, P.layer_table(frozen=P.CONV_LAYERS))
    sol = str(tmp_path / "solver.prototxt")
    P.write_solver_prototxt(sol, net, base_lr=0.002)
    text = open(sol).read()
    assert "\niter_size" not in text and P.read_solver(sol)["iter_size"] == 1 and P.SOLVER_DEFAULTS["iter_size"] == 1
    # the default file is what it always was, byte for byte: the eleven keys in their order, then the snapshot lines
    d = dict(P.SOLVER_DEFAULTS, base_lr=0.002, train_net=net)
    want = "".join('%s: %s\n' % (k, '"%s"' % d[k] if isinstance(d[k], str) else repr(d[k])) for k in
                   ("train_net", "base_lr", "lr_policy", "gamma", "stepsize", "momentum", "weight_decay", "clip_gradients", "display",
                    "average_loss", "snapshot_prefix")) + "# snapshots are written by SolverWrapper.snapshot\nsnapshot: 0\n"
    assert text == want
    P.write_solver_prototxt(sol, net, iter_size=1)
    assert "\niter_size" not in open(sol).read()
    P.write_solver_prototxt(sol, net, iter_size=4)
    assert "iter_size: 4\n" in open(sol).read() and P.read_solver(sol)["iter_size"] == 4
    # the reference's own solver files carry it as a comment: still 1
    with open(sol, "w") as f:
        f.write('train_net: "%s"\n# iter_size: 3\n' % net)
    assert P.read_solver(sol)["iter_size"] == 1
    for bad in ("0", "-1", "2.5", "true", '"2"'):
        with open(sol, "w") as f:
            f.write('train_net: "%s"\niter_size: %s\n' % (net, bad))
        with pytest.raises(ValueError, match="iter_size"):
            P.read_solver(sol)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="iter_size"):
            P.write_solver_prototxt(str(tmp_path / "bad.prototxt"), net, iter_size=bad)


def test_both_parsers_accept_the_new_flags(monkeypatch):
    tools = os.path.join(REPO, "az-net_amd", "tools")
    monkeypatch.syspath_prepend(tools)
    import _cli
    import train_az_net
    import train_det_net
    for mod in (train_az_net, train_det_net):
        p = _cli.build_parser("t", [mod.COMMON, mod.FLAGS])
        a = p.parse_args(["--iters", "6"])
        assert a.snapshot_state is False and a.restore is None and a.max_iters == 6
        a = p.parse_args(["--snapshot-state", "--restore", "x_iter_4.solverstate", "--iters", "6"])
        assert a.snapshot_state is True and a.restore == "x_iter_4.solverstate" and a.max_iters == 6
    from detect.config import cfg
    assert cfg.TRAIN.SNAPSHOT_STATE is False


# ---- 2. stubs ----------------------------------------------------------------------------------------------------------------
class StubBackbone(object):
    layers = []
    out_channels = 16

    def set_trainable(self, names):
        return []

    def forward_train(self, blob, taps=()):
        import torch
        return torch.zeros(1, 16, 2, 2)


class BareTrainer(object):
    """What the stub trainers of the older host tests have -- parameters and set_hyper, no set_precision, no set_accumulate,
    no history -- plus a step and an update that record their calls.  A step's losses and sum of squares are functions of the
    minibatch's tag and the iteration; an update moves weights and history."""

    def __init__(self, head, nloss):
        self.p = {k: np.array(v, dtype=np.float32) for k, v in head.items()}
        self.h = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.nloss, self.acc, self.calls, self.sumsq = nloss, 0, [], 0.0

    def _shapes(self):
        return {k: v.shape for k, v in self.p.items()}

    def read(self):
        return {k: v.copy() for k, v in self.p.items()}

    def load(self, d):
        for k, v in d.items():
            self.p[k] = np.asarray(v, np.float32).reshape(self.p[k].shape).copy()

    def set_hyper(self, lr, dc, drop):
        pass

    def step(self, conv, rois, *rest, **kw):
        seed, it = rest[-2], rest[-1]
        tag = float(np.asarray(rois).ravel()[0])
        self.calls.append(("step", self.acc, int(it), tag))
        self.sumsq = (self.sumsq if self.acc else 0.0) + 9.0 * (1.0 + tag)          # (the accumulated buffers')
        return np.asarray([tag + 0.1 * i + 1e-3 * it for i in range(self.nloss)], np.float32), self.sumsq

    def update(self, rate, momentum, decay, scale=1.0):
        self.calls.append(("update", rate, momentum, decay, scale))
        for k in self.p:
            self.h[k] = (np.float32(momentum) * self.h[k] + np.float32(rate * scale)).astype(np.float32)
            self.p[k] = self.p[k] - self.h[k]


class RecordingTrainer(BareTrainer):
    """... and the accumulate flag and the history's two directions."""

    def set_accumulate(self, on):
        self.acc = int(on)
        self.calls.append(("acc", int(on)))

    def read_history(self):
        return {k: v.copy() for k, v in self.h.items()}

    def load_history(self, d):
        for k, v in d.items():
            self.h[k] = np.asarray(v, np.float32).reshape(self.h[k].shape).copy()


def az_blobs(tag):
    z = np.zeros((1, 44), np.float32)
    return {"data": None, "rois": np.asarray([[tag, 0, 0, 9, 9]], np.float32), "adj_labels": z[:, :11], "adj_targets": z,
            "adj_loss_weights": z, "zoom_labels": z[:, 0]}


def az_wrapper(tmp, n_images=2, iter_size=1, dims=AZ_DIMS, seed=3, name="a", trainer=RecordingTrainer):
    import train_ref
    from az_data_layer import roidb as rdl
    from datasets.synthetic import SyntheticImdb
    from detect import prototxt as P
    from detect.train_az import SolverWrapper, get_training_roidb
    d = tmp / name
    d.mkdir()
    net = str(d / "train.prototxt")
    P.write_train_prototxt(net, P.layer_table(frozen=P.CONV_LAYERS))
    sol = str(d / "solver.prototxt")
    P.write_solver_prototxt(sol, net, iter_size=iter_size, **SOLVER)
    rdl.set_backend(train_ref.RefBackend())
    try:
        imdb = SyntheticImdb(375, 500, n_images)
        np.random.seed(seed)
        get_training_roidb(imdb)
        tr = trainer(R.filler_head(9, **dims), 3)
        sw = SolverWrapper(sol, imdb, str(d / "out"), trainer=tr, backbone=StubBackbone(), ctx=R.ShapeOnlyBlobCtx(), seed=11)
    finally:
        rdl.set_backend(None)
    return sw


# ---- 3. one accumulating iteration ---------------------------------------------------------------------------------------------
def test_existing_stub_trainers_still_run_without_the_new_calls(tmp_path):
    """A trainer without set_accumulate / set_precision (the stubs of the older host tests) serves iter_size 1."""
    sw = az_wrapper(tmp_path, trainer=BareTrainer)
    calls = sw.trainer.calls
    assert not any(hasattr(sw.trainer, n) for n in ("set_accumulate", "set_precision", "read_history", "load_history"))
    got = sw.step(az_blobs(2.0))
    assert [c[0] for c in calls] == ["step", "update"] and calls[0] == ("step", 0, 0, 2.0)
    assert bits(sw.losses[0]) == bits(got) and sw.iter == 1
    assert calls[1][4] == sw.last_clip == 2.0 / np.sqrt(27.0)             # (n = 1: the clip itself, not clip / 1.0 of another type)


def test_iter_size_three_order_scale_rate_and_losses(tmp_path):
    from detect.solver import clip_scale, learning_rate
    n = 3
    sw = az_wrapper(tmp_path, iter_size=n)
    tr = sw.trainer
    assert sw.iter_size == n
    want_losses = []
    for it in range(5):
        del tr.calls[:]
        mbs = [az_blobs(float(10 * it + k)) for k in range(n)]
        got = sw.step(mbs)
        steps = [c for c in tr.calls if c[0] == "step"]
        # flags 0, 1, 1 set before their sub-steps; dropout iterations iter * n + k; one update, last
        assert [c[0] for c in tr.calls] == ["acc", "step"] * n + ["update"]
        assert [c[1] for c in tr.calls if c[0] == "acc"] == [0, 1, 1]
        assert [(c[1], c[2], c[3]) for c in steps] == [(int(k > 0), it * n + k, float(10 * it + k)) for k in range(n)]
        sumsq = sum(9.0 * (1.0 + 10 * it + k) for k in range(n))
        clip = clip_scale(sumsq, SOLVER["clip_gradients"])
        assert clip < 1.0 and sw.last_sumsq == sumsq and sw.last_clip == clip
        rate = learning_rate(sw.solver_param, it)                           # from iter, which counts iterations
        assert tr.calls[-1] == ("update", rate, SOLVER["momentum"], SOLVER["weight_decay"], clip / n)
        assert sw.last_scale == clip / n and sw.last_rate == rate
        rows = [np.asarray([10 * it + k + 0.1 * i + 1e-3 * (it * n + k) for i in range(3)], np.float32) for k in range(n)]
        mean = ((rows[0] + rows[1]) + rows[2]) / np.float32(n)            # Caffe: loss /= iter_size, in float32
        assert mean.dtype == np.float32 and bits(got) == bits(mean) and bits(sw.losses[-1]) == bits(mean)
        want_losses.append(mean)
    assert sw.iter == 5 and learning_rate(sw.solver_param, 3) == 0.005 and len(sw.losses) == 5
    # what step() takes
    for bad in (az_blobs(1.0), [az_blobs(1.0)] * 2, [az_blobs(1.0)] * 4, [az_blobs(1.0), az_blobs(2.0), 5]):
        del tr.calls[:]
        with pytest.raises(ValueError, match="iter_size"):
            sw.step(bad)
        assert tr.calls == [] and sw.iter == 5
    # n = 1 takes a dict, or a list of one
    sw1 = az_wrapper(tmp_path, name="b")
    sw1.step(az_blobs(1.0))
    sw1.step([az_blobs(1.0)])
    assert [c[0] for c in sw1.trainer.calls] == ["step", "update"] * 2 and [c[2] for c in sw1.trainer.calls if c[0] == "step"] == [0, 1]
    with pytest.raises(ValueError, match="iter_size"):
        sw1.step([az_blobs(1.0)] * 2)


def test_iter_size_draws_n_minibatches_per_iteration(tmp_path):
    from az_data_layer.layer import AZDataLayer
    sw = az_wrapper(tmp_path, n_images=4, iter_size=2, seed=5)
    state = np.random.get_state()
    drawn = []
    sw.layer.forward = lambda f=AZDataLayer._get_next_minibatch_inds: drawn.append(f(sw.layer).copy()) or az_blobs(float(len(drawn)))
    perm0, cur0 = sw.layer._perm.copy(), sw.layer._cur
    for _ in range(3):
        sw.step()
    assert len(drawn) == 6 and sw.iter == 3
    # a plain layer advanced as often from the same stream lands on the same permutation and cursor
    np.random.set_state(state)
    plain = AZDataLayer(ctx=R.ShapeOnlyBlobCtx())
    plain._roidb, plain._perm, plain._cur = sw.layer._roidb, perm0.copy(), cur0
    want = [plain._get_next_minibatch_inds().copy() for _ in range(6)]
    assert all(np.array_equal(a, b) for a, b in zip(drawn, want))
    assert np.array_equal(plain._perm, sw.layer._perm) and plain._cur == sw.layer._cur


# ---- 4. the state file -----------------------------------------------------------------------------------------------------------
def run(sw, its, first):
    for it in range(first, first + its):
        sw.step([az_blobs(float(3 * it + k)) for k in range(sw.iter_size)])


def everything(sw):
    out = [np.int64(sw.iter), np.int64(sw.seed), sw.layer._perm, np.int64(sw.layer._cur), np.asarray(sw.losses[-3:], np.float32)]
    out += [sw.trainer.p[k] for k in sorted(sw.trainer.p)] + [sw.trainer.h[k] for k in sorted(sw.trainer.h)]
    st = np.random.get_state()
    return [bits(np.asarray(x)) for x in out + [st[1], np.int64(st[2]), np.int64(st[3]), np.float64(st[4])]]


def test_state_round_trip_and_refusals(tmp_path, monkeypatch):
    from detect.config import cfg
    sw = az_wrapper(tmp_path, iter_size=2)
    run(sw, 4, 0)
    np.random.standard_normal(3)                                            # (an odd count: a cached gaussian is part of the stream)
    assert np.random.get_state()[3] == 1
    assert sw.state_path() == str(tmp_path / "a" / "out" / "st_iter_4.solverstate")
    path = sw.save_state()
    assert path == sw.state_path() and os.path.exists(path) and not os.path.exists(path + ".npz")
    saved = everything(sw)
    draws = np.random.random(1000)
    with np.load(path, allow_pickle=False) as z:
        st = {k: z[k] for k in z.files}
    assert int(st["format"]) == 1 and str(st["kind"]) == "az" and int(st["iter"]) == 4 and int(st["iter_size"]) == 2 and int(st["seed"]) == 11
    assert set(st) >= set(["w_" + k for k in R.KEYS] + ["h_" + k for k in R.KEYS] + ["bbox_means", "bbox_stds", "rng_keys", "rng_pos",
                           "rng_has_gauss", "rng_cached_gaussian", "layer_perm", "layer_cur", "roidb_len", "losses"])
    assert st["losses"].shape == (3, 3) and bits(st["losses"]) == bits(np.asarray(sw.losses[-3:]))       # average_loss rows
    assert bits(st["w_Wab"]) == bits(sw.trainer.p["Wab"]) and st["h_W6"].any()                           # as the trainer holds them
    assert int(st["roidb_len"]) == 4 and bits(st["bbox_stds"]) == bits(sw.bbox_stds)
    # a wrapper built and seeded the same way, elsewhere in its own stream, takes everything back
    sw2 = az_wrapper(tmp_path, iter_size=2, name="b")
    np.random.seed(99)
    assert everything(sw2) != saved
    assert sw2.restore(path) == 4
    assert everything(sw2) == saved
    assert np.array_equal(np.random.random(1000), draws)                    # the next 1000 draws
    run(sw, 2, 4)
    run(sw2, 2, 4)
    assert everything(sw)[:-4] == everything(sw2)[:-4] and sw2.iter == 6
    assert [c for c in sw.trainer.calls if c[0] == "update"][-2:] == [c for c in sw2.trainer.calls if c[0] == "update"]
    # cfg.TRAIN.SNAPSHOT_STATE: snapshot() writes the state beside the .caffemodel; without it, none
    snap = sw.snapshot()
    assert not os.path.exists(snap.replace(".caffemodel", ".solverstate"))
    monkeypatch.setattr(cfg.TRAIN, "SNAPSHOT_STATE", True)
    monkeypatch.setattr(cfg.TRAIN, "SNAPSHOT_INFIX", "x")
    snap = sw.snapshot()
    assert snap.endswith("st_x_iter_6.caffemodel") and os.path.exists(snap.replace(".caffemodel", ".solverstate"))
    monkeypatch.setattr(cfg.TRAIN, "SNAPSHOT_INFIX", "")

    # ---- refusals: a ValueError that names what differs; iter, weights, history, stream, layer untouched
    def refused(target, file, what):
        np.random.seed(7)
        before = everything(target)
        with pytest.raises(ValueError, match=what):
            target.restore(file)
        assert everything(target) == before

    def edited(name, **kw):
        out = str(tmp_path / name)
        with open(out, "wb") as f:
            np.savez(f, **dict(st, **kw))
        return out
    fresh = az_wrapper(tmp_path, iter_size=2, name="c")
    refused(az_wrapper(tmp_path, iter_size=2, dims=dict(AZ_DIMS, n6=132), name="d"), path, "w_W6|h_W6|w_W71|h_W71")     # a changed n6
    refused(az_wrapper(tmp_path, n_images=3, iter_size=2, name="e"), path, "roidb")                    # a roidb of another length
    refused(az_wrapper(tmp_path, iter_size=1, name="f"), path, "iter_size")
    stds = st["bbox_stds"].copy()
    stds[5] = np.nextafter(stds[5], np.inf)
    refused(fresh, edited("ulp.solverstate", bbox_stds=stds), "bbox_stds")                           # off by one ulp
    refused(fresh, edited("kind.solverstate", kind=np.array("det")), "kind")
    refused(fresh, edited("fmt.solverstate", format=np.int64(2)), "format")
    less = {k: v for k, v in st.items() if k != "h_bz"}
    with open(str(tmp_path / "less.solverstate"), "wb") as f:
        np.savez(f, **less)
    refused(fresh, str(tmp_path / "less.solverstate"), "h_bz")
    raw = open(path, "rb").read()
    for cut in (len(raw) // 2, 100, 0):                                     # a truncated file
        with open(str(tmp_path / "cut.solverstate"), "wb") as f:
            f.write(raw[:cut])
        refused(fresh, str(tmp_path / "cut.solverstate"), "cannot be read|solver state")
    assert fresh.restore(path) == 4 and everything(fresh) == saved          # (and the good file still goes in)


def test_a_det_state_into_the_az_wrapper_and_back(tmp_path, monkeypatch):
    import det_step_ref as D
    from detect.train_det import SolverWrapper
    from roi_data_layer import roidb as rdl
    g = np.load(GOLD)
    rdl.set_backend(DR.RefBackend())
    try:
        imdb, _, _ = DR.synthetic_roidb(rdl, g, tmp_path, monkeypatch)
        for e in imdb.roidb:
            del e["bbox_targets"], e["max_overlaps"]
        tr = RecordingTrainer(D.filler_head(9, 16, 128, 96, 21), 2)
        det = SolverWrapper(D.traj_solver_files(str(tmp_path)), imdb, str(tmp_path / "out"), trainer=tr, backbone=StubBackbone(),
                            ctx=R.ShapeOnlyBlobCtx(), seed=4)
    finally:
        rdl.set_backend(None)
    assert len(imdb.roidb) == 16 and det._state_kind() == "det"
    path = det.save_state(str(tmp_path / "det.solverstate"))
    with np.load(path, allow_pickle=False) as z:
        assert str(z["kind"]) == "det" and z["layer_perm"].shape == (16,) and z["losses"].shape == (0, 2)
    az = az_wrapper(tmp_path, name="az")
    az_path = az.save_state()
    for target, file in ((az, path), (det, az_path)):
        before = everything(target)
        with pytest.raises(ValueError, match="kind"):
            target.restore(file)
        assert everything(target) == before
    assert det.restore(path) == 0 and az.restore(az_path) == 0
