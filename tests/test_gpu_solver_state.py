"""GPU: gradient accumulation (az_solver_set_accumulate / az_det_solver_set_accumulate, Caffe's iter_size) and the resumable
solver state (the *_load_history entries, SolverWrapper.save_state / restore, the tools' --snapshot-state / --restore), on the
AZ-net trainer, the detection trainer and the detection trainer with the skip front, in fp32 and bf16.

Everything here is an equality of bits: an accumulated gradient is the NumPy float32 sum of the gradients the same steps write
alone, a loaded history is what was handed over, a resumed run is the run that never stopped.  The one measured figure is
printed by test_iter_size_two_sums_the_convolutions_gradients (run with -s)."""
import contextlib
import copy
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import det_step_ref as D
import det_train_ref as DR
import skip_ref as S
import skip_train_ref as T
import train_step_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "g21_train_det.npz")
SKIP_YML = os.path.join(REPO, "tests", "golden", "voc_skip.yml")
KINDS = ("az", "det", "skip")
PRECS = ("fp32", "bf16")
# the edge sizes of det_step_ref.HEADS["coco"]: no layer a multiple of the 128 x 128 tile, more than one tile in every product
C, N6, N7, NCLS, N72 = 44, 260, 516, 81, 132
MAP_H, MAP_W = D.MAP_H, D.MAP_W


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bits(a) == bits(b)


# ---- the three trainers behind one face -------------------------------------------------------------------------------------
class Rig(object):
    """One of the three trainers on the reduced head, its maps on the device, and minibatches of any row count."""

    def __init__(self, ctx, kind, prec):
        import torch
        from aznet_hip import synth
        self.ctx, self.kind, self.prec = ctx, kind, {"fp32": 0, "bf16": 1}[prec]
        self.front = None
        if kind == "az":
            self.head = R.filler_head(7, C=C, n6=N6, n71=N7, n72=N72)
            self.keys = R.KEYS
        else:
            self.head = D.filler_head(7, C, N6, N7, NCLS)
            self.keys = D.KEYS
        if kind == "skip":
            self.front = T.make_front(9, S.SMALL_CS, C)
            self.keys = T.KEYS
            self.maps = [torch.from_numpy(m).cuda() for m in T.make_batch_maps(7, S.SMALL_CS, 2)]
        else:
            fmap = np.concatenate([synth.make_feature_map(s, C, MAP_H, MAP_W) for s in (7, 8)], axis=0)
            self.maps = torch.from_numpy(fmap).cuda()

    def trainer(self, load=True, seed=1):
        from aznet_hip import ffi
        head = self.head if load else None
        if self.kind == "az":
            t = ffi.AzSolver(self.ctx, C, N6, N7, N72, max_rois=130, seed=seed, head=head)
        else:
            t = ffi.AzDetSolver(self.ctx, C, N6, N7, NCLS, max_rois=130, seed=seed, head=head)
            if self.kind == "skip":
                t.attach_skip(S.SMALL_CS, S.SCALES, gain=self.front["gain"], eps=self.front["eps"], seed=seed,
                              front=self.front if load else None)
        t.set_precision(self.prec)
        return t

    def batch(self, seed, rows):
        if self.kind == "az":
            return R.random_blobs(seed, rows, 2, MAP_H, MAP_W)
        if self.kind == "det":
            return D.random_blobs(seed, rows, 2, MAP_H, MAP_W, NCLS)
        return T.make_blobs(seed, rows, 2, NCLS)

    def step(self, t, mb, it, seed=5):
        """(losses, sum of squares, the map gradient(s) as bytes) of one step with a map gradient asked for."""
        import torch
        if self.kind == "az":
            dm = torch.zeros_like(self.maps)
            l, sq = t.step(self.maps, mb["rois"], mb["adj_labels"], mb["adj_targets"], mb["adj_loss_weights"], mb["zoom_labels"],
                           seed, it, dmap=dm)
            return l, sq, bits(dm.cpu().numpy())
        if self.kind == "det":
            dm = torch.zeros_like(self.maps)
            l, sq = t.step(self.maps, mb["rois"], mb["labels"], mb["bbox_targets"], mb["bbox_loss_weights"], seed, it, dmap=dm)
            return l, sq, bits(dm.cpu().numpy())
        dms = [torch.zeros_like(m) for m in self.maps]
        l, sq = t.step_skip(self.maps, mb["rois"], mb["labels"], mb["bbox_targets"], mb["bbox_loss_weights"], seed, it, dmaps=dms)
        return l, sq, b"".join(bits(d.cpu().numpy()) for d in dms)

    def grads(self, t):
        return {k: t.fetch("g_" + k) for k in self.keys}

    def state(self, t):
        return {p + k: t.fetch(p + k) for p in ("w_", "h_") for k in self.keys}

    def history(self, t):
        h = t.read_history()
        if self.kind == "skip":
            h.update(t.read_skip_history())
        return h

    def load_history(self, t, h):
        t.load_history({k: v for k, v in h.items() if k not in ("Wp", "bp")})
        if self.kind == "skip":
            t.load_skip_history({k: v for k, v in h.items() if k in ("Wp", "bp")})

    def weights(self, t):
        w = t.read()
        if self.kind == "skip":
            w.update(t.read_skip())
        return w

    def load_weights(self, t, w):
        t.load({k: v for k, v in w.items() if k not in ("Wp", "bp")})
        if self.kind == "skip":
            t.load_skip({k: v for k, v in w.items() if k in ("Wp", "bp")})


def sum_of_squares(gr):
    return float(sum(np.sum(np.square(v.astype(np.float64))) for v in gr.values()))


def assert_grads(rig, t, want, what):
    got = rig.grads(t)
    for k in rig.keys:
        assert same(got[k], want[k]), "%s: g_%s" % (what, k)
    return got


# ---- 1. the sum of gradients --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
def test_accumulated_gradients_are_the_float32_sums(ctx, kind, prec):
    """Minibatches A and C have 5 rows, B has 130.  pick_split on a dW product (M = outputs, N = inputs, K = rows): K = 5 is
    one slab of 32 for every layer -- the store `*d + v` -- and K = 130 with at most 51 tiles is five slabs of 32 -- the slab
    sum `out[e] + (slabs in slab order)`: fc6 / int6 (260 x 2156: 51 tiles), fc7 / int7_1 (516 x 260: 15), int7_2, cls_score,
    bbox_pred, adj_score, adj_bbox, zoom_score (1 to 15 tiles) all alike.  conv_pool5's K is rows x 49 (245 and 6370), split in
    both.  So A-then-B adds through the slab sum, the third sub-step C through the single-slab store, and the bias gradients
    through k_solver_colsum's one add behind the row sum."""
    rig = Rig(ctx, kind, prec)
    A, B, Cc = rig.batch(31, 5), rig.batch(32, 130), rig.batch(33, 5)
    t = rig.trainer()
    alone = []
    for it, mb in enumerate((A, B, Cc)):                                 # flag off: what each step writes by itself
        l, sq, dm = rig.step(t, mb, it)
        gr = rig.grads(t)
        assert all(np.any(v) for v in gr.values()) and abs(sq / sum_of_squares(gr) - 1) <= 1e-12
        alone.append((gr, l.copy(), dm))
    gA, gB, gC = alone[0][0], alone[1][0], alone[2][0]
    t.set_accumulate(0)
    rig.step(t, A, 0)
    assert_grads(rig, t, gA, "A alone, again")
    t.set_accumulate(1)
    l, sq, dm = rig.step(t, B, 1)
    gAB = {k: gA[k] + gB[k] for k in rig.keys}                            # one float32 add per element
    assert all(v.dtype == np.float32 for v in gAB.values())
    got = assert_grads(rig, t, gAB, "A, then B accumulated")
    assert not any(same(got[k], gB[k]) for k in rig.keys)
    print("%s %s: sumsq of A + B %.17g, float64 sum of squares %.17g" % (kind, prec, sq, sum_of_squares(got)))
    assert abs(sq / sum_of_squares(got) - 1) <= 1e-12                    # the norm is the accumulated buffers'
    assert same(l, alone[1][1]) and dm == alone[1][2]                    # losses and map gradients stay the step's own
    l, sq, dm = rig.step(t, Cc, 2)
    gABC = {k: gAB[k] + gC[k] for k in rig.keys}
    got = assert_grads(rig, t, gABC, "A, B, then C accumulated")
    assert abs(sq / sum_of_squares(got) - 1) <= 1e-12 and same(l, alone[2][1]) and dm == alone[2][2]
    t.close()
    # the flag on from the first step after create: zeros + gA (a -0 of the step becomes +0, as NumPy's add makes it)
    t = rig.trainer()
    t.set_accumulate(1)
    l, sq, dm = rig.step(t, A, 0)
    got = assert_grads(rig, t, {k: np.zeros_like(gA[k]) + gA[k] for k in rig.keys}, "zeros + A")
    assert abs(sq / sum_of_squares(got) - 1) <= 1e-12 and same(l, alone[0][1]) and dm == alone[0][2]
    t.close()


# ---- 2. the flag's edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
def test_flag_edges(ctx, kind, prec):
    from aznet_hip import ffi
    rig = Rig(ctx, kind, prec)
    A, B = rig.batch(31, 5), rig.batch(32, 130)
    t = rig.trainer()
    rig.step(t, A, 0)
    gA = rig.grads(t)
    rig.step(t, B, 1)
    gB = rig.grads(t)
    gAB = {k: gA[k] + gB[k] for k in rig.keys}
    for bad in (2, -1):                                                     # refused while off: stays off
        with pytest.raises(ffi.AzError) as e:
            t.set_accumulate(bad)
        assert e.value.code == ffi.AZ_ERR_INVALID
    rig.step(t, A, 0)
    assert_grads(rig, t, gA, "after a refused value the flag is still off")
    t.set_accumulate(1)
    for bad in (2, -1):                                                     # refused while on: stays on
        with pytest.raises(ffi.AzError) as e:
            t.set_accumulate(bad)
        assert e.value.code == ffi.AZ_ERR_INVALID
    rig.step(t, B, 1)
    assert_grads(rig, t, gAB, "after a refused value the flag is still on")
    # an update between two accumulating steps leaves the flag alone (rate 0, momentum 0, decay 0: the weights keep their
    # bits, the history stays zero, the gradients are only read)
    before = rig.state(t)
    t.set_accumulate(0)
    rig.step(t, A, 0)
    t.set_accumulate(1)
    t.update(0.0, 0.0, 0.0, 1.0)
    after = rig.state(t)
    assert all(same(before[k], after[k]) for k in before)
    rig.step(t, B, 1)
    assert_grads(rig, t, gAB, "an update does not clear the flag")
    # off after on: overwrites again, the plain step's bits
    t.set_accumulate(0)
    rig.step(t, B, 1)
    assert_grads(rig, t, gB, "off after on")
    t.close()


# ---- 3. history -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
def test_history_loads_reads_and_carries_a_run_over(ctx, kind, prec):
    from aznet_hip import ffi
    from detect.solver import clip_scale
    rig = Rig(ctx, kind, prec)
    t = rig.trainer()
    shp = t._shapes()
    rng = np.random.Generator(np.random.PCG64(3))
    h1 = {k: rng.standard_normal(shp[k]).astype(np.float32) for k in rig.keys}
    w0 = rig.weights(t)
    rig.load_history(t, h1)
    got = rig.history(t)
    assert set(got) == set(rig.keys) and all(same(got[k], h1[k]) and got[k].shape == shp[k] for k in rig.keys)
    assert all(same(t.fetch("h_" + k), h1[k]) for k in rig.keys)
    # a partial load keeps the rest; an empty one keeps everything; the weights are not touched
    w7 = "W71" if kind == "az" else "W7"
    part = {w7: np.float32(2) * h1[w7], "b6": -h1["b6"]}
    t.load_history(part)
    t.load_history({})
    if kind == "skip":
        t.load_skip_history({"bp": h1["bp"] + np.float32(1)})
        part["bp"] = h1["bp"] + np.float32(1)
        t.load_skip_history({})
    got = rig.history(t)
    assert all(same(got[k], part.get(k, h1[k])) for k in rig.keys)
    now = rig.weights(t)
    assert all(same(now[k], w0[k]) for k in rig.keys)
    # loading history is no step: an update still has no gradients to work with
    with pytest.raises(ffi.AzError) as e:
        t.update(0.01, 0.9, 0.0005, 1.0)
    assert e.value.code == ffi.AZ_ERR_STATE
    if kind == "det":                                                     # the skip entry without a front
        with pytest.raises(ffi.AzError) as e:
            t.load_skip_history({})
        assert e.value.code == ffi.AZ_ERR_STATE
        with pytest.raises(ffi.AzError) as e:
            t.read_skip_history()
        assert e.value.code == ffi.AZ_ERR_STATE
    t.close()
    # two real updates; weights and history into a second trainer (other fillers, nothing loaded); two more on both
    mbs = [rig.batch(40 + i, r) for i, r in enumerate((130, 37, 5, 130))]

    def advance(tr, its):
        out = []
        for it in its:
            l, sq, dm = rig.step(tr, mbs[it], it)
            tr.update(0.01 * 0.5 ** it, 0.9, 0.0005, clip_scale(sq, 0.5))
            out.append((bits(l), sq, dm))
        return out
    t1 = rig.trainer()
    advance(t1, (0, 1))
    t2 = rig.trainer(load=False, seed=99)
    assert not same(t2.fetch("w_W6"), t1.fetch("w_W6"))
    rig.load_weights(t2, rig.weights(t1))
    rig.load_history(t2, rig.history(t1))
    s1, s2 = rig.state(t1), rig.state(t2)
    assert all(same(s1[k], s2[k]) for k in s1) and all(np.any(s1["h_" + k]) for k in rig.keys)
    assert advance(t1, (2, 3)) == advance(t2, (2, 3))
    s1, s2 = rig.state(t1), rig.state(t2)
    assert all(same(s1[k], s2[k]) for k in s1)
    t1.close()
    t2.close()


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def configured(kind, bf16=False):
    """cfg under the skip configuration (kind "skip") and / or TRAIN.PRECISION = 'bf16', restored afterwards.  The skip file
    trains on one image per minibatch, with which 16 entries last 15 minibatches; here it gets the two of the other
    configurations, so that every wrapper of this file reshuffles at its eighth minibatch."""
    from detect import config as Cf
    saved = copy.deepcopy(dict(Cf.cfg))
    try:
        if kind == "skip":
            Cf.cfg_from_file(SKIP_YML)
            Cf.cfg.TRAIN.IMS_PER_BATCH = 2
        if bf16:
            Cf.cfg.TRAIN.PRECISION = "bf16"
        yield
    finally:
        S.restore_tree(Cf.cfg, saved)


def wrapper(kind, ctx, g, tmp, monkeypatch, name, iter_size=1, frozen=True, n_images=8, n6=None):
    """A SolverWrapper of the existing trajectory rigs (width_div = 32 backbone, reduced head) on synthetic_375x500_<n> with
    flips (16 entries for n = 8: the permutation is reshuffled at every eighth minibatch), built and seeded the same way at
    every call."""
    from aznet_hip import ffi, synth
    from detect import prototxt as P
    sub = tmp / name
    sub.mkdir()
    ffi.set_default_context(ctx)
    if kind == "az":
        from datasets.synthetic import SyntheticImdb
        from detect.train_az import SolverWrapper, get_training_roidb
        ref = R
        imdb = SyntheticImdb(375, 500, n_images)
        np.random.seed(R.TRAJ["roidb_seed"])
        get_training_roidb(imdb)
        sol = R.traj_solver_files(str(sub), frozen)
        dims = {k: v for k, v in synth.SMALL_DIMS.items() if k != "C"}
    else:
        from detect.train_det import SolverWrapper
        from roi_data_layer import roidb as rdl
        ref = T if kind == "skip" else D
        imdb, _, _ = DR.synthetic_roidb(rdl, g, sub, monkeypatch, n_images)
        np.random.seed(ref.TRAJ["np_seed"])
        sol = ref.traj_solver_files(str(sub), frozen_all=frozen)
        dims = dict(n6=ref.TRAJ["n6"], n7=ref.TRAJ["n7"])
    if n6 is not None:
        dims["n6"] = n6
    if iter_size != 1:
        P.write_solver_prototxt(sol, P.read_solver(sol)["train_net"], **dict(ref.TRAJ["solver"], iter_size=iter_size))
    sw = SolverWrapper(sol, imdb, str(sub / "out"), backbone=ref.traj_backbone("cuda:0"), ctx=ctx, dims=dims,
                       seed=ref.TRAJ["solver_seed"])
    assert len(imdb.roidb) == 2 * n_images and sw.iter_size == iter_size
    return sw


def trainer_state(sw):
    w, h = sw._trainer_state()
    return dict([("w_" + k, v) for k, v in w.items()] + [("h_" + k, v) for k, v in h.items()])


def whole_state(sw):
    """Everything the next iteration depends on, as bytes."""
    st = np.random.get_state()
    out = {k: bits(v) for k, v in trainer_state(sw).items()}
    out.update(iter=sw.iter, seed=sw.seed, perm=bits(sw.layer._perm), cur=int(sw.layer._cur), rng_keys=bits(st[1]), rng_pos=int(st[2]),
               rng_gauss=(int(st[3]), bits(np.float64(st[4]))))
    for layer in sw.backbone.layers:
        if layer is not None:
            out["conv_w_" + layer[0]], out["conv_b_" + layer[0]] = bits(layer[1].detach().cpu().numpy()), bits(layer[2].detach().cpu().numpy())
    for name, _, _, hw, hb, _, _ in sw.conv_train:
        out["conv_hw_" + name], out["conv_hb_" + name] = bits(hw.cpu().numpy()), bits(hb.cpu().numpy())
    return out


def assert_same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k] == b[k], k


# ---- 4. iter_size: 2 is the sequence written out ----------------------------------------------------------------------------------
def test_iter_size_two_is_the_manual_sequence(ctx, g, tmp_path, monkeypatch):
    from detect.solver import clip_scale, learning_rate
    from roi_data_layer.layer import RoIDataLayer
    with configured("det"):
        sw = wrapper("det", ctx, g, tmp_path, monkeypatch, "w", iter_size=2)
        hand = wrapper("det", ctx, g, tmp_path, monkeypatch, "h")         # (the same construction: the same start)
        assert_same_state({k: bits(v) for k, v in trainer_state(sw).items()}, {k: bits(v) for k, v in trainer_state(hand).items()})
        # a plain layer, advanced eight minibatches from where the wrapper's stands: the blobs of the run
        state0, perm0, cur0 = np.random.get_state(), sw.layer._perm.copy(), sw.layer._cur
        plain = RoIDataLayer(sw.num_classes, ctx=ctx)
        plain._roidb, plain._perm, plain._cur = sw.layer._roidb, perm0.copy(), cur0
        blobs = [plain.forward() for _ in range(8)]
        end = np.random.get_state()
        assert not np.array_equal(plain._perm, perm0), "eight minibatches of 2 over 16 entries reshuffle"
        np.random.set_state(state0)
        for _ in range(4):
            sw.step()
        now = np.random.get_state()
        assert sw.iter == 4 and np.array_equal(sw.layer._perm, plain._perm) and sw.layer._cur == plain._cur
        assert np.array_equal(now[1], end[1]) and now[2:] == end[2:]
        assert all(same(sw.last_blobs[k], blobs[7][k]) for k in blobs[7])
        # the second trainer by hand
        tr, sp = hand.trainer, sw.solver_param
        for it in range(4):
            pair = []
            for k in range(2):
                mb = blobs[2 * it + k]
                tr.set_accumulate(k)
                conv = hand.backbone.forward_train(mb["data"])
                l, sq = tr.step(conv.detach(), mb["rois"], mb["labels"], mb["bbox_targets"], mb["bbox_loss_weights"], sw.seed, 2 * it + k)
                pair.append(np.asarray(l, np.float32))
            tr.update(learning_rate(sp, it), sp["momentum"], sp["weight_decay"], clip_scale(sq, sp["clip_gradients"]) / 2)
            mean = (pair[0] + pair[1]) / np.float32(2)
            assert mean.dtype == np.float32 and same(sw.losses[it], mean), it
        assert learning_rate(sp, 3) == sp["base_lr"] and sw.last_rate == sp["base_lr"] and sw.last_scale == sw.last_clip / 2
        assert_same_state({k: bits(v) for k, v in trainer_state(sw).items()}, {k: bits(v) for k, v in trainer_state(hand).items()})
        assert all(np.any(v) for k, v in trainer_state(sw).items() if k.startswith("h_"))
        sw.trainer.close()
        hand.trainer.close()


# ---- 5. resume is exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,iter_size,bf16", [("az", 1, False), ("det", 1, False), ("skip", 1, False), ("det", 2, True)])
def test_resume_is_exact(ctx, g, tmp_path, monkeypatch, kind, iter_size, bf16):
    """A: ten iterations.  B: five, save_state, closed.  C: built and seeded like B, restore, five more.  C ends where A ends."""
    with configured(kind, bf16):
        mk = lambda name: wrapper(kind, ctx, g, tmp_path, monkeypatch, name, iter_size=iter_size)
        a = mk("a")
        assert a.trainer is not None and a.conv_train == [] and a._state_kind() == {"az": "az", "det": "det", "skip": "det_skip"}[kind]
        for _ in range(10):
            a.step()
        end_a, losses_a = whole_state(a), [bits(l) for l in a.losses]
        snap_a = open(a.snapshot(), "rb").read()
        a.trainer.close()
        b = mk("b")
        for _ in range(5):
            b.step()
        assert [bits(l) for l in b.losses] == losses_a[:5]
        path = b.save_state()
        assert path == os.path.join(b.output_dir, "%s_iter_5.solverstate" % b.solver_param["snapshot_prefix"])
        perm_saved, state_b = b.layer._perm.copy(), whole_state(b)
        b.trainer.close()
        with np.load(path, allow_pickle=False) as z:
            assert int(z["iter"]) == 5 and int(z["iter_size"]) == iter_size and str(z["kind"]) == a._state_kind()
            assert z["losses"].shape == (5, len(a.LOSS_NAMES))              # average_loss: 5 rows
        c = mk("c")
        np.random.seed(4711)                                                # (elsewhere in the stream until the restore)
        assert c.iter == 0 and c.restore(path) == 5
        assert_same_state(whole_state(c), state_b)
        for _ in range(5):
            c.step()
        assert c.iter == 10 and [bits(l) for l in c.losses[-5:]] == losses_a[5:]
        assert_same_state(whole_state(c), end_a)
        assert not np.array_equal(c.layer._perm, perm_saved), "the permutation was to be reshuffled after the save point"
        snap_c = c.snapshot()
        assert open(snap_c, "rb").read() == snap_a and os.path.basename(snap_c).endswith("_iter_10.caffemodel")
        c.trainer.close()


# ---- 6. trainable convolutions ------------------------------------------------------------------------------------------------------
def test_restore_puts_the_convolutions_and_the_next_minibatch_back(ctx, g, tmp_path, monkeypatch):
    b = wrapper("az", ctx, g, tmp_path, monkeypatch, "b", frozen=False)
    assert len(b.conv_train) == 9
    for _ in range(3):
        b.step()
    path = b.save_state()
    state_b = whole_state(b)
    assert all(np.any(np.frombuffer(state_b["conv_hw_" + c[0]], np.uint8)) for c in b.conv_train)
    nxt = b.layer.forward()
    b.trainer.close()
    c = wrapper("az", ctx, g, tmp_path, monkeypatch, "c", frozen=False)
    keep = [(layer[1], layer[2]) for layer in c.backbone.layers if layer is not None]
    np.random.seed(4711)
    assert c.restore(path) == 3
    assert_same_state(whole_state(c), state_b)
    # (in place: the leaves autograd and conv_train hold are the layers' own tensors still)
    assert all(layer[1] is k[0] and layer[2] is k[1] for layer, k in zip([l for l in c.backbone.layers if l is not None], keep))
    got = c.layer.forward()
    assert sorted(got) == sorted(nxt) and all(same(got[k], nxt[k]) for k in nxt)
    c.trainer.close()


def test_iter_size_two_sums_the_convolutions_gradients(ctx, g, tmp_path, monkeypatch):
    """A trainable convolution's .grad behind the two sub-steps of one iteration against the sum of the two minibatches'
    gradients taken separately: bit for bit if two backward passes of one minibatch are bit-equal on this device, else within
    8 x their observed difference.  Which of the two held is printed."""
    import torch
    sw = wrapper("az", ctx, g, tmp_path, monkeypatch, "d", iter_size=2, frozen=False)
    leaves = [p for _, w, b, _, _, _, _ in sw.conv_train for p in (w, b)]
    m0, m1 = sw.layer.forward(), sw.layer.forward()

    def alone(mb, it):
        for p in leaves:
            p.grad = None
        _, _, backward = sw._forward_backward(mb, it)
        backward()
        return [p.grad.detach().clone() for p in leaves]
    g0, g0_again, g1 = alone(m0, 0), alone(m0, 0), alone(m1, 1)
    repeat = max(float((x - y).abs().max()) for x, y in zip(g0, g0_again))
    exact = all(torch.equal(x, y) for x, y in zip(g0, g0_again))
    sw.step([m0, m1])
    worst = max(float((p.grad - (x + y)).abs().max()) for p, x, y in zip(leaves, g0, g1))
    print("two backward passes of one minibatch: %s (max |difference| %.3e); accumulated .grad against the sum: max |difference| %.3e"
          % ("bit-equal" if exact else "NOT bit-equal", repeat, worst))
    assert all(float(x.abs().max()) > 0 for x in g0 + g1)
    if exact:
        assert all(torch.equal(p.grad, x + y) for p, x, y in zip(leaves, g0, g1))
    else:
        assert worst <= 8 * repeat
    assert sw.iter == 1 and sw.last_scale == sw.last_clip / 2
    sw.trainer.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_restore_refuses_what_does_not_fit(ctx, g, tmp_path, monkeypatch):
    src = wrapper("det", ctx, g, tmp_path, monkeypatch, "s")
    for _ in range(2):
        src.step()
    path = src.save_state()
    with np.load(path, allow_pickle=False) as z:
        st = {k: z[k] for k in z.files}
    stds = st["bbox_stds"].copy()
    i = int(np.argmax(stds > 0))
    stds[i] = np.nextafter(stds[i], np.inf)
    ulp = str(tmp_path / "ulp.solverstate")
    with open(ulp, "wb") as f:
        np.savez(f, **dict(st, bbox_stds=stds))
    cut = str(tmp_path / "cut.solverstate")
    raw = open(path, "rb").read()
    with open(cut, "wb") as f:
        f.write(raw[:len(raw) // 2])
    fresh = wrapper("det", ctx, g, tmp_path, monkeypatch, "f")
    cases = [(wrapper("az", ctx, g, tmp_path, monkeypatch, "az"), path, "kind"),                       # a det state into the AZ wrapper
             (wrapper("det", ctx, g, tmp_path, monkeypatch, "n6", n6=132), path, "W6|W7"),             # a changed n6
             (wrapper("det", ctx, g, tmp_path, monkeypatch, "len", n_images=4), path, "roidb"),        # a roidb of another length
             (fresh, ulp, "bbox_stds"), (fresh, cut, "cannot be read")]
    for sw, file, what in cases:
        sw.step()                                                           # (weights and history that differ from a fresh wrapper's)
        np.random.seed(7)
        before = whole_state(sw)
        with pytest.raises(ValueError, match=what) as e:
            sw.restore(file)
        print("refused: %s" % e.value)
        assert_same_state(whole_state(sw), before)
    assert fresh.restore(path) == 2
    st_src = whole_state(src)
    assert all(whole_state(fresh)[k] == st_src[k] for k in st_src if not k.startswith("rng_"))
    for sw in [c[0] for c in cases[:4]] + [src]:
        sw.trainer.close()


# ---- 8. the tools ------------------------------------------------------------------------------------------------------------------
def test_train_det_tool_stops_and_resumes_to_the_same_snapshot():
    """tools/train_det_net.py under the skip --cfg (its written train net is frozen), each run a child process under its own
    time limit: six iterations straight; four with --snapshot-state, then --restore of that state up to six under another
    --exp.  The two snapshots at iteration 6 are the same file."""
    tool = os.path.join(REPO, "az-net_amd", "tools", "train_det_net.py")
    exps = ["solver_state_tool_%s_%d" % (n, os.getpid()) for n in ("straight", "stopped", "resumed")]
    out_dirs = [os.path.join(REPO, "az-net_amd", "output", e, "synthetic_375x500_8") for e in exps]
    base = [sys.executable, tool, "--net", "synthetic:8", "--imdb", "synthetic_375x500_8", "--cfg", SKIP_YML]
    state = os.path.join(out_dirs[1], "vgg16_fast_rcnn_skip_iter_4.solverstate")
    try:
        for exp, extra in zip(exps, (["--iters", "6"], ["--iters", "4", "--snapshot-state"], ["--iters", "6", "--restore", state])):
            out = subprocess.run(base + ["--exp", exp] + extra, capture_output=True, text=True, timeout=600)
            print(out.stdout[-1500:], out.stderr[-3000:])
            assert out.returncode == 0
        assert os.path.exists(state) and not os.path.exists(os.path.join(out_dirs[0], "vgg16_fast_rcnn_skip_iter_6.solverstate"))
        assert "Resuming from iteration 4 of 6" in out.stdout and "Iteration 0, loss" not in out.stdout
        snaps = [open(os.path.join(d, "vgg16_fast_rcnn_skip_iter_6.caffemodel"), "rb").read() for d in (out_dirs[0], out_dirs[2])]
        assert len(snaps[0]) > 1000 and snaps[0] == snaps[1]
    finally:
        for e in exps:
            shutil.rmtree(os.path.join(REPO, "az-net_amd", "output", e), ignore_errors=True)
