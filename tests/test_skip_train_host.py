"""CPU: the host side of training the skip-connection detector -- the hand-written backward of tests/skip_train_ref.py
against torch.autograd in float64, the skip train net's reader and writer, SolverWrapper's configuration checks and the
binding's symbol table.

No Caffe GRN source exists, so the restatement's backward (the yardstick of the GPU tests) is checked here against
something independent: autograd over a torch statement of the same forward.  The window maximum is taken by an explicit
gather at the restatement's arg-max indices (amax would split a tie's gradient); the maps are continuous-valued, so there
are no ties.  Float64 rounding over sums of at most ~25 000 terms is ~1e-11: every gradient must agree to 1e-9 relative.

The three tests of the restatement itself (autograd, all-zero source, float32 closeness) exercise tests/skip_train_ref.py and
torch only: they validate the yardstick and do not depend on the library.  The reference's own finetune/ and frozen/ train
nets are read when AZ_REFERENCE_ROOT names the reference tree (as tests/gen_golden_*.py take it)."""
import copy
import os
import re

import numpy as np
import pytest

import skip_ref as S
import skip_train_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP_YML = os.path.join(REPO, "tests", "golden", "voc_skip.yml")
REF_ROOT = os.environ.get("AZ_REFERENCE_ROOT", "")                     # (as tests/gen_golden_*.py)
REF_NETS = os.path.join(REF_ROOT, "models", "COCO", "VGG16_skip", "frcnn")
TOL = 1e-9


@pytest.fixture
def cfg():
    from detect import config as C
    saved = copy.deepcopy(dict(C.cfg))
    yield C.cfg
    S.restore_tree(C.cfg, saved)


# ---- the backward against autograd -----------------------------------------------------------------------------------------------
def continuous_maps(seed, Cs, N, zero=()):
    rng = np.random.Generator(np.random.PCG64(seed))
    maps = [rng.standard_normal((N, C, h, w)).astype(np.float32) for C, (h, w) in zip(Cs, S.MAP_HW)]
    for i in zero:
        maps[i][:] = 0.0
    return maps


def autograd_front(front, maps, rois, arg, G, Cs):
    """loss = sum(pool5 * G) through a torch float64 statement of the front; returns (pool5, g_Wp, g_bp, [d map])."""
    import torch
    tm = [torch.tensor(m, dtype=torch.float64, requires_grad=True) for m in maps]
    Wp = torch.tensor(front["Wp"], dtype=torch.float64, requires_grad=True)
    bp = torch.tensor(front["bp"], dtype=torch.float64, requires_grad=True)
    off = T.offsets(Cs)
    n_of_row = torch.tensor(np.repeat(rois[:, 0].astype(np.int64), 49))
    blocks = []
    for i, m in enumerate(tm):
        N, C, H, W = m.shape
        a = torch.tensor(arg[:, off[i]:off[i + 1]].astype(np.int64))
        lin = (n_of_row[:, None] * C + torch.arange(C)[None, :]) * (H * W) + a.clamp(min=0)
        x = torch.where(a >= 0, m.reshape(-1)[lin], torch.zeros((), dtype=torch.float64))      # an empty bin pools to 0
        ss = (x * x).sum(dim=1, keepdim=True) + front["eps"]
        blocks.append(front["gain"] * x / torch.sqrt(ss))
    cat = torch.cat(blocks, dim=1)
    y = torch.relu(cat @ Wp.T + bp)
    Rn = rois.shape[0]
    pool5 = y.reshape(Rn, 49, -1).permute(0, 2, 1).reshape(Rn, -1)
    (pool5 * torch.tensor(G)).sum().backward()
    return pool5.detach().numpy(), Wp.grad.numpy(), bp.grad.numpy(), [m.grad.numpy() for m in tm]


def run_both(front, maps, rois, seed=5):
    Cs = tuple(m.shape[1] for m in maps)
    raw, arg = T.pool_argmax(maps, rois)
    fw = T.front_forward(front, raw, Cs)
    G = np.random.Generator(np.random.PCG64(seed)).standard_normal(fw["pool5"].shape)
    bw = T.front_backward(fw, G, Cs, arg, rois, [m.shape for m in maps])
    return fw, bw, autograd_front(front, maps, rois, arg, G, Cs)


def report(name, got, ref):
    e = T.rel_err(got, ref)
    print("  %-10s restatement vs autograd %.3e (max |ref| %.3e)" % (name, e, float(np.abs(ref).max())))
    return e


def test_front_backward_matches_autograd_float64():
    d = T.SMALL
    maps = continuous_maps(3, d["Cs"], 2)
    rois = np.vstack([S.hostile_rois(), S.random_rois(12)])
    rois[:, 0] = np.arange(rois.shape[0]) % 2
    front = T.make_front(9, d["Cs"], d["Cout"])
    fw, bw, (p5, gW, gb, dm) = run_both(front, maps, rois)
    assert (fw["pool5"] > 0).mean() > 0.2 and (fw["pool5"] == 0).mean() > 0.2          # the ReLU gate is exercised
    errs = [report("pool5", fw["pool5"], p5), report("g_Wp", bw["g_Wp"], gW), report("g_bp", bw["g_bp"], gb)]
    errs += [report("d map %d" % i, bw["dmaps"][i], dm[i]) for i in range(3)]
    assert all(np.abs(x).max() > 0 for x in dm)
    assert max(errs) <= TOL


@pytest.mark.parametrize("zero", [0, 2])
def test_all_zero_source(zero):
    d = T.SMALL
    maps = continuous_maps(4, d["Cs"], 1, zero=(zero,))
    rois = S.random_rois(8)
    # eps > 0: finite, and autograd's
    front = T.make_front(9, d["Cs"], d["Cout"], eps=1e-10)
    fw, bw, (p5, gW, gb, dm) = run_both(front, maps, rois)
    assert all(np.isfinite(x).all() for x in bw["dmaps"]) and np.isfinite(bw["g_Wp"]).all()
    errs = [report("g_Wp", bw["g_Wp"], gW), report("g_bp", bw["g_bp"], gb)] + [report("d map %d" % i, bw["dmaps"][i], dm[i]) for i in range(3)]
    assert max(errs) <= TOL
    assert np.abs(bw["dmaps"][zero]).max() > 0            # (x = 0: y = 0, but dy/dx = gain / sqrt(eps) is not)
    # eps = 0: zeros for the all-zero source, never NaN
    front0 = dict(front, eps=0.0)
    Cs = d["Cs"]
    raw, arg = T.pool_argmax(maps, rois)
    fw0 = T.front_forward(front0, raw, Cs)
    G = np.random.Generator(np.random.PCG64(5)).standard_normal(fw0["pool5"].shape)
    bw0 = T.front_backward(fw0, G, Cs, arg, rois, [m.shape for m in maps])
    off = T.offsets(Cs)
    assert not fw0["cat"][:, off[zero]:off[zero + 1]].any() and not bw0["dmaps"][zero].any()
    assert all(np.isfinite(x).all() for x in bw0["dmaps"]) and np.isfinite(bw0["g_Wp"]).all() and np.isfinite(bw0["d_raw"]).all()
    assert all(np.abs(bw0["dmaps"][i]).max() > 0 for i in range(3) if i != zero)


def test_float32_restatement_is_close():
    """The float32 run that sets the GPU tests' bounds is the same computation: within 1e-4 of float64 on SMALL."""
    head, front, maps, blobs = T.case("small")
    masks = None
    r64 = T.step(head, front, maps, blobs, masks)
    r32 = T.step(head, front, maps, blobs, masks, gates=r64["gates"], dtype=np.float32)
    for k in ("cat", "pool5", "d_y", "d_cat", "d_raw"):
        assert T.rel_err(r32[k], r64[k]) < 1e-4, k
    assert all(T.rel_err(a, b) < 1e-4 for a, b in zip(r32["dmaps"], r64["dmaps"]))
    assert len(r64["grads"]) == 10 and r64["grads"]["Wp"].shape == front["Wp"].shape


# ---- the train net ---------------------------------------------------------------------------------------------------------------
def edited(text, old, new):
    assert text.count(old) >= 1, old
    return text.replace(old, new, 1)


def test_read_skip_train_net(tmp_path):
    from detect import prototxt as P
    path = str(tmp_path / "train_skip.prototxt")
    P.write_skip_train_prototxt(path, P.skip_layer_table())
    table, front = P.read_skip_train_net(path)
    assert front["sources"] == ["conv3_3", "conv4_3", "conv5_3"] and front["scales"] == [0.25, 0.125, 0.0625] and front["gain"] == 1000.0
    assert set(table) == set(P.CONV_LAYERS + P.SKIP_HEAD_LAYERS) and "conv_pool5" not in P.CONV_LAYERS
    assert table["conv_pool5"] == {"lr_mult": [1.0, 2.0], "decay_mult": [1.0, 0.0], "dropout_ratio": None, "std": None}
    assert all(table[n]["lr_mult"] == [0.0, 0.0] for n in P.CONV_LAYERS)               # the frozen/ net
    assert table["fc6"]["dropout_ratio"] == 0.5 and table["cls_score"]["std"] == 0.01
    P.write_skip_train_prototxt(path, P.skip_layer_table(frozen=P.CONV_LAYERS[:4]))
    t2, _ = P.read_skip_train_net(path)
    assert t2["conv3_1"]["lr_mult"] == [1.0, 2.0] and t2["conv2_2"]["lr_mult"] == [0.0, 0.0]
    # the plain reader still refuses the skip file, the skip reader a plain file
    with pytest.raises(ValueError, match="conv_pool5"):
        P.read_det_train_net(path)
    plain = str(tmp_path / "train_det.prototxt")
    P.write_train_prototxt(plain, P.det_layer_table(), name="frcnn_train")
    with pytest.raises(ValueError, match="conv_pool5"):
        P.read_skip_train_net(plain)
    # the refusals
    text = open(path).read()
    bad = {"power": edited(text, "power: 1\n", "power: 2\n"),
           "shift": edited(text, "shift: 0\n", "shift: 0.5\n"),
           "pooled": edited(text, "pooled_w: 7\n", "pooled_w: 6\n"),
           "GRN": re.sub(r'layer \{\n  name: "roi_norm4".*?\n\}\n', "", text, count=1, flags=re.S),
           "Concat": edited(text, '  bottom: "roi_pool3"\n  bottom: "roi_pool4"\n', '  bottom: "roi_pool4"\n  bottom: "roi_pool3"\n')}
    assert bad["GRN"] != text
    for what, t in bad.items():
        q = str(tmp_path / ("bad_%s.prototxt" % what))
        with open(q, "w") as f:
            f.write(t)
        with pytest.raises(ValueError):
            P.read_skip_train_net(q)
        print("  refused:", what)


def test_reference_train_nets_when_present():
    from detect import prototxt as P
    fin, fro = (os.path.join(REF_NETS, d, "train.prototxt") for d in ("finetune", "frozen"))
    if not REF_ROOT or not (os.path.exists(fin) and os.path.exists(fro)):
        pytest.skip("AZ_REFERENCE_ROOT does not name the reference tree")
    (tf, ff), (tz, fz) = P.read_skip_train_net(fin), P.read_skip_train_net(fro)
    assert ff == fz == {"sources": ["conv3_3", "conv4_3", "conv5_3"], "scales": [0.25, 0.125, 0.0625], "gain": 1000.0}
    differ = [n for n in tf if tf[n] != tz[n]]
    assert differ == list(P.CONV_LAYERS[4:]) and 2 * len(differ) == 18                 # 18 param rows: conv3_1 .. conv5_3
    for n in differ:
        assert tf[n]["lr_mult"] + tf[n]["decay_mult"] == [1.0, 2.0, 1.0, 0.0]
        assert tz[n]["lr_mult"] + tz[n]["decay_mult"] == [0.0, 0.0, 0.0, 0.0]
    assert tf["conv_pool5"] == tz["conv_pool5"] and tf["conv_pool5"]["lr_mult"] == [1.0, 2.0]


# ---- SolverWrapper's configuration checks -----------------------------------------------------------------------------------------
class _Imdb(object):
    num_classes = 21

    @property
    def roidb(self):
        raise AssertionError("the roidb was touched before the configuration was checked")


def _solver_files(tmp_path, skip, sources=None):
    from detect import prototxt as P
    net = str(tmp_path / ("net_%d.prototxt" % len(os.listdir(str(tmp_path)))))
    if skip:
        P.write_skip_train_prototxt(net, P.skip_layer_table(), sources=sources or P.SKIP_SOURCES)
    else:
        P.write_train_prototxt(net, P.det_layer_table(), name="frcnn_train")
    sol = net.replace("net_", "solver_")
    P.write_solver_prototxt(sol, net, snapshot_prefix="x")
    return sol


def test_solver_wrapper_refuses_mismatched_configurations(cfg, tmp_path, monkeypatch):
    from aznet_hip import ffi
    from detect import config as C
    from detect.train_det import SolverWrapper

    def no_context(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(ffi, "AzContext", no_context)
    monkeypatch.setattr(ffi, "default_context", no_context)
    assert len(cfg.SEAR.FRCNN_CONV) == 1
    with pytest.raises(ValueError, match="conv_pool5"):                                # a skip net under the plain configuration
        SolverWrapper(_solver_files(tmp_path, True), _Imdb(), str(tmp_path / "o"))
    C.cfg_from_file(SKIP_YML)
    assert list(cfg.SEAR.FRCNN_CONV) == ["conv3_3", "conv4_3", "conv5_3"]
    with pytest.raises(ValueError, match="conv_pool5"):                                # a plain net under the skip configuration
        SolverWrapper(_solver_files(tmp_path, False), _Imdb(), str(tmp_path / "o"))
    with pytest.raises(ValueError, match="FRCNN_CONV"):                                # other sources than the configuration's
        SolverWrapper(_solver_files(tmp_path, True, sources=("conv2_2", "conv4_3", "conv5_3")), _Imdb(), str(tmp_path / "o"))
    # the matching pair gets past the checks (and then reaches the roidb)
    with pytest.raises(AssertionError, match="roidb was touched"):
        SolverWrapper(_solver_files(tmp_path, True), _Imdb(), str(tmp_path / "o"))


# ---- the binding --------------------------------------------------------------------------------------------------------------------
NEW = ("az_det_solver_attach_skip", "az_det_solver_load_skip", "az_det_solver_read_skip", "az_det_solver_set_skip_hyper",
       "az_det_solver_step_skip", "az_det_solver_forward_test_skip", "az_skip_pool_bwd_unit")


def test_symbols_and_header_agree_on_the_new_entries():
    from aznet_hip import ffi
    src = open(os.path.join(REPO, "include", "aznet_hip.h")).read()
    L = ffi.load_library()
    for n in NEW:
        assert n in ffi.SYMBOLS and re.search(r"\bint\s+%s\s*\(" % n, src) and hasattr(L, n), n
    for m in ("attach_skip", "load_skip", "read_skip", "set_skip_hyper", "step_skip", "forward_test_skip"):
        assert callable(getattr(ffi.AzDetSolver, m)), m
    for name in ("cat", "skip_argmax", "skip_factor", "d_y", "d_cat", "d_raw", "g_Wp", "g_bp", "h_Wp", "h_bp", "w_Wp", "w_bp"):
        assert name in src, name


def test_forward_train_taps_are_in_the_graph():
    import torch
    from aznet_hip.backbone import VGG16Conv5
    bk = VGG16Conv5(device="cpu", seed=3, width_div=32)
    blob = np.random.RandomState(0).uniform(-100, 100, (1, 3, 48, 64)).astype(np.float32)
    bk.set_trainable([])
    plain = bk.forward_train(blob)
    assert isinstance(plain, torch.Tensor)                                             # without taps: unchanged
    bk.set_trainable(["conv4_1", "conv5_3"])
    x, taps = bk.forward_train(blob, taps=("conv3_3", "conv4_3", "conv5_3"))
    assert torch.equal(x, plain) and torch.equal(taps[2], x)
    assert [tuple(t.shape[2:]) for t in taps] == [(12, 16), (6, 8), (3, 4)]
    assert [t.requires_grad for t in taps] == [False, True, True]
    torch.autograd.backward(taps[1:], [torch.ones_like(t) for t in taps[1:]])
    conv = {l[0]: l for l in bk.layers if l is not None}
    assert conv["conv4_1"][1].grad is not None and conv["conv5_3"][1].grad is not None and conv["conv3_3"][1].grad is None
    with pytest.raises(ValueError):
        bk.forward_train(blob, taps=("conv9_9",))


# ---- the frozen 20-step run on the CPU ---------------------------------------------------------------------------------------------
def test_frozen_skip_run_restatement_lowers_the_loss(cfg, tmp_path, monkeypatch):
    """The GPU front-door test requires the summed loss of the last five of 20 steps to lie below that of the first five.
    That must first hold, with room, for the float64 restatement at the recorded base_lr: the data layer answered by the
    NumPy restatement, the frozen backbone and the image front-end on the CPU, conv_pool5 from the xavier filler."""
    import torch
    import det_step_ref as D
    import det_train_ref as DR
    from detect import config as C, prototxt as P
    from roi_data_layer import roidb as rdl
    from roi_data_layer.layer import RoIDataLayer
    K = 21
    g = np.load(os.path.join(REPO, "tests", "golden", "g21_train_det.npz"))
    C.cfg_from_file(SKIP_YML)
    rdl.set_backend(DR.RefBackend())
    try:
        imdb, _, _ = DR.synthetic_roidb(rdl, g, tmp_path, monkeypatch)
        tr = T.TRAJ
        np.random.seed(tr["np_seed"])
        layer = RoIDataLayer(K, ctx=D.TorchBlobCtx())
        layer.set_roidb(imdb.roidb)
        bb = T.traj_backbone("cpu")
        conv = {l[0]: l[1] for l in bb.layers if l is not None}
        Cs = tuple(int(conv[n].shape[0]) for n in P.SKIP_SOURCES)
        Cout = bb.out_channels
        rng = np.random.Generator(np.random.PCG64(tr["solver_seed"]))
        shapes = {"W6": (tr["n6"], Cout * 49), "W7": (tr["n7"], tr["n6"]), "Wc": (K, tr["n7"]), "Wb": (4 * K, tr["n7"])}
        std = {"W6": P.DET_FILLER_DEFAULT, "W7": P.DET_FILLER_DEFAULT, "Wc": 1e-2, "Wb": 1e-3}
        head = {k: (rng.standard_normal(shapes[k]) * std[k]).astype(np.float32) if k in shapes else
                np.zeros(shapes["W" + k[1:]][0], np.float32) for k in D.KEYS}
        ref = T.RefTrajectory(head, T.xavier_front(tr["solver_seed"], Cs, Cout), np.float64, tr["solver"])
        tot = []
        for _ in range(tr["steps"]):
            b = layer.forward()
            with torch.no_grad():
                _, taps = bb.forward_train(b["data"], taps=P.SKIP_SOURCES)
            tot.append(float(ref.step([t.numpy() for t in taps], b, tr["solver_seed"])["losses"].sum()))
    finally:
        rdl.set_backend(None)
    first, last = sum(tot[:5]), sum(tot[-5:])
    print("float64 restatement, frozen skip run at base_lr %g: first five %.4f, last five %.4f" % (tr["solver"]["base_lr"], first, last))
    print("  per step: " + " ".join("%.3f" % t for t in tot))
    assert last < 0.9 * first, (first, last)
