"""A CPU restatement of ONE training step of the skip-connection detector (test infrastructure; the yardstick of
tests/test_skip_train_host.py and tests/test_gpu_skip_train.py): skip_ref's front forward (roi_pool3/4/5 with arg-max, GRN,
concat, scale, conv_pool5 + relu_pool) in front of det_step_ref.step (fc6 .. losses and their backward, which already
returns d_pool5), and the front's backward written by hand from include/aznet_hip.h, not from the HIP code: the relu_pool
gate, g_Wp, g_bp, d_cat, the GRN + scale backward and the arg-max scatter in roi-then-bin order.  Every stage runs in
`dtype`: float64 (the reference) or float32 (what sets the tolerance: train_step_ref.bound).  The dropout masks and
(optionally) the ReLU gates -- "pool" for relu_pool beside det_step_ref's 6 and 7 -- are inputs."""
import numpy as np

import det_step_ref as D
import skip_ref as S
import train_step_ref as R
from train_step_ref import bound, rel_err  # noqa: F401

KEYS = D.KEYS + ("Wp", "bp")
LR_MULT = dict(D.LR_MULT, Wp=1.0, bp=2.0)
DECAY_MULT = dict(D.DECAY_MULT, Wp=1.0, bp=0.0)

# the sizes of the issue
SMALL = dict(Cs=S.SMALL_CS, hw=S.MAP_HW, Cout=12, n6=260, n7=516, ncls=21)
EDGE = dict(Cs=(68, 132, 60), hw=S.MAP_HW, Cout=132, n6=64, n7=48, ncls=21, N=2, R=130)


def pool_argmax(maps, rois, scales=S.SCALES):
    """ROIPooling 7x7 of every map [N, C, H, W] -> (raw [R*49, sum C] f32, arg [R*49, sum C] int32: h*W + w of the first
    maximum in row-major window order, -1 in an empty bin), rows (roi, bin), the sources side by side."""
    Rn = rois.shape[0]
    raws, args = [], []
    for m, sc in zip(maps, scales):
        p, a = R.roi_pool(np.asarray(m, np.float32), rois, sc)
        C = m.shape[1]
        raws.append(p.reshape(Rn, C, 49).transpose(0, 2, 1))
        args.append(a.reshape(Rn, C, 49).transpose(0, 2, 1))
    return (np.ascontiguousarray(np.concatenate(raws, axis=2).reshape(Rn * 49, -1)),
            np.ascontiguousarray(np.concatenate(args, axis=2).reshape(Rn * 49, -1)))


def offsets(Cs):
    return np.concatenate([[0], np.cumsum(Cs)]).astype(int)


def flatten_caffe(y, Rn):
    """rows (roi, bin) x Cout -> [R, Cout * 49], column c * 49 + p."""
    return np.ascontiguousarray(y.reshape(Rn, 49, -1).transpose(0, 2, 1)).reshape(Rn, -1)


def unflatten_caffe(x, Rn):
    """[R, Cout * 49] -> rows (roi, bin) x Cout."""
    return np.ascontiguousarray(x.reshape(Rn, -1, 49).transpose(0, 2, 1)).reshape(Rn * 49, -1)


def front_forward(front, raw, Cs, dtype=np.float64, gate=None):
    """GRN + scale + conv_pool5 + relu_pool on the raw maxima.  front: Wp [Cout, sum C], bp, gain, eps."""
    dt = dtype
    gain, eps = dt(front.get("gain", 1000.0)), dt(front.get("eps", 1e-10))
    off = offsets(Cs)
    x = np.asarray(raw, dt)
    cat, fac, tot = np.zeros_like(x), np.zeros((x.shape[0], len(Cs)), dt), np.zeros((x.shape[0], len(Cs)), dt)
    for i in range(len(Cs)):
        xi = x[:, off[i]:off[i + 1]]
        t = (xi * xi).sum(axis=1, dtype=dt) + eps
        f = np.where(t > 0, gain / np.sqrt(np.where(t > 0, t, 1)), 0).astype(dt)
        cat[:, off[i]:off[i + 1]] = xi * f[:, None]
        fac[:, i], tot[:, i] = f, t
    Wp = np.asarray(front["Wp"], dt).reshape(np.asarray(front["bp"]).size, -1)
    pre = cat @ Wp.T + np.asarray(front["bp"], dt)
    g = (pre > 0) if gate is None else np.asarray(gate, bool)
    y = np.where(g, pre, 0).astype(dt)
    Rn = x.shape[0] // 49
    return dict(x=x, cat=cat, fac=fac, tot=tot, pre_pool=pre, gate_pool=g, y=y, pool5=flatten_caffe(y, Rn), Wp=Wp)


def front_backward(fw, d_pool5, Cs, arg, rois, shapes, dtype=np.float64, want=None):
    """d_pool5 [R, Cout * 49] -> d_y, g_Wp, g_bp, d_cat, d_raw and the map gradients [N, C, H, W] (want: which sources)."""
    dt = dtype
    Rn = rois.shape[0]
    off = offsets(Cs)
    d_y = np.where(fw["gate_pool"], unflatten_caffe(np.asarray(d_pool5, dt), Rn), 0).astype(dt)
    out = dict(d_y=d_y, g_Wp=d_y.T @ fw["cat"], g_bp=d_y.sum(0))
    d_cat = d_y @ fw["Wp"]
    d_raw = np.zeros_like(d_cat)
    for i in range(len(Cs)):
        sl = slice(off[i], off[i + 1])
        x, dy, f, t = fw["x"][:, sl], d_cat[:, sl], fw["fac"][:, i], fw["tot"][:, i]
        s = (x * dy).sum(axis=1, dtype=dt)
        k = np.where(t > 0, s / np.where(t > 0, t, 1), 0).astype(dt)
        d_raw[:, sl] = f[:, None] * (dy - x * k[:, None])
    out.update(d_cat=d_cat, d_raw=d_raw)
    out["dmaps"] = scatter(d_raw, arg, Cs, rois, shapes, want)
    return out


def scatter(d_raw, arg, Cs, rois, shapes, want=None):
    """Each d_raw to its arg-max cell, roi by roi and bin by bin (the order of the device's gather); [N, C, H, W] per source
    (None where not wanted)."""
    off = offsets(Cs)
    outs = []
    for i, (N, C, H, W) in enumerate(shapes):
        if want is not None and not want[i]:
            outs.append(None)
            continue
        d = np.zeros((N, C, H * W), dtype=d_raw.dtype)
        cc = np.arange(C)
        a, g = arg[:, off[i]:off[i + 1]], d_raw[:, off[i]:off[i + 1]]
        for row in range(arg.shape[0]):
            n = int(rois[row // 49, 0])
            ok = a[row] >= 0
            if ok.any():
                d[n, cc[ok], a[row][ok]] += g[row][ok]
        outs.append(d.reshape(N, C, H, W))
    return outs


def step(params, front, maps, blobs, masks, gates=None, dtype=np.float64, ratios=(0.5, 0.5), scales=S.SCALES, want=None,
         pooled=None):
    """One step of front + head.  params: det_step_ref's eight; front: {Wp, bp, gain, eps}; maps: [N, C_i, H_i, W_i] f32;
    gates: {"pool", 6, 7} or None; pooled: (raw, arg) computed before.  Returns det_step_ref.step's dict plus cat, pool5,
    pre_pool, d_y, d_cat, d_raw, dmaps; grads also holds Wp and bp, sumsq covers all ten."""
    Cs = tuple(int(m.shape[1]) for m in maps)
    raw, arg = pool_argmax(maps, blobs["rois"], scales) if pooled is None else pooled
    fw = front_forward(front, raw, Cs, dtype, None if gates is None else gates["pool"])
    r = D.step(params, fw["pool5"], blobs, masks, gates=gates, dtype=dtype, ratios=ratios, want_dpool=True)
    bw = front_backward(fw, r["d_pool5"], Cs, arg, blobs["rois"], [m.shape for m in maps], dtype, want)
    r.update(raw=raw, skip_argmax=arg, cat=fw["cat"], pre_pool=fw["pre_pool"], pool5=fw["pool5"], d_y=bw["d_y"], d_cat=bw["d_cat"],
             d_raw=bw["d_raw"], dmaps=bw["dmaps"])
    r["grads"]["Wp"], r["grads"]["bp"] = bw["g_Wp"], bw["g_bp"]
    r["sumsq"] = float(sum(np.sum(np.asarray(v, np.float64) ** 2) for v in r["grads"].values()))
    r["gates"]["pool"] = fw["gate_pool"]
    return r


def forward_test(params, front, maps, rois, dtype=np.float64, scales=S.SCALES):
    Cs = tuple(int(m.shape[1]) for m in maps)
    raw, _ = pool_argmax(maps, rois, scales)
    return D.forward_test(params, front_forward(front, raw, Cs, dtype)["pool5"], dtype)


# ---- seeded cases ------------------------------------------------------------------------------------------------------------
def make_front(seed, Cs, Cout, gain=1000.0, eps=1e-10):
    """conv_pool5 at a scale that keeps about half of pool5 alive: rows of `cat` have norm gain * sqrt(n sources)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sumC = int(sum(Cs))
    return {"Wp": (rng.standard_normal((Cout, sumC)) / (gain * np.sqrt(len(Cs)))).astype(np.float32),
            "bp": (0.05 * rng.standard_normal(Cout)).astype(np.float32), "gain": float(gain), "eps": float(eps)}


def make_batch_maps(seed, Cs, N, hw=S.MAP_HW):
    from aznet_hip import synth
    return [np.concatenate([synth.make_feature_map(seed + 17 * i + 101 * n, C, h, w) for n in range(N)], axis=0)
            for i, (C, (h, w)) in enumerate(zip(Cs, hw))]


def make_blobs(seed, Rn, N, ncls, interleave=True):
    """det_step_ref.random_blobs on the 96 x 128 image of skip_ref (6 x 8 cells at 1/16); the image indices interleaved."""
    b = D.random_blobs(seed, Rn, N, S.MAP_HW[2][0], S.MAP_HW[2][1], ncls)
    if interleave and N > 1:
        b["rois"][:, 0] = np.arange(Rn) % N
    return b


def case(name, seed=7):
    """(head, front, maps, blobs) of SMALL (N = 1, the hostile rois + 40 random ones) or EDGE (N = 2, R = 130)."""
    d = SMALL if name == "small" else EDGE
    if name == "small":
        rois = np.vstack([S.hostile_rois(), S.random_rois(40)])
        N = 1
        blobs = make_blobs(seed, rois.shape[0], 1, d["ncls"])
        blobs["rois"] = rois
    else:
        N = d["N"]
        blobs = make_blobs(seed, d["R"], N, d["ncls"])
    head = D.filler_head(seed, d["Cout"], d["n6"], d["n7"], d["ncls"])
    return head, make_front(seed + 2, d["Cs"], d["Cout"]), make_batch_maps(seed, d["Cs"], N, d["hw"]), blobs


def sgd(params, grads, hist, rate, momentum, weight_decay, clip, dtype=np.float64, lr_mult=LR_MULT, decay_mult=DECAY_MULT):
    return R.sgd(params, grads, hist, rate, momentum, weight_decay, clip, dtype=dtype, lr_mult=lr_mult, decay_mult=decay_mult)


# ---- the 20-step run through detect.train_det.SolverWrapper under the skip configuration ---------------------------------------
# det_step_ref.TRAJ's head sizes, seeds and schedule on the same frozen width_div = 32 backbone (Cs = 8, 16, 16); base_lr: found
# on the CPU (tests/test_skip_train_host.py::test_frozen_skip_run_restatement_lowers_the_loss prints the float64 restatement's
# summed loss of the first and the last five steps at this value)
TRAJ = dict(D.TRAJ, solver=dict(D.TRAJ["solver"], base_lr=0.002, snapshot_prefix="frcnn_skip_small"))
traj_backbone = D.traj_backbone


def traj_solver_files(dirname, frozen_all=True):
    import os
    from detect import prototxt as P
    net = os.path.join(dirname, "train_det_skip_%d.prototxt" % int(frozen_all))
    P.write_skip_train_prototxt(net, P.skip_layer_table(frozen=P.CONV_LAYERS if frozen_all else P.CONV_LAYERS[:4]))
    sol = os.path.join(dirname, "solver_det_skip_%d.prototxt" % int(frozen_all))
    P.write_solver_prototxt(sol, net, **TRAJ["solver"])
    return sol


def xavier_front(seed, Cs, Cout, gain=1000.0, eps=1e-10):
    """conv_pool5 as train.prototxt's fillers leave it (uniform in +-sqrt(3 / sum C), bias 0), from NumPy's generator."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = np.sqrt(3.0 / sum(Cs))
    return {"Wp": rng.uniform(-a, a, (Cout, int(sum(Cs)))).astype(np.float32), "bp": np.zeros(Cout, np.float32),
            "gain": float(gain), "eps": float(eps)}


class RefTrajectory(object):
    """The restatement stepping beside a device run of the frozen-backbone skip net: same start (the ten parameters), same
    minibatches, same tapped maps, same masks."""

    def __init__(self, params, front, dtype, solver):
        self.dt = dtype
        self.p = {k: np.asarray(params[k], dtype) for k in D.KEYS}
        self.p["Wp"], self.p["bp"] = np.asarray(front["Wp"], dtype), np.asarray(front["bp"], dtype)
        self.h = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.front = {"gain": front.get("gain", 1000.0), "eps": front.get("eps", 1e-10)}
        self.sp = dict(solver)
        self.it = 0

    def step(self, maps, blobs, seed, gates=None, pooled=None):
        Cs = tuple(int(m.shape[1]) for m in maps)
        raw, arg = pool_argmax(maps, blobs["rois"]) if pooled is None else pooled
        front = dict(self.front, Wp=self.p["Wp"], bp=self.p["bp"])
        fw = front_forward(front, raw, Cs, self.dt, None if gates is None else gates["pool"])
        head = {k: self.p[k] for k in D.KEYS}
        masks = D.step_masks(seed, self.it, fw["pool5"].shape[0], head)
        r = D.step(head, fw["pool5"], blobs, masks, gates=gates, dtype=self.dt, want_dpool=True)
        d_y = np.where(fw["gate_pool"], unflatten_caffe(np.asarray(r["d_pool5"], self.dt), blobs["rois"].shape[0]), 0).astype(self.dt)
        r["grads"]["Wp"], r["grads"]["bp"] = d_y.T @ fw["cat"], d_y.sum(0)
        r["sumsq"] = float(sum(np.sum(np.asarray(v, np.float64) ** 2) for v in r["grads"].values()))
        r["pre_pool"], r["gates"]["pool"] = fw["pre_pool"], fw["gate_pool"]
        rate = R.learning_rate(self.sp["lr_policy"], self.sp["base_lr"], self.it, self.sp["gamma"], self.sp["stepsize"])
        self.p, self.h = sgd(self.p, r["grads"], self.h, rate, self.sp["momentum"], self.sp["weight_decay"],
                             R.clip_scale(r["sumsq"], self.sp["clip_gradients"]), dtype=self.dt)
        self.it += 1
        return r


# ---- the edge steps of tests/test_skip_edges_host.py and tests/test_gpu_skip_edges.py ---------------------------------------------
# Every entry is one step of the trainer at Cout 12, 21 classes.  Defaults: N = 1, the maps of S.MAP_HW at S.SCALES, the fc sizes
# of SMALL, gain 1000, eps 1e-10.  rois: a name of S.source_rois, else skip_ref's random rois on the 96 x 128 image; images: the
# image index of every roi; boxes: the rois themselves; zero: all-zero sources; shrink: the rois scaled to a smaller image.
_SM = dict(Cs=S.SMALL_CS, scales=S.SCALES, hw=S.MAP_HW)
STEP_CASES = {
    "mixed": dict(Cs=(1028, 4, 520), scales=S.SCALES, hw=S.MAP_HW, N=2, R=6, n6=8, n7=8),
    "one": dict(S.SOURCE_CASES["one"], rois="one"),
    "two": dict(S.SOURCE_CASES["two"], rois="two"),
    "odd": dict(S.SOURCE_CASES["odd"], rois="odd"),
    "tiny": dict(S.SOURCE_CASES["tiny"], rois="tiny"),
    "image_without_rois": dict(_SM, N=3, R=9, images=(0, 0, 0, 0, 2, 2, 2, 2, 2)),
    "r1": dict(_SM, N=2, R=1, images=(1,), boxes=((20.0, 12.0, 100.0, 80.0),)),
    "rmax": dict(_SM, N=2, R=20),
    "shrunk": dict(_SM, hw=((12, 10), (6, 5), (3, 3)), N=2, R=3, shrink=0.3),
    "gain0": dict(_SM, N=2, R=8, gain=0.0),
    "gain_negative": dict(_SM, N=2, R=8, gain=-2.5),
    "eps0_zero_source": dict(_SM, N=2, R=8, eps=0.0, zero=(1,)),
    "gain1_eps1": dict(_SM, N=2, R=8, gain=1.0, eps=1.0),
}
# the seeds tried, in order, for a step none of whose float64 pre-activations (pre_pool, pre6, pre7) lies within twice the
# forward bound of zero -- the device's ReLU gates are then float64's, exactly -- and the first that meets it, per case, as
# tests/test_skip_edges_host.py finds it
SEED_TRIALS = (7, 8, 9, 10, 11, 12, 13, 14)
STEP_SEEDS = {name: 7 for name in STEP_CASES}


def edge_step(name, seed):
    """(head, front, maps, blobs, scales) of STEP_CASES[name]: the weights, labels, targets and random rois from `seed`, the
    maps from the case alone."""
    d = STEP_CASES[name]
    Cs, N, ncls = d["Cs"], d.get("N", 1), 21
    maps = S.edge_maps("relu", 7, Cs, d["hw"], N)
    for i in d.get("zero", ()):
        maps[i][:] = 0.0
    rois = S.source_rois(d["rois"]) if "rois" in d else None
    Rn = d["R"] if rois is None else rois.shape[0]
    blobs = make_blobs(seed, Rn, N, ncls)
    if rois is not None:
        blobs["rois"] = rois
    else:
        blobs["rois"][:, 1:] = S.random_rois(Rn, seed=seed)[:, 1:] * np.float32(d.get("shrink", 1.0))
    if "boxes" in d:
        blobs["rois"][:, 1:] = np.asarray(d["boxes"], np.float32)
    if "images" in d:
        blobs["rois"][:, 0] = d["images"]
    head = D.filler_head(seed, 12, d.get("n6", SMALL["n6"]), d.get("n7", SMALL["n7"]), ncls)
    gain = d.get("gain", 1000.0)
    front = make_front(seed + 2, Cs, 12, gain=abs(gain) if gain else 1000.0, eps=d.get("eps", 1e-10))
    front["gain"] = float(gain)
    return head, front, maps, blobs, tuple(d["scales"])


def gate_margins(r64, r32):
    """[(name, smallest |pre-activation_64|, twice the forward bound in its units)] of relu_pool, fc6 and fc7."""
    out = []
    for key in ("pre_pool", "pre6", "pre7"):
        pre = np.asarray(r64[key], np.float64)
        out.append((key, float(np.abs(pre).min()), 2.0 * bound(rel_err(r32[key], pre)) * float(np.abs(pre).max())))
    return out


_EDGE_REFS = {}


def edge_reference(name, seed):
    """The step at `seed` (dropout seed `seed`, iteration 0) in float64 with its own gates and in float32 under those gates,
    computed once: dict(head, front, maps, blobs, scales, masks, pooled, r64, r32, margins).  Nothing in it may be changed."""
    if (name, seed) not in _EDGE_REFS:
        head, front, maps, blobs, scales = edge_step(name, seed)
        pooled = pool_argmax(maps, blobs["rois"], scales)
        masks = D.step_masks(seed, 0, blobs["rois"].shape[0], head)
        r64 = step(head, front, maps, blobs, masks, scales=scales, pooled=pooled)
        r32 = step(head, front, maps, blobs, masks, gates=r64["gates"], dtype=np.float32, scales=scales, pooled=pooled)
        _EDGE_REFS[(name, seed)] = dict(head=head, front=front, maps=maps, blobs=blobs, scales=scales, masks=masks, pooled=pooled,
                                        r64=r64, r32=r32, margins=gate_margins(r64, r32))
    return _EDGE_REFS[(name, seed)]


def find_seed(name):
    """The first of SEED_TRIALS whose step keeps every pre-activation outside twice the forward bound of zero (None: none)."""
    for seed in SEED_TRIALS:
        if all(lo > two_fwd for _, lo, two_fwd in edge_reference(name, seed)["margins"]):
            return seed
    return None


_CHANNEL_REFS = {}


def channel_reference(Cs, kind):
    """A CHANNEL_SETS entry on "relu" maps (eps 1e-10) or "ties" maps (eps 0; every sum of squares a whole number), N = 1, the
    rois of S.channel_rois: dict(maps, scales, rois, front, raw, arg, f64, cat32) with f64 = front_forward in float64 and
    cat32 its float32 `cat`.  Computed once; nothing in it may be changed."""
    if (Cs, kind) not in _CHANNEL_REFS:
        scales, hw = S.geometry(Cs)
        maps, rois = S.edge_maps(kind, 11, Cs, hw), S.channel_rois()
        front = make_front(4, Cs, 12, eps=0.0 if kind == "ties" else 1e-10)
        raw, arg = pool_argmax(maps, rois, scales)
        _CHANNEL_REFS[(Cs, kind)] = dict(maps=maps, scales=scales, rois=rois, front=front, raw=raw, arg=arg,
                                         f64=front_forward(front, raw, Cs), cat32=front_forward(front, raw, Cs, np.float32)["cat"])
    return _CHANNEL_REFS[(Cs, kind)]


_GATHER_REFS = {}


def gather_reference(tag):
    """Inputs and exact answers of the gather on whole-number gradients in [-8, 8] (every sum exact in any order):
    "sweep_ties" / "sweep_perm": S.sweep_rois on one 9 x 11 map of 4 channels at scale 1.0, tie-heavy or all-distinct;
    "all_in_last" / "descending": the maps and rois of STEP_CASES["image_without_rois"] with every roi in image 2, or the
    rois in descending image order.  dict(maps, scales, rois, raw, arg, d_raw, want); computed once, not to be changed."""
    if tag not in _GATHER_REFS:
        if tag.startswith("sweep"):
            w = S.SWEEP
            maps, scales = S.edge_maps(tag[6:], 5, (w["C"],), ((w["H"], w["W"]),)), (1.0,)
            rois = S.sweep_rois()[0]
        else:
            _, _, maps, blobs, scales = edge_step("image_without_rois", 7)
            rois = blobs["rois"].copy()
            rois[:, 0] = 2 if tag == "all_in_last" else (2, 2, 2, 1, 1, 1, 0, 0, 0)
        Cs = tuple(int(m.shape[1]) for m in maps)
        raw, arg = pool_argmax(maps, rois, scales)
        d_raw = np.random.Generator(np.random.PCG64(8)).integers(-8, 9, raw.shape).astype(np.float32)
        _GATHER_REFS[tag] = dict(maps=maps, scales=scales, rois=rois, raw=raw, arg=arg, d_raw=d_raw,
                                 want=scatter(d_raw, arg, Cs, rois, [m.shape for m in maps]))
    return _GATHER_REFS[tag]
