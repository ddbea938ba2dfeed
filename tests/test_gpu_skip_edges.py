"""GPU: the skip-connection front (csrc/az_skip.hip) and its trainer (csrc/az_skip_train.hip) off the one configuration of
tests/test_gpu_skip.py and tests/test_gpu_skip_train.py -- three sources at 1/4, 1/8, 1/16 on maps of image * scale, 12 to 512
channels, every image with rois, gain 1000, eps 1e-10.  tests/test_skip_edges_host.py asserts the inputs' conditions on the
references alone.

  1. the channel-quad partition of both pool kernels (nqb = min(256, quads left), G = 256 / nqb): 1, 130, 256, 257, 300 and
     1024 quads and (257, 1, 130) side by side, on post-ReLU-like and on tie-heavy maps; one whole step at (1028, 4, 520)
  2. one and two sources, scales that are no power of two, maps that are not image * scale: the inference head and one step
  3. the trainer's batch and state edges: an image without rois, all rois in the last image, R = 1, R = max_rois, stale rows
  4. gain 0, gain < 0, eps 0 with an all-zero source, eps 1: one step each, and the inference front
  5. the profiled launch form (one launch per source) of both fronts: the bits of the unprofiled calls, the launch names
  6. a device row count far below the host bound: a trailing chunk without rows
  7. the gather over a sweep of window sizes, bit for bit
  8. conv_pool5's GEMM (k_skip_conv) against the trainer's form-0 GEMM (k_solver_gemm), whose tile it shares: bit for bit
References: train_step_ref.roi_pool, skip_train_ref.pool_argmax / scatter / front_forward / step, skip_ref.det_forward.
Tolerance: train_step_ref.bound (8 x the float32 restatement's error against float64, floor 1e-6); what is exact is compared
bit for bit.  The steps' seeds (skip_train_ref.STEP_SEEDS) keep every float64 pre-activation outside twice the forward bound
of zero, so the device's ReLU gates must be float64's, all of them.  Every figure is printed before it is asserted."""
import contextlib

import numpy as np
import pytest

import det_step_ref as D
import skip_ref as S
import skip_train_ref as T

pytestmark = pytest.mark.gpu
TEN = T.KEYS
IDS = lambda Cs: "x".join(map(str, Cs))
WORST = {}         # the largest device error / bound: per section over the tests run so far, and "test": of the test running


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check(section, name, got, r64, r32):
    e_dev, e_cpu = T.rel_err(got, r64), T.rel_err(r32, r64)
    b = T.bound(e_cpu)
    WORST[section], WORST["test"] = max(WORST.get(section, 0.0), e_dev / b), max(WORST.get("test", 0.0), e_dev / b)
    print("  %-22s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (name, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b


@pytest.fixture(autouse=True)
def own_share():
    """Every test prints its own worst share of the bound (what one test run alone gives); a section's figure in DESIGN.md is
    the largest of its tests'."""
    WORST["test"] = 0.0
    yield
    print("  this test: worst share of the bound %.3f" % WORST["test"])


def share(section):
    print("  section %s: worst share of the bound so far %.3f" % (section, WORST.get(section, 0.0)))


def to_dev(maps, channels_last=False):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in maps]
    return [t.contiguous(memory_format=torch.channels_last) for t in out] if channels_last else out


def make_trainer(ctx, head, front, Cs, scales, max_rois=32, seed=1):
    from aznet_hip import ffi
    n6, n7, ncls = head["W6"].shape[0], head["W7"].shape[0], head["Wc"].shape[0]
    sol = ffi.AzDetSolver(ctx, head["W6"].shape[1] // 49, n6, n7, ncls, max_rois=max_rois, seed=seed, head=head)
    sol.attach_skip(Cs, scales, gain=front["gain"], eps=front["eps"], seed=seed, front=front)
    return sol


@contextlib.contextmanager
def inference_context(head, front, maps=None, max_regions=64):
    """A context with a tiny AZ head (a context takes maps once it has one), the detection head and the front."""
    from aznet_hip import ffi, synth
    c = ffi.AzContext(0, max_regions=max_regions)
    try:
        c.load_head(synth.make_head(seed=3, C=head["W6"].shape[1] // 49, n6=4, n71=4, n72=4))
        c.load_det_head(head)
        c.load_skip_front(front)
        if maps is not None:
            c.set_skip_maps(to_dev(maps))
        yield c
    finally:
        c.close()


def skip_args(maps, blobs):
    return (maps, blobs["rois"], blobs["labels"], blobs["bbox_targets"], blobs["bbox_loss_weights"])


def kernel_cat(raw, fac, Cs):
    """The kernel's own statement of its rounding: float32(float64(raw) * factor[row, source])."""
    off = T.offsets(Cs)
    return np.concatenate([(raw[:, off[i]:off[i + 1]].astype(np.float64) * fac[:, i:i + 1]).astype(np.float32) for i in range(len(Cs))], axis=1)


# ---- one step against the restatement ---------------------------------------------------------------------------------------------
def run_step(ctx, name, channels_last, max_rois=32):
    """One step_skip of STEP_CASES[name] at its recorded seed with every d map prefilled with 7.0:
    (trainer, reference, d maps as NumPy, losses, sumsq)."""
    import torch
    seed = T.STEP_SEEDS[name]
    r = T.edge_reference(name, seed)
    Cs = T.STEP_CASES[name]["Cs"]
    print("%s: Cs %s, scales %s, maps %s, N %d, R %d, gain %g, eps %g, %s" % (
        name, Cs, r["scales"], [m.shape[2:] for m in r["maps"]], r["maps"][0].shape[0], r["blobs"]["rois"].shape[0], r["front"]["gain"],
        r["front"]["eps"], "channels_last" if channels_last else "NCHW"))
    sol = make_trainer(ctx, r["head"], r["front"], Cs, r["scales"], max_rois=max_rois)
    dev = to_dev(r["maps"], channels_last)
    dmaps = [torch.full_like(m, 7.0) for m in dev]
    losses, sumsq = sol.step_skip(*skip_args(dev, r["blobs"]), seed, 0, dmaps=dmaps)
    return sol, r, [d.cpu().numpy() for d in dmaps], losses, sumsq


def check_step(section, sol, r, dmaps, losses, sumsq):
    """Every tensor tests/test_gpu_skip_train.py::test_one_step checks -- the clipped update, the unclipped one on top of its
    history and read_skip included -- after the arg-max, the masks and the gates (exactly)."""
    r64, r32, Rn, Cs = r["r64"], r["r32"], r["blobs"]["rois"].shape[0], tuple(m.shape[1] for m in r["maps"])
    assert same_bits(sol.fetch("skip_argmax"), r["pooled"][1]), "skip_argmax"
    for t, _, _ in D.LAYERS:
        assert np.array_equal(sol.fetch("mask%d" % t), r["masks"][t]), "mask of layer %d" % t
    gates = {t: sol.fetch("pre%d" % t) > 0 for t, _, _ in D.LAYERS}
    gates["pool"] = T.unflatten_caffe(sol.fetch("pool5"), Rn) > 0
    for key, lo, two_fwd in r["margins"]:
        print("  %s: smallest |float64| %.3e, twice the forward bound %.3e" % (key, lo, two_fwd))
        assert lo > two_fwd
    for t in ("pool", 6, 7):
        diff = int((gates[t] != r64["gates"][t]).sum())
        print("  gates of %s: %d of %d differ from float64" % (t, diff, gates[t].size))
        assert diff == 0
    ok = True
    for nm in ("cat", "pool5", "pre6", "a6", "pre7", "a7", "cls_score", "cls_prob", "bbox_pred", "d_cls_score", "d_bbox_pred", "d_pre7",
               "d_pre6", "d_pool5", "d_y", "d_cat", "d_raw"):
        ok &= check(section, nm, sol.fetch(nm).reshape(np.shape(r64[nm])), r64[nm], r32[nm])
    fac = sol.fetch("skip_factor")
    assert fac.dtype == np.float64 and fac.shape == (Rn * 49, len(Cs))
    assert same_bits(sol.fetch("cat"), kernel_cat(r["pooled"][0], fac, Cs)), "cat is not float32(float64(raw) * skip_factor)"
    for i in range(len(Cs)):
        ok &= check(section, "d map %d" % i, dmaps[i], r64["dmaps"][i], r32["dmaps"][i])
    ok &= check(section, "losses", losses, r64["losses"], r32["losses"])
    fetched = {k: sol.fetch("g_" + k) for k in TEN}
    for k in TEN:
        ok &= check(section, "g_" + k, fetched[k], r64["grads"][k], r32["grads"][k])
    total = float(sum(np.sum(v.astype(np.float64) ** 2) for v in fetched.values()))
    print("  sumsq %.17g, f64 sum over the ten fetched gradients %.17g" % (sumsq, total))
    assert abs(sumsq - total) <= 1e-12 * total
    rate, mom, wd = 0.001, 0.9, 0.0005
    start = dict(r["head"], Wp=r["front"]["Wp"], bp=r["front"]["bp"])
    zeros = {k: np.zeros_like(v) for k, v in start.items()}
    for rep, clip_at in ((0, 1e-3), (1, None)):                       # a clipped step, then an unclipped one on top of its history
        cs = D.clip_scale(sumsq, clip_at)
        if rep == 0:
            assert cs < 1.0
            p64, h64 = T.sgd(start, r64["grads"], zeros, rate, mom, wd, D.clip_scale(r64["sumsq"], clip_at))
            p32, h32 = T.sgd(start, r32["grads"], zeros, rate, mom, wd, D.clip_scale(r32["sumsq"], clip_at), dtype=np.float32)
        else:
            p64, h64 = T.sgd(p64, r64["grads"], h64, rate, mom, wd, 1.0)
            p32, h32 = T.sgd(p32, r32["grads"], h32, rate, mom, wd, 1.0, dtype=np.float32)
        sol.update(rate, mom, wd, cs)
        for k in TEN:
            ok &= check(section, "w_%s/%d" % (k, rep), sol.fetch("w_" + k), p64[k], p32[k])
            ok &= check(section, "h_%s/%d" % (k, rep), sol.fetch("h_" + k), h64[k], h32[k])
    got = sol.read_skip()
    assert np.array_equal(got["Wp"], sol.fetch("w_Wp")) and np.array_equal(got["bp"], sol.fetch("w_bp"))
    finite = all(np.isfinite(a).all() for a in list(fetched.values()) + list(dmaps) + [sol.fetch(n) for n in ("cat", "pool5", "d_cat", "d_raw")])
    share(section)
    assert finite, "a non-finite value"
    return ok


# ---- 1. the channel partition of both pool kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["relu", "ties"])
@pytest.mark.parametrize("Cs", S.CHANNEL_SETS, ids=IDS)
def test_channel_partition(ctx, Cs, kind):
    from aznet_hip import ffi, synth
    c = T.channel_reference(Cs, kind)
    maps, rois, scales, front, raw, arg = c["maps"], c["rois"], c["scales"], c["front"], c["raw"], c["arg"]
    head = D.filler_head(5, 12, 8, 8, 21)
    print("%s %s: quads %s, eps %g" % (Cs, kind, [C // 4 for C in Cs], front["eps"]))
    with inference_context(synth.make_det_head(seed=9, C=12, n6=4, n7=4, ncls=2), dict(front, Cs=Cs, scales=scales), maps) as ictx:
        raw_inf = ictx.skip_pool(rois, normalise=False)
        cat_inf = ictx.skip_pool(rois, normalise=True)
    assert same_bits(raw_inf, raw), "az_skip_pool(normalise = 0)"
    sol = make_trainer(ctx, head, front, Cs, scales, max_rois=32)
    ok, worst_ulp = True, 0.0
    for cl in (False, True):
        tag = "nhwc" if cl else "nchw"
        sol.forward_test_skip(to_dev(maps, cl), rois)
        got_arg, got_cat, fac = sol.fetch("skip_argmax"), sol.fetch("cat"), sol.fetch("skip_factor")
        print("  %s: %d of %d arg-max cells differ; %d empty" % (tag, int((got_arg != arg).sum()), arg.size, int((arg == -1).sum())))
        assert got_arg.dtype == np.int32 and same_bits(got_arg, arg)
        assert same_bits(got_cat, cat_inf), "cat differs from az_skip_pool's bits"
        assert fac.dtype == np.float64 and fac.shape == (rois.shape[0] * 49, len(Cs))
        assert same_bits(got_cat, kernel_cat(raw, fac, Cs)), "cat is not float32(float64(raw) * skip_factor)"
        ok &= check("1", "cat %s" % tag, got_cat, c["f64"]["cat"], c["cat32"])
        if kind == "ties":
            ref = c["f64"]["fac"]
            assert not fac[ref == 0].any()
            ulp = float((np.abs(fac - ref)[ref != 0] / np.spacing(np.abs(ref[ref != 0]))).max())
            worst_ulp = max(worst_ulp, ulp)
            print("  %s: skip_factor against float64 gain / sqrt(tot): %.2f ulp at worst" % (tag, ulp))
        pooled, uarg, _ = ffi.skip_pool_bwd_unit(ctx, maps, scales, rois, channels_last=cl)
        assert same_bits(pooled, raw) and same_bits(uarg, arg), "az_skip_pool_bwd_unit"
    sol.close()
    share("1")
    assert ok, "cat exceeds 8 x the float32 restatement's error"
    assert worst_ulp <= 2.0


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_whole_step_at_mixed_channel_regimes(ctx, channels_last):
    sol, r, dmaps, losses, sumsq = run_step(ctx, "mixed", channels_last)
    ok = check_step("1", sol, r, dmaps, losses, sumsq)
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


# ---- 2. one and two sources, other scales, other map shapes -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.SOURCE_CASES))
def test_sources_inference_head(name):
    import torch
    from oracle import az_oracle as orc
    c = S.source_case(name)
    front, head, maps, rois, boxes = c["front"], c["head"], c["maps"], c["rois"], c["boxes"]
    names = S.NAMES[3 - len(c["Cs"]):]
    r64, r32 = S.det_forward(front, head, maps, rois, np.float64), S.det_forward(front, head, maps, rois, np.float32)
    s64, b64 = S.detect(orc, front, head, maps, boxes, 1.0, (S.IM_H, S.IM_W), 1. / 16., np.float64, names=names)
    s32, b32 = S.detect(orc, front, head, maps, boxes, 1.0, (S.IM_H, S.IM_W), 1. / 16., np.float32, names=names)
    ok, outs = True, []
    with inference_context(head, front) as ictx:
        for cl in (False, True):
            tag = "%s %s" % (name, "nhwc" if cl else "nchw")
            ictx.set_skip_maps(to_dev(maps, cl))
            p, b = ictx.det_forward_skip(rois)
            ok &= check("2", "%s cls_prob" % tag, p, r64[0], r32[0]) & check("2", "%s bbox_pred" % tag, b, r64[1], r32[1])
            p5 = ictx.skip_conv(ictx.skip_pool(rois, normalise=True)).reshape(rois.shape[0], 49, -1).transpose(0, 2, 1).reshape(rois.shape[0], -1)
            ok &= check("2", "%s pool5" % tag, p5, S.pool5(front, maps, rois, np.float64), S.pool5(front, maps, rois, np.float32))
            assert same_bits(ictx.skip_pool(rois, normalise=False), S.cat_raw(maps, rois, c["scales"]))
            s, bx = ictx.detect_skip(boxes, 1.0, S.IM_H, S.IM_W)
            assert s.shape == s64.shape and bx.shape == b64.shape
            ok &= check("2", "%s detect scores" % tag, s, s64, s32)
            ok &= check("2", "%s detect boxes" % tag, bx, b64, b32)
            np.testing.assert_allclose(bx, b64, rtol=1e-4, atol=1e-4 * S.IM_W)
            assert np.array_equal(s[-3:], s[:3])
            outs.append((p, b, s, bx))
    assert all(same_bits(x, y) for x, y in zip(*outs)), "the memory format of the maps handed over shows in the result"
    share("2")
    assert ok, "a tensor exceeds 8 x the float32 restatement's error"


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", sorted(S.SOURCE_CASES))
def test_sources_one_step(ctx, name, channels_last):
    sol, r, dmaps, losses, sumsq = run_step(ctx, name, channels_last)
    assert sol.fetch("skip_factor").shape == (r["blobs"]["rois"].shape[0] * 49, len(S.SOURCE_CASES[name]["Cs"]))
    ok = check_step("2", sol, r, dmaps, losses, sumsq)
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


# ---- 3. batch and state edges of the trainer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_an_image_without_rois(ctx, channels_last):
    sol, r, dmaps, losses, sumsq = run_step(ctx, "image_without_rois", channels_last)
    for i, d in enumerate(dmaps):
        print("  d map %d: image 1 has %d non-zero cells, images 0 and 2 %d" % (i, int((d[1] != 0).sum()), int((d[0] != 0).sum() + (d[2] != 0).sum())))
        assert d.shape[0] == 3 and not d[1].any() and d[0].any() and d[2].any()
    ok = check_step("3", sol, r, dmaps, losses, sumsq)
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


@pytest.mark.parametrize("tag", ["all_in_last", "descending"])
def test_rois_in_the_last_image_and_in_descending_order(ctx, tag):
    from aznet_hip import ffi
    g = T.gather_reference(tag)
    for cl in (False, True):
        pooled, uarg, dm = ffi.skip_pool_bwd_unit(ctx, g["maps"], g["scales"], g["rois"], d_raw=g["d_raw"], channels_last=cl)
        assert same_bits(pooled, g["raw"]) and same_bits(uarg, g["arg"])
        for i, w in enumerate(g["want"]):
            print("  %s %s map %d: |d| max %.0f, %d cells hit" % (tag, "nhwc" if cl else "nchw", i, np.abs(w).max(), int((w != 0).sum())))
            assert same_bits(dm[i], w)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["r1", "rmax"])
def test_one_roi_and_max_rois(ctx, name, channels_last):
    sol, r, dmaps, losses, sumsq = run_step(ctx, name, channels_last, max_rois=20)
    assert r["blobs"]["rois"].shape[0] == (1 if name == "r1" else sol.max_rois)
    ok = check_step("3", sol, r, dmaps, losses, sumsq)
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


STATE = ["cat", "skip_argmax", "skip_factor", "pool5", "cls_prob", "d_y", "d_cat", "d_raw"] + ["g_" + k for k in TEN]


def test_stale_rows_do_not_show(ctx):
    """One trainer: a step at R = 20 on 24x32 / 12x16 / 6x8, a step at R = 3 on 12x10 / 6x5 / 3x3 (cat, arg and geo keep the
    first step's rows past the 147 in use), one forward_test_skip -- each with the bits of the same call on a fresh trainer
    from the same weights (no update in between)."""
    import torch
    big, small = T.edge_step("rmax", 7), T.edge_step("shrunk", 7)
    head, front, Cs = big[0], big[1], T.STEP_CASES["rmax"]["Cs"]
    assert all(same_bits(big[0][k], small[0][k]) for k in D.KEYS) and same_bits(big[1]["Wp"], small[1]["Wp"])
    test_rois = np.vstack([S.hostile_rois()[[2, 5, 7]], S.random_rois(2, 9)])
    test_rois[:, 0] = (1, 0, 1, 0, 1)

    def step(sol, case):
        dev = to_dev(case[2], True)
        dmaps = [torch.full_like(m, 7.0) for m in dev]
        losses, sq = sol.step_skip(*skip_args(dev, case[3]), 7, 0, dmaps=dmaps)
        return [losses, np.float64(sq)] + [d.cpu().numpy() for d in dmaps] + [sol.fetch(n) for n in STATE]

    def test(sol):
        p, b = sol.forward_test_skip(to_dev(big[2], True), test_rois)
        return [p, b] + [sol.fetch(n) for n in ("cat", "skip_argmax", "skip_factor", "pool5")]

    used = make_trainer(ctx, head, front, Cs, S.SCALES, max_rois=20)
    got = [step(used, big), step(used, small), test(used)]
    used.close()
    want = []
    for call, case in ((step, big), (step, small), (test, None)):
        fresh = make_trainer(ctx, head, front, Cs, S.SCALES, max_rois=20)
        want.append(call(fresh, case) if case is not None else call(fresh))
        fresh.close()
    assert got[0][5].shape == (20 * 49, sum(Cs)) and got[1][5].shape == (3 * 49, sum(Cs)) and got[2][2].shape == (5 * 49, sum(Cs))
    for k, (a, b) in enumerate(zip(got, want)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert same_bits(np.atleast_1d(x), np.atleast_1d(y)), "call %d, output %d" % (k, j)
    assert not same_bits(got[0][0], got[1][0])                          # (the two steps do differ)


# ---- 4. gain and eps --------------------------------------------------------------------------------------------------------------------------
GAIN_EPS = ["gain0", "gain_negative", "eps0_zero_source", "gain1_eps1"]


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", GAIN_EPS)
def test_gain_and_eps_one_step(ctx, name, channels_last):
    sol, r, dmaps, losses, sumsq = run_step(ctx, name, channels_last)
    Rn = r["blobs"]["rois"].shape[0]
    if name == "gain0":
        bp = np.maximum(r["front"]["bp"], 0).astype(np.float32)
        assert not sol.fetch("cat").any(), "cat"
        assert same_bits(sol.fetch("pool5"), T.flatten_caffe(np.tile(bp, (Rn * 49, 1)), Rn)), "pool5 is not relu(bp)"
        assert not sol.fetch("g_Wp").any() and not any(d.any() for d in dmaps), "g_Wp and the d maps are exactly zero"
    if name == "eps0_zero_source":
        assert not dmaps[1].any(), "the all-zero source's d map"
        assert dmaps[0].any() and dmaps[2].any()
    ok = check_step("4", sol, r, dmaps, losses, sumsq)
    sol.close()
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


@pytest.mark.parametrize("name", GAIN_EPS)
def test_gain_and_eps_inference_front(name):
    from aznet_hip import synth
    r = T.edge_reference(name, T.STEP_SEEDS[name])
    Cs, front = T.STEP_CASES[name]["Cs"], r["front"]
    maps = [m[:1] for m in r["maps"]]
    rois = np.vstack([S.hostile_rois(), r["blobs"]["rois"]])
    rois[:, 0] = 0
    raw, _ = T.pool_argmax(maps, rois)
    c64, c32 = T.front_forward(front, raw, Cs)["cat"], T.front_forward(front, raw, Cs, np.float32)["cat"]
    with inference_context(synth.make_det_head(seed=9, C=12, n6=4, n7=4, ncls=2), dict(front, Cs=Cs, scales=S.SCALES), maps) as ictx:
        got = ictx.skip_pool(rois, normalise=True)
    assert np.isfinite(got).all() and np.isfinite(c32).all()
    ok = check("4", "concat5 %s" % name, got, c64, c32)
    if name == "gain0":
        assert not got.any()
    if name == "eps0_zero_source":
        assert not got[:, Cs[0]:Cs[0] + Cs[1]].any() and got[:, :Cs[0]].any()
    share("4")
    assert ok, "concat5 exceeds 8 x the float32 restatement's error"


# ---- 5. the profiled launch form ------------------------------------------------------------------------------------------------------------
def launch_names(c):
    return [n for n, _, _ in c.last_kernel_times()]


PROFILED = {"small": dict(Cs=S.SMALL_CS, scales=S.SCALES, hw=S.MAP_HW), "two": S.SOURCE_CASES["two"]}


@pytest.mark.parametrize("which", sorted(PROFILED))
def test_profiled_launch_form_of_the_inference_front(which):
    from aznet_hip import synth
    d = PROFILED[which]
    n = len(d["Cs"])
    maps = S.edge_maps("relu", 14, d["Cs"], d["hw"])
    rois, boxes = np.vstack([S.hostile_rois(), S.random_rois(10, 8)]), S.random_boxes(30, 5)
    front = synth.make_skip_front(seed=1, Cs=d["Cs"], Cout=12, scales=d["scales"])
    calls = (lambda c: (c.skip_pool(rois, normalise=True),), lambda c: c.det_forward_skip(rois),
             lambda c: c.detect_skip(boxes, 1.0, S.IM_H, S.IM_W))
    with inference_context(synth.make_det_head(seed=9, C=12, n6=260, n7=516, ncls=21), front, maps) as ictx:
        plain = [call(ictx) for call in calls]
        ictx.set_profiling(2)
        try:
            prof, names = [], []
            for call in calls:
                prof.append(call(ictx))
                names.append(launch_names(ictx))
        finally:
            ictx.set_profiling(0)
        after = [call(ictx) for call in calls]
    for k, (a, b, z) in enumerate(zip(plain, prof, after)):
        assert all(same_bits(x, y) for x, y in zip(a, b)) and all(same_bits(x, y) for x, y in zip(a, z)), "call %d under set_profiling(2)" % k
    for k in (1, 2):
        print("  %s call %d: %s" % (which, k, names[k]))
        pools = [x for x in names[k] if x.startswith("skip_pool_norm")]
        assert pools == ["skip_pool_norm_%d" % i for i in range(n)] and names[k].count("skip_conv_gemm") == 1
        assert names[k].index("skip_conv_gemm") > names[k].index(pools[-1])
    assert set(x for x in names[0] if x.startswith("skip_pool_norm")) == set("skip_pool_norm_%d" % i for i in range(n))


@pytest.mark.parametrize("which", ["rmax", "two"])
def test_profiled_step(ctx, which):
    import torch
    head, front, maps, blobs, scales = T.edge_step(which, 7)
    Cs = T.STEP_CASES[which]["Cs"]
    n = len(Cs)
    dev = to_dev(maps)

    def run():
        sol = make_trainer(ctx, head, front, Cs, scales)
        dmaps = [torch.full_like(m, 7.0) for m in dev]
        losses, sq = sol.step_skip(*skip_args(dev, blobs), 7, 0, dmaps=dmaps)
        names = launch_names(ctx)
        out = [losses, np.float64(sq)] + [d.cpu().numpy() for d in dmaps] + [sol.fetch(k) for k in STATE]
        sol.close()
        return out, names

    plain, _ = run()
    ctx.set_profiling(2)
    try:
        prof, names = run()
    finally:
        ctx.set_profiling(0)
    print("  %s: %s" % (which, names))
    for j, (x, y) in enumerate(zip(plain, prof)):
        assert same_bits(np.atleast_1d(x), np.atleast_1d(y)), "output %d under set_profiling(2)" % j
    want = ["skip_pool_argmax", "conv_pool5_fwd", "conv_pool5_finish", "relu_pool_bwd", "conv_pool5_dw", "conv_pool5_dx", "skip_grn_bwd"]
    want += ["skip_pool_bwd_%d" % i for i in range(n)]
    assert all(names.count(w) == 1 for w in want), [w for w in want if names.count(w) != 1]
    assert [x for x in names if x.startswith("skip_pool_bwd")] == want[-n:]
    assert [names.index(w) for w in want] == sorted(names.index(w) for w in want)


# ---- 6. a device row count far below the host bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_regions,P", [(300, 259), (64, 64)])
def test_device_row_count_far_below_the_host_bound(max_regions, P):
    """az_detect_skip hands the front the host bound P while the dedup leaves 5 rows on the device: with a chunk of 128 and
    P = 259 the two trailing chunks have no row.  `cat` and pool5 hold P distinct rows from the call before.  Again with the
    chunk equal to the context's capacity, at the smallest capacity a context takes: 64 regions (az_set_limits refuses
    fewer, 40 for one)."""
    from aznet_hip import ffi, synth
    from oracle import az_oracle as orc
    Cs = S.SMALL_CS
    maps = S.make_maps(16, Cs)
    head, front = synth.make_det_head(seed=9, C=12, n6=260, n7=516, ncls=21), synth.make_skip_front(seed=1, Cs=Cs, Cout=12)
    assert min(max_regions, ffi.AZ_SKIP_CHUNK) == (128 if max_regions == 300 else max_regions) and P <= max_regions
    if max_regions == 64:
        with pytest.raises(ffi.AzError) as e:
            ffi.AzContext(0, max_regions=40)
        assert e.value.code == ffi.AZ_ERR_INVALID
    fill, five = S.random_boxes(P, 22), S.random_boxes(5, 23)
    tiled = five[np.arange(P) % 5]
    with inference_context(head, front, maps, max_regions=max_regions) as ictx:
        assert len(ictx.roi_dedup(fill, 1.0, dedup=0.0)[1]) == P and len(ictx.roi_dedup(tiled, 1.0)[1]) == 5
        ictx.detect_skip(fill, 1.0, S.IM_H, S.IM_W, dedup=0.0)
        s, bx = ictx.detect_skip(tiled, 1.0, S.IM_H, S.IM_W)
        s5, bx5 = ictx.detect_skip(five, 1.0, S.IM_H, S.IM_W)
        assert same_bits(s, s5[np.arange(P) % 5]) and same_bits(bx, bx5[np.arange(P) % 5]), "the rows of 5 boxes, tiled"
        s64, b64 = S.detect(orc, front, head, maps, five, 1.0, (S.IM_H, S.IM_W), 1. / 16., np.float64)
        s32, b32 = S.detect(orc, front, head, maps, five, 1.0, (S.IM_H, S.IM_W), 1. / 16., np.float32)
        ok = check("6", "scores, %d regions" % max_regions, s, s64[np.arange(P) % 5], s32[np.arange(P) % 5])
        ok &= check("6", "boxes, %d regions" % max_regions, bx, b64[np.arange(P) % 5], b32[np.arange(P) % 5])
        np.testing.assert_allclose(bx, b64[np.arange(P) % 5], rtol=1e-4, atol=1e-4 * S.IM_W)
        if P == max_regions:                                           # every region of the context through az_det_forward_skip
            rois = S.random_rois(P, 30)
            p, b = ictx.det_forward_skip(rois)
            r64, r32 = S.det_forward(front, head, maps, rois, np.float64), S.det_forward(front, head, maps, rois, np.float32)
            ok &= check("6", "cls_prob, %d of %d" % (P, P), p, r64[0], r32[0]) & check("6", "bbox_pred, %d of %d" % (P, P), b, r64[1], r32[1])
    share("6")
    assert ok, "a tensor exceeds 8 x the float32 restatement's error"


# ---- 7. the gather over a sweep of window sizes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ties", "perm"])
def test_gather_over_a_sweep_of_window_sizes(ctx, kind):
    from aznet_hip import ffi
    g = T.gather_reference("sweep_" + kind)
    for cl in (False, True):
        pooled, uarg, dm = ffi.skip_pool_bwd_unit(ctx, g["maps"], g["scales"], g["rois"], d_raw=g["d_raw"], channels_last=cl)
        print("  %s %s: %d of %d arg-max cells differ, %d of %d gradient cells differ; |d| max %.0f" % (
            kind, "nhwc" if cl else "nchw", int((uarg != g["arg"]).sum()), uarg.size, int((dm[0] != g["want"][0]).sum()), dm[0].size,
            np.abs(g["want"][0]).max()))
        assert same_bits(pooled, g["raw"]) and same_bits(uarg, g["arg"])
        assert same_bits(dm[0], g["want"][0])


# ---- 8. conv_pool5 is the trainer's form-0 tile ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", [12, 132])
@pytest.mark.parametrize("sumC", [36, 64])
@pytest.mark.parametrize("rows", [1, 129])
def test_conv_pool5_has_the_trainer_gemms_bits(ctx, rows, sumC, Cout):
    """skip_conv(cat) with bp = 0 == max(gemm_unit form 0 (cat, Wp), 0), bit for bit: one tile (az_solver_dev.h) behind both
    kernels.  129 rows need a second, one-row tile in M, 132 outputs a partial tile in N, sumC = 36 a partial K stage past 32.
    The unit entry splits K (pick_split: two slabs of 32 at these shapes) and adds the slabs in a second kernel, conv_pool5 runs
    K in one pass; so the operands are multiples of 1/8 in [-2, 2]: every product is a multiple of 1/64, every partial sum
    of at most 64 of them is below 2^8 and so a multiple of 2^-6 below 2^14 -- exact in float32 in any order.  What is compared
    is then the staging, the bounds, the MFMA operand order and the C/D walk, not a summation order."""
    from aznet_hip import ffi, synth
    rng = np.random.Generator(np.random.PCG64(1000 * rows + 10 * sumC + Cout))
    cat = (rng.integers(-16, 17, (rows, sumC)) / 8.0).astype(np.float32)
    Wp = (rng.integers(-16, 17, (Cout, sumC)) / 8.0).astype(np.float32)
    front = dict(Cs=(sumC,), scales=S.SCALES[-1:], Wp=Wp, bp=np.zeros(Cout, np.float32), gain=1000.0, eps=1e-10)
    prod = ffi.gemm_unit(ctx, 0, cat, Wp)
    want = np.where(prod > 0, prod, np.float32(0))                   # (the kernel's own ReLU: y > 0 ? y : +0)
    with inference_context(synth.make_det_head(seed=9, C=Cout, n6=4, n7=4, ncls=2), front) as ictx:
        got = ictx.skip_conv(cat)
    exact = np.maximum(cat.astype(np.float64) @ Wp.astype(np.float64).T, 0.0)
    print("  rows %d sumC %d Cout %d: %d of %d outputs differ from the trainer's GEMM, %d from float64; %d positive" % (
        rows, sumC, Cout, int((got != want).sum()), got.size, int((got != exact).sum()), int((got > 0).sum())))
    assert (got > 0).any() and (got == 0).any()
    assert same_bits(got, want)
    assert np.array_equal(got.astype(np.float64), exact)
