"""GPU: the AZ head with int6 compressed by truncated SVD (az_load_head_lowrank) -- the head
(az_head_forward) on planted integer factors and on random heads, the load paths and refusals, every form of the search
on planted zoom trees whose zoom path the factors keep exact, and the tools end to end.  References: tests/lowrank_az_ref.py.
Every figure is printed before it is asserted (run with -s for the tables)."""
import functools
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

import head_sizes_ref as H
import lowrank_az_ref as AZ
import lowrank_ref as LR
import search_limits_ref as SL
import train_step_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")


def _pool(fmap, rois):
    from oracle import az_oracle as orc
    return orc.roi_pool(fmap[0], rois)


@pytest.fixture(scope="module")
def env():
    from aznet_hip import ffi
    ctx = ffi.AzContext(0, max_regions=AZ.CAP)
    yield ffi, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def planted(dims, r6):
    return AZ.planted_az_head(dims, r6, pool=_pool)


@functools.lru_cache(maxsize=None)
def rand(dims, r6):
    """The random case with the float64 and float32-CPU evaluations of the two-stage model (computed once)."""
    c = AZ.random_az_case(dims, r6)
    p5 = _pool(c["fmap"], c["rois"]).reshape(c["rois"].shape[0], -1)
    c["r64"], c["r32"] = AZ.head_on_pool5(c["head"], p5, np.float64), AZ.head_on_pool5(c["head"], p5, np.float32)
    return c


def check(tag, got, r64, r32):
    e_dev, e_cpu = R.rel_err(got, r64), R.rel_err(r32, r64)
    b = R.bound(e_cpu)
    print("  %-40s device %.3e   float32-CPU %.3e   bound %.3e   share %.2f   %s"
          % (tag, e_dev, e_cpu, b, e_dev / b, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b, e_dev / b


def same3(a, b, what):
    for x, y, n in zip(a, b, ("zoom_prob", "adj_prob", "adj_bbox")):
        assert x.shape == y.shape and np.array_equal(x, y), (what, n)


# ---- 1. the head ------------------------------------------------------------------------------------------------------------
PLANTED = [(d, r) for d in (AZ.SMALL, AZ.ODD) for r in AZ.RANKS[d]]


@pytest.mark.parametrize("dims,r6", PLANTED, ids=["%s-r%d" % ("x".join(map(str, d)), r) for d, r in PLANTED])
def test_planted_integer_factors_match_the_full_head(env, dims, r6):
    """U6, L6 small integers, W6 = U6 L6, every partial sum below 2^24: box outputs and scores of az_load_head_lowrank are
    bit for bit those of az_load_head(W6), at row counts on both sides of gemm12_min_rows and up to the context's capacity;
    the boxes are the exact integers; the probabilities are within 1e-6 of the float64 sigmoid of the exact scores."""
    ffi, ctx = env
    c = planted(dims, r6)
    rois = c["rois"]
    ctx.load_head(c["head"])
    assert ctx.dims["r6"] == r6
    ctx.set_feature_map(c["fmap"])
    low = {n: ctx.head_forward(rois[:n]) for n in AZ.ROWS}
    ctx.load_head(c["full"])
    assert "r6" not in ctx.dims
    ctx.set_feature_map(c["fmap"])
    worst = 0.0
    for n in AZ.ROWS:
        full = ctx.head_forward(rois[:n])
        same3(low[n], full, (dims, r6, n))
        assert np.array_equal(low[n][2], c["bbox"][:n]), (dims, r6, n)
        worst = max(worst, float(np.abs(low[n][0] - c["p64"]["zoom"][:n]).max()), float(np.abs(low[n][1] - c["p64"]["adj"][:n]).max()))
    print("planted %s r6 = %d: k = %d, max |prob - float64| = %.3e" % (dims, r6, c["k"], worst))
    assert worst <= 1e-6


def test_planted_factors_on_the_many_row_l_stage(env):
    """K6 = 18816 at rank 128: from gemm12_min_rows on the L stage runs on the many-row GEMM (294 chunks of 64), below on
    k_fc_splitk; the full head W6 = U6 L6 (n6 = 132) stays on k_fc_splitk with 16 chunks.  All of them give the exact
    integers."""
    ffi, ctx0 = env
    c = AZ.planted_az_head(AZ.MANY, AZ.MANY_RANK, pool=_pool, rois=H.rois300())
    assert ffi.az_lowrank_split(49 * AZ.MANY[0], AZ.MANY_RANK) == 294
    ctx = ffi.AzContext(0, max_regions=512)
    try:
        out = {}
        for tag in ("head", "full"):
            ctx.load_head(c[tag])
            ctx.set_feature_map(c["fmap"])
            out[tag] = {n: ctx.head_forward(c["rois"][:n]) for n in AZ.MANY_ROWS}
        for n in AZ.MANY_ROWS:
            same3(out["head"][n], out["full"][n], n)
            assert np.array_equal(out["head"][n][2], c["bbox"][:n]), n
    finally:
        ctx.close()


RANDOM = [(AZ.SMALL, 36), (AZ.SMALL, 128), (AZ.ODD, 4), (AZ.ODD, 132), (AZ.ODD, 256)]


@pytest.mark.parametrize("dims,r6", RANDOM, ids=["%s-r%d" % ("x".join(map(str, d)), r) for d, r in RANDOM])
def test_random_head_within_the_rule_and_a_rois_bits_do_not_depend_on_its_batch(env, dims, r6):
    """synth heads compressed at rank r6 against the float64 restatement of the two-stage model: every output within 8 x the
    float32-CPU restatement's own error.  Rows of shorter launches, and a roi alone, have the bits of the 300-row launch."""
    ffi, ctx = env
    c = rand(dims, r6)
    rois = c["rois"]
    ctx.load_head(c["head"])
    ctx.set_feature_map(c["fmap"])
    ref = ctx.head_forward(rois)
    ok, worst = True, 0.0
    print("random AZ head %s at rank %d" % (dims, r6))
    for name, got, r64, r32 in zip(("zoom_prob", "adj_prob", "adj_bbox"), ref, c["r64"], c["r32"]):
        good, share = check(name, got, r64, r32)
        ok, worst = ok and good, max(worst, share)
    print("  worst share of the bound: %.2f" % worst)
    for n in (1, 31, 33, 160, 161, 299):
        same3(ctx.head_forward(rois[:n]), [y[:n] for y in ref], ("prefix", n))
    for j in (0, 161, 299):
        same3(ctx.head_forward(rois[j:j + 1]), [y[j:j + 1] for y in ref], ("alone", j))
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


def test_a_roi_alone_and_among_688_others(env):
    """One roi at the front, in the middle and at the end of launches of 2 .. 689 rows (both sides of gemm12_min_rows):
    the same bits as alone."""
    ffi, ctx = env
    c = rand(AZ.ODD, 132)
    ctx.load_head(c["head"])
    ctx.set_feature_map(c["fmap"])
    others = AZ.rois_all()[:688]
    one = c["rois"][7:8]
    alone = ctx.head_forward(one)
    for n in (1, 32, 159, 160, 161, 688):
        for pos in (0, n // 2, n):
            batch = np.concatenate([others[:pos], one, others[pos:n]], 0)
            got = ctx.head_forward(batch)
            same3([g[pos:pos + 1] for g in got], alone, (n, pos))


def test_low_rank_full_low_rank_on_one_context_equals_fresh_contexts(env):
    ffi, ctx = env
    a, b = rand(AZ.ODD, 36), rand(AZ.ODD, 256)
    rois = a["rois"]
    seq = ((a["head"], a["fmap"]), (a["uncompressed"], a["fmap"]), (b["head"], b["fmap"]))
    got = []
    for head, fmap in seq:
        ctx.load_head(head)
        ctx.set_feature_map(fmap)
        got.append([ctx.head_forward(rois[:n]) for n in (48, 300)])
    for (head, fmap), g in zip(seq, got):
        fresh = ffi.AzContext(0, max_regions=512)
        try:
            fresh.load_head(head)
            fresh.set_feature_map(fmap)
            for n, x in zip((48, 300), g):
                same3(fresh.head_forward(rois[:n]), x, n)
        finally:
            fresh.close()


def _zero_low(C, n6, r6, n71=8, n72=4):
    z = lambda *s: np.zeros(s, np.float32)          # noqa: E731
    return {"L6": z(r6, C * 49), "U6": z(n6, r6), "b6": z(n6), "W71": z(n71, n6), "b71": z(n71), "W72": z(n72, n6), "b72": z(n72),
            "Was": z(11, n71), "bas": z(11), "Wab": z(44, n71), "bab": z(44), "Wz": z(1, n72), "bz": z(1)}


def test_refusals_leave_the_loaded_head_answering(env):
    """r6 no multiple of 4, below 4, above n6, above C * 49, above AZ_LOWRANK_MAX and az_load_head's own size rules:
    AZ_ERR_INVALID; the head loaded before (low rank, then full) answers with the same bits."""
    ffi, ctx = env
    c = rand(AZ.ODD, 36)
    bad = [_zero_low(44, 260, 6), _zero_low(44, 260, 2), _zero_low(44, 260, 264), _zero_low(4, 260, 200),
           _zero_low(44, 2056, ffi.AZ_LOWRANK_MAX + 4), _zero_low(44, 258, 36), _zero_low(44, 260, 36, n71=3000, n72=76)]
    for head in (c["head"], c["uncompressed"]):
        ctx.load_head(head)
        ctx.set_feature_map(c["fmap"])
        want = ctx.head_forward(c["rois"][:48])
        for i, z in enumerate(bad):
            with pytest.raises(ffi.AzError) as e:
                ctx.load_head(z)
            assert e.value.code == ffi.AZ_ERR_INVALID and "az_load_head_lowrank" in str(e.value), i
            same3(ctx.head_forward(c["rois"][:48]), want, i)
    with pytest.raises(ValueError, match="both L6 and U6"):
        ctx.load_head({k: v for k, v in c["head"].items() if k != "U6"})
    with pytest.raises(ValueError, match="do not chain"):
        ctx.load_head(dict(c["head"], U6=c["head"]["U6"][:, :-4]))


@pytest.mark.parametrize("mode", [2, 3])
def test_gemm_modes_refuse_a_lowrank_az_head(mode):
    from aznet_hip import ffi
    c = rand(AZ.SMALL, 36)
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=mode)
    try:
        ctx.load_head(c["uncompressed"])
        ctx.set_feature_map(c["fmap"])
        want = ctx.head_forward(c["rois"][:48])
        with pytest.raises(ffi.AzError) as e:
            ctx.load_head(c["head"])
        assert e.value.code == ffi.AZ_ERR_STATE and "fp32 only" in str(e.value) and "az_load_head_lowrank" in str(e.value)
        same3(ctx.head_forward(c["rois"][:48]), want, mode)
    finally:
        ctx.close()
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=0)
    try:
        ctx.load_head(c["head"])
        assert ctx.L.az_set_gemm_mode(ctx.h, mode) == ffi.AZ_ERR_STATE
        assert "az_load_head" in ctx.L.az_last_error(ctx.h).decode()
    finally:
        ctx.close()


def test_az_and_detection_low_rank_heads_share_a_context(env):
    """test_shared's arrangement: both compressed heads on one context give the bits of two separate contexts."""
    ffi, ctx = env
    from aznet_hip import synth
    a = rand(AZ.SMALL, 36)
    det = synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)
    det_low = {k: v for k, v in det.items() if k not in ("W6", "W7")}
    det_low["L6"], det_low["U6"] = LR.compress_layer(det["W6"], 36)
    det_low["L7"], det_low["U7"] = LR.compress_layer(det["W7"], 20)
    rois = a["rois"]
    ctx.load_head(a["head"])
    ctx.load_det_head(det_low)
    ctx.set_feature_map(a["fmap"])
    got = []
    for n in (48, 300):
        got.append((ctx.head_forward(rois[:n]), ctx.det_forward(rois[:n]), ctx.head_forward(rois[:n])))
    one, two = ffi.AzContext(0, max_regions=512), ffi.AzContext(0, max_regions=512)
    try:
        one.load_head(a["head"])
        one.set_feature_map(a["fmap"])
        two.load_head(a["uncompressed"])
        two.load_det_head(det_low)
        two.set_feature_map(a["fmap"])
        for n, (az1, dt, az2) in zip((48, 300), got):
            want = one.head_forward(rois[:n])
            same3(az1, want, n)
            same3(az2, want, n)
            for x, y in zip(dt, two.det_forward(rois[:n])):
                assert np.array_equal(x, y), n
    finally:
        one.close()
        two.close()


def test_profiling_names_the_three_launches(env):
    ffi, ctx = env
    c = rand(AZ.SMALL, 36)
    ctx.load_head(c["head"])
    ctx.set_feature_map(c["fmap"])
    ctx.set_profiling(2)
    try:
        ctx.head_forward(c["rois"])
        names = [n for n, _, _ in ctx.last_kernel_times()]
    finally:
        ctx.set_profiling(0)
    i = names.index("fc6_L")
    assert names[i:i + 3] == ["fc6_L", "fc6_L_reduce", "fc6_U"] and "fc6_gemm" not in names and "fc6_reduce" not in names
    assert names.index("roi_pool") < i < names.index("fc7_gemm")


# ---- 2. the search ---------------------------------------------------------------------------------------------------------
CASES = SL.load_cases()
NAMES = ("cap", "pre_49")
RANK = 36
PLAIN = dict(speculate=False, fused=False, fused_levels=False, static_tree=False, pair_spec=False, full_spec=False,
             early_end=False)
# (tests/test_gpu_search_limits.py: FORMS, restated)
FORMS = {"default": {}, "fused_only": dict(fused=True, fused_levels=False), "levels_only": dict(fused=False, fused_levels=True),
         "pair": dict(pair_spec=True), "full": dict(full_spec=True), "closure": dict(full_spec="closure")}


def params(ffi, name, **kw):
    c = CASES[name]
    return ffi.AzContext.make_params(c["H"], c["W"], c["scale"], SL.TZ, **kw)


def result(net, got):
    Y, S, st = got
    Ya, Sa = net.ctx.last_candidates()
    return dict(Y=Y, S=S, Ya=Ya, Sa=Sa, st=st)


def run(ffi, net, name, **kw):
    return result(net, net.propose(params(ffi, name, **kw), want_scores=True, want_stats=True))


def same(a, b, what="", candidates=True):
    for k in ("Y", "S") + (("Ya", "Sa") if candidates else ()):
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), (what, k)
    for f in ("n_proposals", "num_eval", "depth", "n_levels", "n_candidates"):
        assert getattr(a["st"], f) == getattr(b["st"], f), (what, f)
    for f in ("level_regions", "level_unique", "level_zoomed"):
        assert list(getattr(a["st"], f)) == list(getattr(b["st"], f)), (what, f)


@pytest.fixture(scope="module")
def world():
    """The compressed head (one for all cases: the zoom-exact factors of the cases' head at rank 36), every case's map and
    the plain level loop's result, computed once on a context of its own."""
    from aznet_hip import ffi
    from aznet_hip.net import HipAZNet

    class World(object):
        pass

    w = World()
    inp = {k: SL.case_inputs(CASES[k]) for k in NAMES}
    w.full = inp[NAMES[0]][0]
    w.head = AZ.zoom_exact_factors(w.full, RANK)
    w.fmap = {k: v[1] for k, v in inp.items()}
    w.plain_net = HipAZNet(w.head, name="lraz_plain")
    assert w.plain_net.ctx.dims["r6"] == RANK
    w.plain = {}
    for k in NAMES:
        w.plain_net.set_conv(w.fmap[k])
        w.plain[k] = run(ffi, w.plain_net, k, **PLAIN)
    yield w
    w.plain_net.ctx.close()


def fresh(world, name, tag, **kw):
    from aznet_hip import ffi
    from aznet_hip.net import HipAZNet
    net = HipAZNet(world.head, name="lraz_%s_%s" % (name, tag), **kw)
    net.ctx.set_pass_costs(ffi.AzContext.REFERENCE_PASS_COSTS)      # (as tests/test_gpu_search_limits.py pins them)
    net.set_conv(world.fmap[name])
    return net


@pytest.mark.parametrize("name", NAMES)
def test_plain_loop_walks_the_planted_tree_and_is_the_oracles_loop(world, name):
    from oracle import az_oracle as orc
    c, p = CASES[name], SL.case_populations(CASES[name])
    got = world.plain[name]
    st = got["st"]
    assert st.n_reruns == 0 and st.search_form == 0 and st.n_levels == p["nlev"]
    for l in range(p["nlev"]):
        assert (st.level_regions[l], st.level_unique[l], st.level_zoomed[l]) == (p["P"][l], p["U"][l], p["PZ"][l]), (name, l)
    net, fmap = world.plain_net, world.fmap[name]

    class Injected(object):      # pycaffe-shaped view of the HIP head
        name = "inj"
        blobs = net.blobs

        def forward(self, blobs=None, **kw):
            kw.pop("data", None)
            kw["conv5_3"] = fmap
            return net.forward(blobs=blobs, **kw)

    inj = Injected()
    _, tr = orc.im_propose({"full": inj, "fc": inj}, (c["H"], c["W"]), c["scale"], orc.OracleCfg(Tz=SL.TZ), return_trace=True)
    assert st.depth == tr["depth"] and st.num_eval == tr["num_eval"]
    assert got["Ya"].shape == tr["Y_all"].shape
    assert np.array_equal(got["Sa"].astype(np.float64), tr["aScores"])              # scores: same bits
    np.testing.assert_allclose(got["Ya"], tr["Y_all"], rtol=1e-6, atol=1e-4)        # decode: f32-exp ulps (px)
    idx = np.argsort(-tr["aScores"], kind="stable")[:300]
    assert np.array_equal(got["Y"], got["Ya"][idx]) and np.array_equal(got["S"], got["Sa"][idx])
    # the compressed head is another model: its adjacency scores are not the full head's, its tree is
    full = fresh(world, name, "fullhead")
    full.ctx.load_head(world.full)
    full.set_conv(fmap)
    from aznet_hip import ffi
    ref = run(ffi, full, name, **PLAIN)
    assert list(ref["st"].level_regions) == list(st.level_regions) and list(ref["st"].level_zoomed) == list(st.level_zoomed)
    assert not np.array_equal(ref["Sa"], got["Sa"])
    full.ctx.close()


FORM_CASES = [(n, f) for n in NAMES for f in sorted(FORMS)]


@pytest.mark.parametrize("name,form", FORM_CASES, ids=["%s-%s" % nf for nf in FORM_CASES])
def test_every_form_gives_the_plain_loops_bits(world, name, form):
    from aznet_hip import ffi
    net = fresh(world, name, form)
    try:
        for turn in ("first", "again"):
            got = run(ffi, net, name, static_tree=False, **FORMS[form])
            same(got, world.plain[name], (name, form, turn))
            print(name, form, turn, "n_reruns", got["st"].n_reruns, "form", got["st"].search_form, "passes", got["st"].n_passes)
            # (tests/test_gpu_search_limits.py: WHOLE / expected_first for these two trees, which fit every table -- a forced
            #  form is taken, in one pass where it is a whole-tree form, and nothing is handed over)
            assert got["st"].n_reruns == 0, (name, form, turn)
            if form in ("full", "closure"):
                assert (got["st"].search_form, got["st"].n_passes) == ({"full": 2, "closure": 3}[form], 1), (name, form, turn)
            elif form == "pair":
                assert turn == "again" or got["st"].search_form == 1, (name, form)
            elif form in ("fused_only", "levels_only") or turn == "first":
                assert got["st"].search_form == 0, (name, form, turn)
    finally:
        net.ctx.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_three_searches_queued_on_one_and_two_lanes(world, lanes):
    import torch
    from aznet_hip import ffi
    net = fresh(world, NAMES[0], "lanes%d" % lanes)
    try:
        net.ctx.set_lanes(lanes)
        maps = {n: torch.from_numpy(world.fmap[n]).cuda() for n in NAMES}
        order = (NAMES[0], NAMES[1], NAMES[0])
        for rnd in range(3):
            for n in order:
                net.ctx.propose_launch(params(ffi, n, static_tree=False), fmap=maps[n])
            for n in order:
                Y, S, st = net.ctx.propose_fetch(want_scores=True, want_stats=True)
                ref = world.plain[n]
                assert np.array_equal(Y, ref["Y"]) and np.array_equal(S, ref["S"]), (lanes, rnd, n)
                assert list(st.level_regions) == list(ref["st"].level_regions) and st.num_eval == ref["st"].num_eval
    finally:
        net.ctx.close()


@pytest.mark.parametrize("name", NAMES)
def test_graph_replay(world, name):
    from aznet_hip import ffi
    net = fresh(world, name, "graph")
    try:
        net.ctx.set_graphs(True)
        for turn in range(3):                    # (un-captured + capture, then replays)
            same(run(ffi, net, name, static_tree=False), world.plain[name], (name, "graph", turn))
        # a reload drops the captured launches of the old head: the full head's search on the same map is its own
        net.ctx.load_head(world.full)
        net.set_conv(world.fmap[name])
        a = run(ffi, net, name, static_tree=False)
        net.ctx.set_graphs(False)
        b = run(ffi, net, name, **PLAIN)
        same(a, b, (name, "graph after reload"))
        assert not np.array_equal(a["Sa"], world.plain[name]["Sa"])
    finally:
        net.ctx.close()


def test_batch_of_three_images_against_each_alone(world):
    import torch
    from aznet_hip import ffi
    name = NAMES[0]
    fh, fw = world.fmap[name].shape[2:]
    rng = np.random.Generator(np.random.PCG64(3))
    fmaps = [world.fmap[name]]
    for i in range(2):                           # two more 0/1 masks of the shape: other trees
        m = world.fmap[name].copy()
        m[0, SL.HEAD_KW["zoom_channel"]] = (rng.random((fh, fw)) < (0.02, 0.3)[i]).astype(np.float32)
        fmaps.append(m)
    alone = []
    for m in fmaps:
        world.plain_net.set_conv(m)
        alone.append(run(ffi, world.plain_net, name, **PLAIN))
    assert len({tuple(a["st"].level_regions) for a in alone}) == 3
    net = fresh(world, name, "batch")
    try:
        dev = [torch.from_numpy(m).cuda().contiguous(memory_format=torch.channels_last) for m in fmaps]
        for turn in range(2):
            net.ctx.batch_launch(params(ffi, name), dev)
            for i, ref in enumerate(alone):
                Y, S, st = net.ctx.batch_fetch(i, want_scores=True, want_stats=True)
                assert np.array_equal(Y, ref["Y"]) and np.array_equal(S, ref["S"]), (turn, i)
                assert list(st.level_regions) == list(ref["st"].level_regions) and st.num_eval == ref["st"].num_eval
    finally:
        net.ctx.close()


def test_pyramid_of_two_scales():
    """az_propose_pyramid over two distinct scales with a compressed head (rank 36) against the oracle's level loop with the
    pyramid projection, RoIPool on each roi's level and the two-stage head restated on the CPU (tests/pyramid_ref.py, as
    tests/test_gpu_pyramid.py checks the full head): the same tree, candidates and scores within that test's tolerances, and
    the rois of every call bit for bit the device's projection and dedup."""
    import torch
    import pyramid_ref as pr
    from aznet_hip import ffi, synth
    from oracle import az_oracle as orc
    shape, max_size = (375, 500), 1000
    scales = pr.scales_for(shape, (480, 688), max_size)
    assert len(scales) == 2 and scales[0] != scales[1]
    _, _, Hb, Wb = pr.blob_shape(shape, scales)
    C = synth.SMALL_DIMS["C"]
    maps = np.concatenate([synth.make_feature_map(40 + i, C, synth.conv_out_size(Hb), synth.conv_out_size(Wb))
                           for i in range(2)]).astype(np.float32)
    dev = [torch.from_numpy(m[None]).cuda().contiguous(memory_format=torch.channels_last) for m in maps]
    head = rand(AZ.SMALL, 36)["head"]

    class LowNet(pr.PyramidNet):
        def forward(self, blobs=None, **kw):
            h, rois = self.head, kw["rois"]
            self.rec.append(np.array(rois, dtype=np.float32))
            p5 = pr.pool_pyramid(orc, self.maps, rois)
            t = orc.fc(p5, h["L6"], np.zeros(h["L6"].shape[0], np.float32), False)
            h6 = orc.fc(t, h["U6"], h["b6"], True)
            h71, h72 = orc.fc(h6, h["W71"], h["b71"], True), orc.fc(h6, h["W72"], h["b72"], True)
            out = {"zoom_prob": orc.sigmoid(orc.fc(h72, h["Wz"], h["bz"], False)),
                   "adj_prob": orc.sigmoid(orc.fc(h71, h["Was"], h["bas"], False)), "adj_bbox": orc.fc(h71, h["Wab"], h["bab"], False)}
            for b in blobs or []:
                out[b] = self.maps
            return out

    ctx = ffi.AzContext(0)
    try:
        ctx.load_head(head)
        ctx.set_feature_pyramid(dev)
        p = ffi.AzContext.make_params(shape[0], shape[1], scales[0], 0.0, batch_size=64)
        Y, S, st = ctx.propose_pyramid(p, scales, want_scores=True, want_stats=True)
        net = LowNet(orc, head, maps)
        cfg = orc.OracleCfg()
        cfg.BATCH_SIZE = 64
        with pr.oracle_on_pyramid(orc):
            _, tr = orc.im_propose(net, shape, scales, cfg, return_trace=True)
        assert st.num_eval == tr["num_eval"] and st.depth == tr["depth"]
        Yall, Sall = ctx.last_candidates()
        assert Yall.shape == tr["Y_all"].shape and Y.shape == (300, 4)
        assert np.allclose(Sall, tr["aScores"], rtol=0, atol=1e-4)
        assert np.allclose(Yall, tr["Y_all"], rtol=1e-4, atol=1e-3)
        k, levels = 0, set()
        for l, lv in enumerate(tr["levels"]):
            assert st.level_regions[l] == lv["B"].shape[0] and st.level_unique[l] == sum(f["U"] for f in lv["fwd"]), l
            rois, index, _ = ctx.roi_dedup_pyramid(lv["B"], scales, 1. / 16., 64)
            fed = np.concatenate(net.rec[k:k + len(lv["fwd"])])
            k += len(lv["fwd"])
            assert np.array_equal(rois[index], fed), l
            levels |= set(fed[:, 0].astype(int))
        assert levels == {0, 1}                                     # (both levels of the pyramid carry rois)
    finally:
        ctx.close()


def test_search_and_batch_send_the_l_stage_through_the_many_row_gemm():
    """K6 = 18816 at rank 128 (294 chunks: the many-row GEMM takes the L stage from gemm12_min_rows on).  The Tz = 0 search of
    a 375 x 500 image in its one-pass form (one pass of several hundred rows, through launch_head) and a lockstep batch of
    two such images (head_pass_batch) against the plain level loop, whose small passes stay on k_fc_splitk: the same bits."""
    import torch
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipAZNet
    kw = dict(SL.HEAD_KW)
    kw.update(C=AZ.MANY[0], n6=AZ.MANY[1], n71=64, n72=32)
    head = AZ.zoom_exact_factors(synth.make_object_head(**kw), AZ.MANY_RANK)
    c = CASES["cap"]
    fh, fw = SL.map_size(c["H"], c["W"], c["scale"])
    fmaps = [synth.make_feature_map(70 + i, AZ.MANY[0], fh, fw) for i in range(2)]
    net = HipAZNet(head, name="lraz_many", max_regions=2048)
    try:
        assert net.ctx.dims["r6"] == AZ.MANY_RANK and ffi.az_lowrank_split(49 * AZ.MANY[0], AZ.MANY_RANK) == 294
        plain, one = [], []
        for m in fmaps:
            net.set_conv(m)
            plain.append(result(net, net.propose(ffi.AzContext.make_params(c["H"], c["W"], c["scale"], 0.0, **PLAIN),
                                                 want_scores=True, want_stats=True)))
            one.append(result(net, net.propose(ffi.AzContext.make_params(c["H"], c["W"], c["scale"], 0.0),
                                               want_scores=True, want_stats=True)))
        for a, b in zip(one, plain):
            same(a, b, "one pass")
            rows = [int(a["st"].pass_rows[i]) for i in range(a["st"].n_passes)]
            assert a["st"].n_passes == 1 and rows[0] >= 161, rows
            assert max(int(b["st"].pass_rows[i]) for i in range(b["st"].n_passes)) >= 161     # (the plain loop's deep levels too)
            assert min(int(b["st"].pass_rows[i]) for i in range(b["st"].n_passes)) < 161
        dev = [torch.from_numpy(m).cuda().contiguous(memory_format=torch.channels_last) for m in fmaps]
        for turn in range(2):
            net.ctx.batch_launch(ffi.AzContext.make_params(c["H"], c["W"], c["scale"], 0.0), dev)
            for i, ref in enumerate(plain):
                Y, S, st = net.ctx.batch_fetch(i, want_scores=True, want_stats=True)
                assert np.array_equal(Y, ref["Y"]) and np.array_equal(S, ref["S"]), (turn, i)
                assert st.num_eval == ref["st"].num_eval
    finally:
        net.ctx.close()


# ---- 3. end to end, once ---------------------------------------------------------------------------------------------------
def _snapshot_layers(seed=7, width_div=16, n6=260, n71=132, n72=36):
    """{layer: blobs} of a seeded AZ-net snapshot: a VGG16 at 1 / width_div of its width and a reduced head."""
    from aznet_hip import synth
    from aznet_hip.backbone import VGG16Conv5
    bk = VGG16Conv5(device="cpu", seed=seed + 1, width_div=width_div)
    bk.normalize_output(np.ones((1, 3, 600, 800), dtype=np.float32))
    conv = [layer for layer in bk.layers if layer is not None]
    C = int(conv[-1][1].shape[0])
    head = synth.make_head(seed=seed, C=C, n6=n6, n71=n71, n72=n72)
    layers = {name: [w.numpy(), b.numpy()] for name, w, b in conv}
    for name, w, b in (("int6", "W6", "b6"), ("int7_1", "W71", "b71"), ("int7_2", "W72", "b72"), ("adj_score", "Was", "bas"),
                       ("adj_bbox", "Wab", "bab"), ("zoom_score", "Wz", "bz")):
        layers[name] = [head[w], head[b]]
    return layers, C


def test_compress_net_then_prop_az(tmp_path):
    """compress_net.py --int6 <full rank> on a synthetic snapshot, prop_az.py --net on the file; then, in this process, the
    compressed and the uncompressed net's head outputs on one image's map against the float64 restatement of the
    compressed model, within the rule; and their Tz = 0 searches (the same tree) propose from candidate sets of one shape."""
    import torch
    from aznet_hip import caffemodel as cm
    from datasets.factory import get_imdb
    from detect import config as Cf
    from detect import test as T
    import pyramid_ref as pr
    from oracle import az_oracle as orc
    layers, C = _snapshot_layers()
    base = str(tmp_path / "az16.caffemodel")
    cm.write_caffemodel(base, layers)
    sys.path[:0] = [TOOLS]
    try:
        import compress_net
        import prop_az
    finally:
        sys.path.remove(TOOLS)
    r6 = min(260, C * 49)                                        # full rank: the compressed model is the model
    path = compress_net.main(["--net", base, "--int6", str(r6)])
    assert path == str(tmp_path / ("az16_svd_int6_%d.caffemodel" % r6))
    got_layers = cm.load_caffemodel(path)
    assert "int6" not in got_layers and set(got_layers) - {"int6_L", "int6_U"} == set(layers) - {"int6"}
    exp = "lowrank_az_test_%d" % os.getpid()
    out_root = os.path.join(Cf.cfg.ROOT_DIR, "output", exp)
    env = dict(os.environ)
    env["AZ_BACKBONE_DETERMINISTIC"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([TOOLS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    old = (torch.backends.cudnn.deterministic, Cf.cfg.EXP_DIR)
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(TOOLS, "prop_az.py"), "--gpu", "0", "--net", path,
                            "--imdb", "synthetic_375x500_4", "--tz", "0.0", "--exp", exp], env=env, cwd=REPO, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        pf = os.path.join(out_root, "synthetic_375x500_4", os.path.splitext(os.path.basename(path))[0], "proposals.pkl")
        with open(pf, "rb") as f:
            prop = pickle.load(f)
        assert len(prop["boxes"]) == 4 and all(b.shape == (300, 4) for b in prop["boxes"])
        torch.backends.cudnn.deterministic = True
        im = get_imdb("synthetic_375x500_4").image_at(0)
        head = cm.az_head_from_layers(got_layers)
        assert head["L6"].shape == (r6, C * 49) and head["U6"].shape == (260, r6)
        rois = H.rois300()
        rois[:, 1:] *= np.float32(0.9)                            # (inside the scaled 375 x 500 image)
        out, cand, props = {}, {}, {}
        for tag, spec in (("compressed", path), ("uncompressed", base)):
            net = prop_az.load_net(spec, 0)
            assert net.ctx.dims.get("r6", 0) == (r6 if tag == "compressed" else 0)
            scale = T._im_scale(im.shape)[0]
            conv = net.compute_conv(net.image_blob_enqueue(im, Cf.cfg.PIXEL_MEANS, scale))
            fmap = conv.detach().cpu().contiguous().numpy()
            net.set_conv(fmap)
            out[tag] = net.ctx.head_forward(rois)
            p = net.ctx.make_params(im.shape[0], im.shape[1], scale, 0.0)
            Y, S, st = net.propose(p, want_scores=True, want_stats=True)
            cand[tag] = (Y.shape, net.ctx.last_candidates()[0].shape, list(st.level_regions))
            props[tag] = (Y, S) + tuple(net.ctx.last_candidates())
            if tag == "compressed":
                shape_scale = (im.shape[:2], scale)
                fmap_c = fmap
            if tag == "compressed":
                p5 = orc.roi_pool(fmap[0], rois).reshape(300, -1)
                r64, r32 = AZ.head_on_pool5(head, p5, np.float64), AZ.head_on_pool5(head, p5, np.float32)
            net.ctx.close()
        assert cand["compressed"] == cand["uncompressed"]
        ok = True
        for tag in ("compressed", "uncompressed"):
            for name, got, a, b in zip(("zoom_prob", "adj_prob", "adj_bbox"), out[tag], r64, r32):
                ok &= check("%s net, %s" % (tag, name), got, a, b)[0]
        # the proposals: the oracle's level loop (Tz = 0: the tree is the shape's) on the compressed model, its head in
        # float64 and in float32 on the CPU -- candidates, their scores and the 300 proposals of both nets within the rule
        class ModelNet(object):
            def __init__(self, dtype):
                self.dtype, self.blobs = dtype, {k: pr.PyramidNet._Blob() for k in ("data", "rois", "conv5_3")}

            def forward(self, blobs=None, **kw):
                rois = np.asarray(kw["rois"], np.float32)
                z, a, d = AZ.head_on_pool5(head, orc.roi_pool(fmap_c[0], rois).reshape(rois.shape[0], -1), self.dtype)
                o = {"zoom_prob": z, "adj_prob": a, "adj_bbox": d}
                for b in blobs or []:
                    o[b] = fmap_c
                return o

        ref = {}
        for dt in (np.float64, np.float32):
            m = ModelNet(dt)
            Yr, tr = orc.im_propose({"full": m, "fc": m}, shape_scale[0], shape_scale[1], orc.OracleCfg(Tz=0.0), return_trace=True)
            idx = np.argsort(-tr["aScores"], kind="stable")[:300]
            ref[dt] = (tr["Y_all"][idx], tr["aScores"][idx], tr["Y_all"], tr["aScores"])
        for tag in ("compressed", "uncompressed"):
            assert props[tag][2].shape == ref[np.float64][2].shape
            ok &= check("%s net, candidate scores" % tag, props[tag][3], ref[np.float64][3], ref[np.float32][3])[0]
            ok &= check("%s net, candidate boxes" % tag, props[tag][2], ref[np.float64][2], ref[np.float32][2])[0]
            ok &= check("%s net, proposal scores" % tag, props[tag][1], ref[np.float64][1], ref[np.float32][1])[0]
            ok &= check("%s net, proposal boxes" % tag, props[tag][0], ref[np.float64][0], ref[np.float32][0])[0]
        assert ok, "a tensor exceeds 8 x the float32-CPU error against the compressed model in float64"
    finally:
        torch.backends.cudnn.deterministic, Cf.cfg.EXP_DIR = old
        shutil.rmtree(out_root, ignore_errors=True)
