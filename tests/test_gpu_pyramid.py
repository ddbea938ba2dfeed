"""GPU: multi-scale test pyramids (cfg.TEST.SCALES with several entries) -- az_roi_dedup_pyramid against what the
REFERENCE's own lib/detect/test.py recorded (tests/golden/g19_pyramid.npz), RoIPool on each roi's level, the pyramid
search (az_propose_pyramid, plain and tuner variant) and detection (az_detect_pyramid) against the oracle's level loop
with the pyramid projection (tests/pyramid_ref.py), S = 1 against the single-scale entries bit for bit, synchronous
argument errors, and a multi-scale YAML through the four CLIs."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pyramid_ref as pr
from helpers import load

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
SHAPE = (375, 500)
TARGETS, MAX_SIZE = (480, 576, 688), 1000


@pytest.fixture(scope="module")
def env():
    import torch
    from aznet_hip import ffi, synth
    from oracle import az_oracle as orc
    return torch, ffi, synth, orc


@pytest.fixture(scope="module")
def heads(env):
    torch, ffi, synth, orc = env
    return synth.make_head(seed=77, **synth.SMALL_DIMS), synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)


@pytest.fixture(scope="module")
def ctx(env, heads):
    torch, ffi, synth, orc = env
    c = ffi.AzContext(0)
    c.load_head(heads[0])
    c.load_det_head(heads[1])
    yield c
    c.close()


def _pyramid(env, scales, seed=40):
    """Seeded conv5_3 maps of the padded blob's size, one per level: NumPy [S,C,h,w] and channels_last CUDA tensors."""
    torch, ffi, synth, orc = env
    _, _, H, W = pr.blob_shape(SHAPE, scales)
    C = synth.SMALL_DIMS["C"]
    maps = np.concatenate([synth.make_feature_map(seed + i, C, synth.conv_out_size(H), synth.conv_out_size(W))
                           for i in range(len(scales))]).astype(np.float32)
    dev = [torch.from_numpy(m[None]).cuda().contiguous(memory_format=torch.channels_last) for m in maps]
    return maps, dev


def test_roi_dedup_pyramid_is_the_references(ctx):
    g = load("g19_pyramid.npz")
    for i in range(int(g["n_cases"])):
        rois, index, inv = ctx.roi_dedup_pyramid(g["c%d_boxes" % i], g["c%d_scales" % i], float(g["c%d_dedup" % i]),
                                                 int(g["c%d_batch" % i]))
        assert np.array_equal(rois, g["c%d_rois" % i]), i
        assert np.array_equal(index, g["c%d_index" % i]), i
        assert np.array_equal(inv, g["c%d_inv" % i]), i


def test_roi_pool_pyramid_reads_each_rois_level(env, ctx):
    torch, ffi, synth, orc = env
    scales = pr.scales_for(SHAPE, TARGETS, MAX_SIZE)
    maps, dev = _pyramid(env, scales)
    ctx.set_feature_pyramid(dev)
    rng = np.random.RandomState(5)
    n = 300
    x1, y1 = rng.uniform(-40, SHAPE[1], n), rng.uniform(-40, SHAPE[0], n)
    side = np.exp(rng.uniform(np.log(4), np.log(700), n))
    boxes = np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.5, 2, n)], 1)
    boxes[:20, 2:] = [SHAPE[1] + 300, SHAPE[0] + 300]           # past the padded border of every level
    rois = pr.rois_blob(boxes, scales)
    assert set(rois[:, 0].astype(int)) == {0, 1, 2}
    got = ctx.roi_pool_pyramid(rois)
    assert np.array_equal(got, pr.pool_pyramid(orc, maps, rois))


def test_pyramid_search_matches_the_oracle_level_loop(env, ctx, heads):
    torch, ffi, synth, orc = env
    scales = pr.scales_for(SHAPE, TARGETS, MAX_SIZE)
    maps, dev = _pyramid(env, scales)
    ctx.set_feature_pyramid(dev)
    for tune in (False, True):
        p = ffi.AzContext.make_params(SHAPE[0], SHAPE[1], scales[0], 0.0, batch_size=64, tune=tune)
        Y, S, st = ctx.propose_pyramid(p, scales, want_scores=True, want_stats=True)
        net = pr.PyramidNet(orc, heads[0], maps)
        cfg = orc.OracleCfg()
        cfg.BATCH_SIZE = 64
        with pr.oracle_on_pyramid(orc):
            if tune:
                YS, Bhis = orc.im_propose_tune(net, SHAPE, scales, cfg)
            else:
                Yref, tr = orc.im_propose(net, SHAPE, scales, cfg, return_trace=True)
        if tune:
            regions, zoom = ctx.last_anchors()
            assert regions.shape[0] == Bhis.shape[0]
            assert np.array_equal(regions, Bhis[:, :4])
            assert np.allclose(zoom, Bhis[:, 4], rtol=0, atol=1e-4)
            assert Y.shape[0] == YS.shape[0] and np.allclose(S, YS[:, 4], rtol=0, atol=1e-4)
            continue
        assert st.num_eval == tr["num_eval"] and st.depth == tr["depth"]
        for l, lv in enumerate(tr["levels"]):
            assert st.level_regions[l] == lv["B"].shape[0], l
            assert st.level_unique[l] == sum(f["U"] for f in lv["fwd"]), l
            assert st.level_zoomed[l] == len(lv["indZ"]), l
        Yall, Sall = ctx.last_candidates()
        assert Yall.shape == tr["Y_all"].shape
        assert np.allclose(Sall, tr["aScores"], rtol=0, atol=1e-4)
        assert np.allclose(Yall, tr["Y_all"], rtol=1e-4, atol=1e-3)
        assert Y.shape == (300, 4)
        # the rois each call of the oracle's loop forwarded: bit for bit the device projection + dedup of its level
        k = 0
        for l, lv in enumerate(tr["levels"]):
            rois, index, _ = ctx.roi_dedup_pyramid(lv["B"], scales, 1. / 16., 64)
            fed = np.concatenate(net.rec[k:k + len(lv["fwd"])])
            k += len(lv["fwd"])
            assert np.array_equal(rois[index], fed), l


def test_pyramid_detection_matches_the_oracle(env, ctx, heads):
    torch, ffi, synth, orc = env
    scales = pr.scales_for(SHAPE, TARGETS, MAX_SIZE)
    maps, dev = _pyramid(env, scales, seed=50)
    ctx.set_feature_pyramid(dev)
    rng = np.random.RandomState(9)
    x1, y1 = rng.uniform(-10, SHAPE[1] - 20, 300), rng.uniform(-10, SHAPE[0] - 20, 300)
    side = np.exp(rng.uniform(np.log(8), np.log(450), 300))
    boxes = np.round(np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.5, 2, 300)], 1), 1)
    boxes[250:] = boxes[:50]
    s, b = ctx.detect_pyramid(boxes, scales, SHAPE[0], SHAPE[1], batch_size=128)
    cfg = orc.OracleCfg()
    cfg.BATCH_SIZE = 128
    with pr.oracle_on_pyramid(orc):
        rs, rb = orc.frcnn_forward(pr.PyramidDetNet(orc, heads[1], maps), SHAPE, scales, boxes, s.shape[1],
                                   {"conv5_3": maps}, cfg)
    np.testing.assert_allclose(s, rs, rtol=0, atol=1e-4)
    np.testing.assert_allclose(b, rb, rtol=1e-4, atol=1e-3)


def test_one_level_is_bit_identical_to_the_single_scale_entries(env, ctx):
    torch, ffi, synth, orc = env
    scale = 1.6
    C = synth.SMALL_DIMS["C"]
    m = synth.make_feature_map(5, C, synth.conv_out_size(600), synth.conv_out_size(800))
    t = torch.from_numpy(m).cuda().contiguous(memory_format=torch.channels_last)
    for tune in (False, True):
        p = ffi.AzContext.make_params(SHAPE[0], SHAPE[1], scale, 0.3, tune=tune)
        ctx.set_feature_map(t)
        Y1, S1, st1 = ctx.propose(p, want_scores=True, want_stats=True)
        A1 = ctx.last_anchors() if tune else ctx.last_candidates()
        ctx.set_feature_pyramid([t])
        Y2, S2, st2 = ctx.propose_pyramid(p, [scale], want_scores=True, want_stats=True)
        A2 = ctx.last_anchors() if tune else ctx.last_candidates()
        assert np.array_equal(Y1, Y2) and np.array_equal(S1, S2)
        assert (st1.num_eval, st1.depth) == (st2.num_eval, st2.depth)
        assert list(st1.level_regions) == list(st2.level_regions) and list(st1.level_unique) == list(st2.level_unique)
        assert np.array_equal(A1[0], A2[0]) and np.array_equal(A1[1], A2[1])
    rng = np.random.RandomState(3)
    boxes = np.round(np.stack([rng.uniform(0, 300, 200), rng.uniform(0, 200, 200)], 1).repeat(2, 1) +
                     [0, 0, 1, 1] * rng.uniform(8, 200, (200, 1)), 1)
    ctx.set_feature_map(t)
    s1, b1 = ctx.detect(boxes, scale, SHAPE[0], SHAPE[1], batch_size=64)
    ctx.set_feature_pyramid([t])
    s2, b2 = ctx.detect_pyramid(boxes, [scale], SHAPE[0], SHAPE[1], batch_size=64)
    assert np.array_equal(s1, s2) and np.array_equal(b1, b2)
    r1 = ctx.roi_dedup(boxes, scale, 1. / 16., 64)
    r2 = ctx.roi_dedup_pyramid(boxes, [scale], 1. / 16., 64)
    assert all(np.array_equal(a, b) for a, b in zip(r1, r2))


def test_argument_errors_are_synchronous(env, ctx, heads):
    torch, ffi, synth, orc = env
    scales = pr.scales_for(SHAPE, TARGETS, MAX_SIZE)
    maps, dev = _pyramid(env, scales)
    ctx.set_feature_pyramid(dev)
    p = ffi.AzContext.make_params(SHAPE[0], SHAPE[1], scales[0], 0.0)
    boxes = np.array([[0, 0, 100, 100.0]])

    def code(fn, *a, **kw):
        with pytest.raises(ffi.AzError) as e:
            fn(*a, **kw)
        return e.value.code
    for bad in ([], list(np.ones(9)), [1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("nan"), 1.0], [1.0, np.inf, 1.0]):
        assert code(ctx.propose_pyramid, p, bad) == ffi.AZ_ERR_INVALID, bad
        assert code(ctx.detect_pyramid, boxes, bad, SHAPE[0], SHAPE[1]) == ffi.AZ_ERR_INVALID, bad
        assert code(ctx.roi_dedup_pyramid, boxes, bad) == ffi.AZ_ERR_INVALID, bad
    assert code(ctx.propose_pyramid, p, scales[:2]) == ffi.AZ_ERR_STATE          # two scales, three maps set
    assert code(ctx.detect_pyramid, boxes, scales[:2], SHAPE[0], SHAPE[1]) == ffi.AZ_ERR_STATE
    assert code(ctx.roi_pool_pyramid, np.array([[3, 0, 0, 10, 10]], np.float32)) == ffi.AZ_ERR_INVALID
    with pytest.raises(ValueError):
        other = torch.zeros((1, dev[0].shape[1], dev[0].shape[2] - 1, dev[0].shape[3]), device=dev[0].device)
        ctx.set_feature_pyramid([dev[0], other.contiguous(memory_format=torch.channels_last)])   # maps of two sizes
    with pytest.raises(ValueError):
        ctx.set_feature_pyramid(dev * 3)                                          # 9 > AZ_PYRAMID_MAX
    for mode in (2, 3):
        c2 = ffi.AzContext(0, gemm_mode=mode)
        try:
            c2.load_head(heads[0])
            c2.load_det_head(heads[1])
            c2.set_feature_pyramid(dev)
            assert code(c2.propose_pyramid, p, scales) == ffi.AZ_ERR_STATE
            assert code(c2.detect_pyramid, boxes, scales, SHAPE[0], SHAPE[1]) == ffi.AZ_ERR_STATE
        finally:
            c2.close()
    # the context still works after every refusal
    Y = ctx.propose_pyramid(p, scales)
    assert Y.shape == (300, 4)


# ---- a multi-scale YAML through the four CLIs ------------------------------------------------------------------------
def _run_tool(args, timeout=900):
    env = dict(os.environ)
    env["AZ_BACKBONE_DETERMINISTIC"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([TOOLS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(TOOLS, args[0])] + args[1:],
                          env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_multi_scale_yaml_through_the_clis(env, tmp_path):
    from detect import config as C
    exp = "pyramid_test_%d" % os.getpid()
    out_root = os.path.join(C.cfg.ROOT_DIR, "output", exp)
    yml = os.path.join(str(tmp_path), "pyramid.yml")
    with open(yml, "w") as f:
        f.write("TEST:\n  SCALES: [480, 600, 720]\n")
    imdb = "synthetic_600x1000_4"
    try:
        r = _run_tool(["prop_az.py", "--gpu", "0", "--net", "synthetic", "--imdb", imdb, "--tz", "0.5", "--exp", exp,
                       "--cfg", yml])
        assert r.returncode == 0, r.stdout[-3000:]
        assert r.stdout.count("proposals, evaluate") == 4
        pf = os.path.join(out_root, imdb, "vgg16_az_net_synthetic_1234", "proposals.pkl")
        with open(pf, "rb") as f:
            props = pickle.load(f)["boxes"]
        assert len(props) == 4 and all(p.ndim == 2 and p.shape[1] == 4 and 0 < p.shape[0] <= 300 for p in props)
        r = _run_tool(["set_thresh.py", "--gpu", "0", "--net", "synthetic", "--imdb", imdb, "--exp", exp, "--cfg", yml])
        assert r.returncode == 0, r.stdout[-3000:]
        assert "the threshold is set to" in r.stdout
        dets = {}
        for nb in (1, 4):
            r = _run_tool(["test_det_net.py", "--gpu", "0", "--def", "ignored.prototxt", "--net", "synthetic:7",
                           "--prop", pf, "--imdb", imdb, "--exp", exp, "--batch-images", str(nb), "--cfg", yml])
            assert r.returncode == 0, r.stdout[-3000:]
            assert r.stdout.count("im_detect: ") == 4
            df = os.path.join(out_root, imdb, "vgg16_frcnn_synthetic_7", "detections.pkl")
            with open(df, "rb") as f:
                dets[nb] = pickle.load(f)
            os.remove(df)
        for j in range(1, 21):
            for i in range(4):
                assert np.array_equal(dets[1][j][i], dets[4][j][i]), (j, i)
        shared = {}
        for nb in (1, 4):
            r = _run_tool(["test_shared.py", "--gpu", "0", "--net_az", "synthetic", "--net_frcnn", "synthetic:7",
                           "--imdb", imdb, "--exp", exp, "--tz", "0.5", "--batch-images", str(nb), "--cfg", yml])
            assert r.returncode == 0, r.stdout[-3000:]
            assert r.stdout.count("im_detect: ") == 4
            found = [os.path.join(d, f) for d, _, fs in os.walk(out_root) for f in fs if f == "detections.pkl"]
            assert len(found) == 1, found
            with open(found[0], "rb") as f:
                shared[nb] = pickle.load(f)
            os.remove(found[0])
        for j in range(1, 21):
            for i in range(4):
                assert np.array_equal(shared[1][j][i], shared[4][j][i]), (j, i)
    finally:
        shutil.rmtree(out_root, ignore_errors=True)
