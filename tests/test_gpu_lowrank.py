"""GPU: the truncated-SVD detection head (az_load_det_head_lowrank; references and cases: tests/lowrank_ref.py).

  1. the U-stage kernel alone (az_lowrank_gemm_unit) on integer operands, bit for bit, over row counts around its 64-row
     tiles, widths that are no multiple of its 64-column tiles and K that are no multiple of its 32-wide K step;
  2. heads whose factors are small integers, so that W = U L and every intermediate is exact: the low-rank head against
     az_load_det_head(U L) bit for bit in bbox_pred -- the feature pinned to the existing head without a restatement;
  3. random heads against the float64 / float32 restatements of the two-stage model (the 8 x rule), a roi's bits alone
     and among others, az_detect_batch against az_detect, one case through az_detect_pyramid and az_detect_skip;
  4. load paths: full -> low-rank -> full, refusals, the 16-bit-term GEMM modes;
  5. tools/compress_net.py -> tools/test_det_net.py on a synthetic detection snapshot, once.
Every figure is printed before it is asserted (run with -s for the table)."""
import functools
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

import det_infer_ref as D
import head_sizes_ref as H
import lowrank_ref as LR
import pyramid_ref as PR
import skip_ref as S
import train_step_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")
ROWS = (1, 8, 31, 32, 33, 64, 65, 130, 161, 300)


@pytest.fixture(scope="module")
def env():
    from aznet_hip import ffi
    from oracle import az_oracle as orc
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=0)
    # (an AZ head of the detection head's C: the two heads of a context share C, the map and the pooled rows)
    ctx.load_head(H.int_az_case((LR.DIMS[0], 4, 4, 4), pool=_pool)["head"])
    yield ffi, orc, ctx
    ctx.close()


def _pool(fmap, rois):
    from oracle import az_oracle as orc
    return orc.roi_pool(fmap[0], rois)


def check(tag, got, r64, r32):
    e_dev, e_cpu = R.rel_err(got, r64), R.rel_err(r32, r64)
    b = R.bound(e_cpu)
    print("  %-40s device %.3e   float32-CPU %.3e   bound %.3e   %s" % (tag, e_dev, e_cpu, b, "ok" if e_dev <= b else "EXCEEDS"))
    return e_dev <= b


# ---- 1. the U-stage kernel alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", LR.UNIT_K)
def test_unit_integer_products(K):
    """Y = X W^T + b on integers, with and without ReLU, bit for bit; the entry also checks that the 64 rows behind row M
    of the device buffer are left as they were (AZ_ERR_HIP otherwise)."""
    from aznet_hip import ffi
    ctx = ffi.AzContext(0, max_regions=LR.UNIT_CAP)
    try:
        for N in LR.UNIT_N:
            X, W, b, Y = LR.unit_case(LR.UNIT_CAP, N, K)
            assert (Y < 0).any() and (Y > 0).any()
            for M in LR.UNIT_M + (LR.UNIT_CAP,):
                for relu in (False, True):
                    got = ctx.lowrank_gemm_unit(X, W, b, relu=relu, M=M)
                    want = (np.maximum(Y[:M], 0) if relu else Y[:M]).astype(np.float32)
                    assert got.shape == want.shape and np.array_equal(got, want), (M, N, K, relu, int((got != want).sum()))
    finally:
        ctx.close()


def test_unit_refusals():
    from aznet_hip import ffi
    ctx = ffi.AzContext(0, max_regions=LR.UNIT_CAP)
    try:
        z = lambda *s: np.zeros(s, np.float32)          # noqa: E731
        for M, N, K in ((4, 8, ffi.AZ_LOWRANK_MAX + 4), (4, 8, 6), (4, 8, 0), (4, 6, 8)):
            with pytest.raises(ffi.AzError) as e:
                ctx.lowrank_gemm_unit(z(M, K), z(N, K), z(N))
            assert e.value.code == ffi.AZ_ERR_INVALID, (M, N, K)
        with pytest.raises(ffi.AzError) as e:
            ctx.lowrank_gemm_unit(z(LR.UNIT_CAP + 1, 8), z(8, 8), z(8))
        assert e.value.code == ffi.AZ_ERR_CAPACITY
        # M == 0: a no-op, whatever the pointers
        assert ctx.lowrank_gemm_unit(z(4, 8), z(8, 8), z(8), M=0).shape == (0, 8)
        assert ctx.L.az_lowrank_gemm_unit(ctx.h, None, None, None, 0, 8, 8, 1, None) == ffi.AZ_OK
    finally:
        ctx.close()


# ---- 2. planted exact factorisations --------------------------------------------------------------------------------------------
PLANTED = ((21, 4, 0), (81, 36, 0), (21, 128, 0), (81, 0, 4), (21, 0, 36), (81, 0, 128), (21, 4, 128), (81, 36, 36), (21, 128, 4))


@functools.lru_cache(maxsize=None)
def planted(ncls, r6, r7):
    return LR.planted_head(ncls, r6, r7, pool=_pool)


@pytest.mark.parametrize("case", PLANTED, ids=lambda c: "ncls%d_r6_%d_r7_%d" % c)
def test_planted_factorisation_matches_the_full_head(env, case):
    ffi, orc, ctx = env
    c = planted(*case)
    rois = c["rois"]
    ctx.load_det_head(c["full"])
    ctx.set_feature_map(c["fmap"])
    p_full, b_full = ctx.det_forward(rois)
    assert np.array_equal(b_full, c["bbox"]), "the full head on W = U L"
    ctx.load_det_head_lowrank(c["head"])
    assert (ctx.det_dims["r6"], ctx.det_dims["r7"]) == case[1:]
    p, b = ctx.det_forward(rois)
    assert np.array_equal(b, b_full), "bbox_pred, low rank against the full head: %d elements differ" % int((b != b_full).sum())
    e_lr, e_full = float(np.abs(p - c["p64"]).max()), float(np.abs(p_full - c["p64"]).max())
    print("  planted %s: max |cls_prob - f64| low rank %.3e, full %.3e (k = %d, partial sums <= %.0f)" % (case, e_lr, e_full, c["k"], c["abs_sum"]))
    assert e_lr <= 1e-6 and e_full <= 1e-6
    for n in ROWS:
        pn, bn = ctx.det_forward(rois[:n])
        assert np.array_equal(bn, c["bbox"][:n]) and np.array_equal(pn, p[:n]), n


# ---- 3. random heads ---------------------------------------------------------------------------------------------------------------
RANDOM = ((36, 128), (128, 0), (0, 36))


@functools.lru_cache(maxsize=None)
def rand(r6, r7):
    c = LR.random_case(r6, r7)
    p5 = _pool(c["fmap"], c["rois"])
    c["r64"], c["r32"] = LR.head_on_pool5(c["head"], p5, np.float64), LR.head_on_pool5(c["head"], p5, np.float32)
    return c


def _head_fn(c, dtype, pool=None):
    pool = pool or (lambda rois_u: _pool(c["fmap"], rois_u))
    return lambda index, rois_u: LR.head_on_pool5(c["head"], pool(rois_u), dtype)


@pytest.mark.parametrize("ranks", RANDOM, ids=lambda r: "r6_%d_r7_%d" % r)
def test_random_head_forward_and_detect(env, ranks):
    ffi, orc, ctx = env
    c = rand(*ranks)
    rois, ok = c["rois"], True
    ctx.load_det_head(c["head"])                      # (the dict carries L / U: this goes through the low-rank entry)
    assert (ctx.det_dims["r6"], ctx.det_dims["r7"]) == ranks
    ctx.set_feature_map(c["fmap"])
    ref = ctx.det_forward(rois)
    print("random low-rank head %s" % (ranks,))
    for name, got, r64, r32 in zip(("cls_prob", "bbox_pred"), ref, c["r64"], c["r32"]):
        ok &= check(name, got, r64, r32)
    # a roi's bits: alone, and among 1 ... 300 others
    for n in ROWS:
        for x, y in zip(ctx.det_forward(rois[:n]), ref):
            assert np.array_equal(x, y[:n]), "prefix of the 300-row launch, %d rows" % n
    for j in (0, 63, 64, 137, 299):
        for x, y in zip(ctx.det_forward(rois[j:j + 1]), ref):
            assert np.array_equal(x[0], y[j]), "roi %d alone" % j
    # az_detect: the decoded boxes and the scores of every proposal
    boxes = rois[:, 1:].astype(np.float64)
    im_hw, eps = (H.IM_H, H.IM_W), 1e-14
    s, b = ctx.detect(boxes, 1.0, im_hw[0], im_hw[1], eps=eps)
    s64, b64, _ = D.detect_ref(boxes, [1.0], 1. / 16., 10000, im_hw, eps, _head_fn(c, np.float64))
    s32, b32, _ = D.detect_ref(boxes, [1.0], 1. / 16., 10000, im_hw, eps, _head_fn(c, np.float32))
    ok &= check("az_detect scores", s, s64, s32)
    ok &= check("az_detect boxes", b, b64, b32)
    assert ok, "a tensor exceeds 8 x the float32-CPU error"


def test_detect_batch_is_detect_per_image(env):
    import torch
    from aznet_hip import synth
    ffi, orc, ctx = env
    c = rand(36, 128)
    ctx.load_det_head(c["head"])
    C = LR.DIMS[0]
    sizes = ((24, 32), (19, 25), (12, 40))                      # maps of three images of different sizes
    maps = [synth.make_feature_map(70 + i, C, h, w) for i, (h, w) in enumerate(sizes)]
    ims = [(16 * h, 16 * w) for h, w in sizes]
    rng = np.random.Generator(np.random.PCG64(12))
    boxes = []
    for (ih, iw), n in zip(ims, (300, 37, 130)):
        x1, y1 = rng.uniform(0, iw - 40, n), rng.uniform(0, ih - 40, n)
        boxes.append(np.stack([x1, y1, np.minimum(x1 + rng.uniform(16, iw, n), iw - 1), np.minimum(y1 + rng.uniform(16, ih, n), ih - 1)], 1))
    single = []
    for m, bx, (ih, iw) in zip(maps, boxes, ims):
        ctx.set_feature_map(m)
        single.append(ctx.detect(bx, 1.0, ih, iw))
    got = ctx.detect_batch([torch.from_numpy(m).cuda() for m in maps], boxes, [1.0] * 3, ims)
    for i in range(3):
        assert np.array_equal(got[i][0], single[i][0]) and np.array_equal(got[i][1], single[i][1]), i
    assert np.abs(single[0][1]).max() > 0


def test_detect_pyramid(env):
    import torch
    from aznet_hip import synth
    ffi, orc, ctx = env
    c = rand(36, 128)
    ctx.load_det_head(c["head"])
    C, scales = LR.DIMS[0], (1.0, 2.0)
    im_hw = (H.IM_H // 2, H.IM_W // 2)                           # the blob of scale 2 is 384 x 512: maps of 24 x 32
    maps = np.concatenate([synth.make_feature_map(90 + i, C, H.MAP_H, H.MAP_W) for i in range(2)], 0)
    ctx.set_feature_pyramid([torch.from_numpy(maps[i:i + 1]).cuda().contiguous(memory_format=torch.channels_last) for i in range(2)])
    boxes = c["rois"][:200, 1:].astype(np.float64) / 2.0
    s, b = ctx.detect_pyramid(boxes, scales, im_hw[0], im_hw[1])
    pool = lambda rois_u: PR.pool_pyramid(orc, maps, rois_u)       # noqa: E731
    s64, b64, info = D.detect_ref(boxes, scales, 1. / 16., 10000, im_hw, 1e-14, _head_fn(c, np.float64, pool))
    s32, b32, _ = D.detect_ref(boxes, scales, 1. / 16., 10000, im_hw, 1e-14, _head_fn(c, np.float32, pool))
    assert len(set(info["rois"][:, 0])) == 2, "both levels are used"
    ok = check("az_detect_pyramid scores", s, s64, s32)
    ok &= check("az_detect_pyramid boxes", b, b64, b32)
    assert ok
    ctx.set_feature_map(c["fmap"])                                # (back to a single map for the tests that follow)


def test_detect_skip(env):
    import torch
    from aznet_hip import synth
    ffi, orc, ctx = env
    c = rand(36, 128)
    ctx.load_det_head(c["head"])
    front = synth.make_skip_front(seed=21, Cs=S.SMALL_CS, Cout=LR.DIMS[0])
    ctx.load_skip_front(front)
    maps = S.make_maps(5, S.SMALL_CS)
    ctx.set_skip_maps([torch.from_numpy(m).cuda() for m in maps])
    boxes = S.random_boxes(60, 8)
    im_hw = (S.IM_H, S.IM_W)
    s, b = ctx.detect_skip(boxes, 1.0, im_hw[0], im_hw[1])
    fn = lambda dt: (lambda index, rois_u: LR.head_on_pool5(c["head"], S.pool5(front, maps, rois_u, dt), dt))   # noqa: E731
    s64, b64, _ = D.detect_ref(boxes, [1.0], 1. / 16., 10000, im_hw, 1e-14, fn(np.float64))
    s32, b32, _ = D.detect_ref(boxes, [1.0], 1. / 16., 10000, im_hw, 1e-14, fn(np.float32))
    ok = check("az_detect_skip scores", s, s64, s32)
    ok &= check("az_detect_skip boxes", b, b64, b32)
    assert ok


# ---- 4. load paths -------------------------------------------------------------------------------------------------------------------
def test_full_lowrank_full_and_refusals(env):
    ffi, orc, ctx = env
    c = rand(36, 128)
    full, head, rois = c["uncompressed"], c["head"], c["rois"][:130]
    ctx.load_det_head(full)
    ctx.set_feature_map(c["fmap"])
    first = ctx.det_forward(rois)
    ctx.load_det_head(head)
    low = ctx.det_forward(rois)
    assert not np.array_equal(low[1], first[1]), "rank 36 / 128 of a random head is another model"
    ctx.load_det_head(full)
    for x, y in zip(ctx.det_forward(rois), first):
        assert np.array_equal(x, y), "full -> low rank -> full"
    ctx.load_det_head(head)
    C, n6, n7 = LR.DIMS
    z = lambda *s: np.zeros(s, np.float32)          # noqa: E731

    def zero_head(r6, r7, n6=n6, n7=n7, ncls=21, K6=C * 49):
        h = {"b6": z(n6), "b7": z(n7), "Wc": z(ncls, n7), "bc": z(ncls), "Wb": z(4 * ncls, n7), "bb": z(4 * ncls)}
        h.update({"L6": z(r6, K6), "U6": z(n6, r6)} if r6 else {"W6": z(n6, K6)})
        h.update({"L7": z(r7, n6), "U7": z(n7, r7)} if r7 else {"W7": z(n7, n6)})
        return h

    bad = [zero_head(2, 0), zero_head(6, 0), zero_head(n6 + 4, 0), zero_head(0, 6), zero_head(0, n6 + 4), zero_head(0, n7 + 4, n7=128),
           zero_head(4, 4, n7=n7 + 2), zero_head(4, 4, ncls=1), zero_head(4, 4, ncls=257),
           zero_head(ffi.AZ_LOWRANK_MAX + 4, 0, n6=4096, K6=49 * 64)]
    for h in bad:
        with pytest.raises(ffi.AzError) as e:
            ctx.load_det_head_lowrank(h)
        assert e.value.code == ffi.AZ_ERR_INVALID, {k: v.shape for k, v in h.items()}
        for x, y in zip(ctx.det_forward(rois), low):
            assert np.array_equal(x, y), "a refused load leaves the loaded head answering as before"
    # a rank of 0 needs a NULL L, a rank a non-NULL one
    fp = lambda a: a.ctypes.data_as(ffi.ctypes.POINTER(ffi.ctypes.c_float))     # noqa: E731
    h = zero_head(4, 0)
    args = [fp(h[k]) for k in ("U6", "b6")] + [None] + [fp(h[k]) for k in ("W7", "b7", "Wc", "bc", "Wb", "bb")]
    assert ctx.L.az_load_det_head_lowrank(ctx.h, C, n6, n7, 21, 4, 0, None, *args) == ffi.AZ_ERR_INVALID
    assert ctx.L.az_load_det_head_lowrank(ctx.h, C, n6, n7, 21, 0, 0, fp(h["L6"]), *args) == ffi.AZ_ERR_INVALID
    for x, y in zip(ctx.det_forward(rois), low):
        assert np.array_equal(x, y)
    # both layers at rank 0 through the low-rank entry: the full head's bits
    ctx.load_det_head_lowrank(full)
    for x, y in zip(ctx.det_forward(rois), first):
        assert np.array_equal(x, y), "rank 0 / 0"
    with pytest.raises(ValueError, match="both L6 and U6"):
        ctx.load_det_head_lowrank({k: v for k, v in head.items() if k != "U6"})


@pytest.mark.parametrize("mode", [2, 3])
def test_gemm_modes_refuse_a_lowrank_head(mode):
    from aznet_hip import ffi
    c = rand(36, 128)
    # a context in a 16-bit-term mode: the low-rank load is refused by name and the full head stays loaded
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=mode)
    try:
        ctx.load_head(H.int_az_case((LR.DIMS[0], 4, 4, 4), pool=_pool)["head"])
        ctx.load_det_head(c["uncompressed"])
        ctx.set_feature_map(c["fmap"])
        want = ctx.det_forward(c["rois"][:48])
        with pytest.raises(ffi.AzError) as e:
            ctx.load_det_head(c["head"])
        assert e.value.code == ffi.AZ_ERR_STATE and "fp32 only" in str(e.value)
        for x, y in zip(ctx.det_forward(c["rois"][:48]), want):
            assert np.array_equal(x, y)
    finally:
        ctx.close()
    # a context with a low-rank head loaded: the mode cannot be switched on
    ctx = ffi.AzContext(0, max_regions=512, gemm_mode=0)
    try:
        ctx.load_det_head(c["head"])
        assert ctx.L.az_set_gemm_mode(ctx.h, mode) == ffi.AZ_ERR_STATE
        assert "low-rank" in ctx.L.az_last_error(ctx.h).decode()
        assert ctx.L.az_set_gemm_mode(ctx.h, 0) == ffi.AZ_OK
    finally:
        ctx.close()


# ---- 5. end to end, once ---------------------------------------------------------------------------------------------------------------
def _snapshot_layers(seed=7, width_div=16, n6=260, n7=516, ncls=21):
    """{layer: blobs} of a seeded plain Fast R-CNN snapshot: a VGG16 at 1 / width_div of its width and a reduced head."""
    from aznet_hip import synth
    from aznet_hip.backbone import VGG16Conv5
    bk = VGG16Conv5(device="cpu", seed=seed + 1, width_div=width_div)
    bk.normalize_output(np.ones((1, 3, 600, 800), dtype=np.float32))
    conv = [layer for layer in bk.layers if layer is not None]
    C = int(conv[-1][1].shape[0])
    head = synth.make_det_head(seed=seed, C=C, n6=n6, n7=n7, ncls=ncls)
    layers = {name: [w.numpy(), b.numpy()] for name, w, b in conv}
    for name, w, b in (("fc6", "W6", "b6"), ("fc7", "W7", "b7"), ("cls_score", "Wc", "bc"), ("bbox_pred", "Wb", "bb")):
        layers[name] = [head[w], head[b]]
    return layers, C


def test_compress_net_then_test_det_net(tmp_path):
    import torch
    from aznet_hip import caffemodel as cm
    from datasets.factory import get_imdb
    from detect import config as Cf
    from detect import test as T
    from oracle import az_oracle as orc
    layers, C = _snapshot_layers()
    base = str(tmp_path / "frcnn16.caffemodel")
    cm.write_caffemodel(base, layers)
    sys.path[:0] = [TOOLS]
    try:
        import compress_net
        import test_det_net
    finally:
        sys.path.remove(TOOLS)
    r6, r7 = min(260, C * 49), min(516, 260)                     # full rank: the compressed model is the model
    path = compress_net.main(["--net", base, "--fc6", str(r6), "--fc7", str(r7)])
    assert path == str(tmp_path / ("frcnn16_svd_fc6_%d_fc7_%d.caffemodel" % (r6, r7)))
    imdb = get_imdb("synthetic_375x500_4")
    rng = np.random.Generator(np.random.PCG64(2))
    props = []
    for n in (40, 0, 25, 33):
        x1, y1 = rng.uniform(0, 440, n), rng.uniform(0, 320, n)
        props.append(np.stack([x1, y1, np.minimum(x1 + rng.uniform(20, 400, n), 499), np.minimum(y1 + rng.uniform(20, 300, n), 374)], 1))
    pf = str(tmp_path / "proposals.pkl")
    with open(pf, "wb") as f:
        pickle.dump({"boxes": props, "time": 0.0, "recall": 0}, f)
    exp = "lowrank_test_%d" % os.getpid()
    out_root = os.path.join(Cf.cfg.ROOT_DIR, "output", exp)
    env = dict(os.environ)
    env["AZ_BACKBONE_DETERMINISTIC"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([TOOLS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    old = (torch.backends.cudnn.deterministic, Cf.cfg.EXP_DIR)
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(TOOLS, "test_det_net.py"), "--gpu", "0", "--net", path,
                            "--prop", pf, "--imdb", "synthetic_375x500_4", "--exp", exp], env=env, cwd=REPO, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-3000:]
        assert r.stdout.count("im_detect: ") == 3 and "Applying NMS to all detections" in r.stdout
        df = os.path.join(out_root, "synthetic_375x500_4", os.path.splitext(os.path.basename(path))[0], "detections.pkl")
        with open(df, "rb") as f:
            dets = pickle.load(f)
        assert len(dets) == 21 and sum(dets[j][i].shape[0] for j in range(1, 21) for i in (0, 2, 3)) > 0
        # ... and in this process: the compressed and the uncompressed net on image 0 against the float64 restatement of
        # the compressed model
        torch.backends.cudnn.deterministic = True
        im = imdb.image_at(0)
        head = cm.det_head_from_layers(cm.load_caffemodel(path))
        assert head["L6"].shape == (r6, C * 49) and head["U7"].shape == (516, r7)
        out = {}
        for tag, spec in (("compressed", path), ("uncompressed", base)):
            net = test_det_net.load_frcnn_net(spec, 0)
            assert (net.ctx.det_dims.get("r6", 0), net.ctx.det_dims.get("r7", 0)) == ((r6, r7) if tag == "compressed" else (0, 0))
            out[tag] = T.im_detect({"full": net}, im, props[0], 21)
            if tag == "compressed":
                scale = T._im_scale(im.shape)[0]
                fmap = net.compute_conv(net.image_blob_enqueue(im, Cf.cfg.PIXEL_MEANS, scale)).detach().cpu().contiguous().numpy()
            net.ctx.close()
        fn = lambda dt: (lambda index, rois_u: LR.head_on_pool5(head, orc.roi_pool(fmap[0], rois_u), dt))     # noqa: E731
        args = (props[0], [scale], Cf.cfg.DEDUP_BOXES, Cf.cfg.SEAR.BATCH_SIZE, im.shape[:2], Cf.cfg.EPS)
        s64, b64, _ = D.detect_ref(*args, fn(np.float64))
        s32, b32, _ = D.detect_ref(*args, fn(np.float32))
        ok = True
        for tag in ("compressed", "uncompressed"):
            ok &= check("%s net, scores" % tag, out[tag][0], s64, s32)
            ok &= check("%s net, boxes" % tag, out[tag][1], b64, b32)
        assert ok, "a tensor exceeds 8 x the float32-CPU error against the compressed model in float64"
    finally:
        torch.backends.cudnn.deterministic, Cf.cfg.EXP_DIR = old
        shutil.rmtree(out_root, ignore_errors=True)
