"""Detection over saved proposals on the GPU: az_detect_batch, HipFrcnnNet, detect.test.test_net
(lib/detect/test.py:541-668) and tools/test_det_net.py.

Pinned by tests/golden/g16_test_net.npz -- what the REFERENCE's own test_net printed, pickled and returned per image
for four stub images with seeded conv5_3 maps and the seed-99 small detection head on the CPU
(tests/gen_golden_test_net.py)."""
import ctypes
import io
import os
import pickle
import re
import shutil
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from helpers import load

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "az-net_amd", "tools")


def scrub(text):
    return re.sub(r"\d+\.\d{3}s", "0.000s", text)


@pytest.fixture(scope="module")
def mods():
    import torch
    from aznet_hip import ffi, synth
    from aznet_hip.net import HipFrcnnNet
    return torch, ffi, synth, HipFrcnnNet


@pytest.fixture(scope="module")
def dhead(mods):
    torch, ffi, synth, HipFrcnnNet = mods
    return synth.make_det_head(seed=99, **synth.SMALL_DET_DIMS)


@pytest.fixture(scope="module")
def ctx(mods, dhead):
    torch, ffi, synth, HipFrcnnNet = mods
    # (an AZ head of the same width as well: az_detect, the per-image yardstick, reads the map set_feature_map binds,
    #  which needs one)
    c = ffi.AzContext(0)
    c.load_head(synth.make_head(seed=77, **synth.SMALL_DIMS))
    c.load_det_head(dhead)
    yield c
    c.close()


@pytest.fixture()
def det_cfg():
    from detect import config as C
    old = (C.cfg.SEAR.BATCH_SIZE, C.cfg.EXP_DIR, C.cfg.TEST.get("BATCH_IMAGES", 1))
    C.cfg_set_path("test_net_test")
    yield C
    C.cfg.SEAR.BATCH_SIZE, C.cfg.EXP_DIR, C.cfg.TEST.BATCH_IMAGES = old
    shutil.rmtree(os.path.join(C.cfg.ROOT_DIR, "output", "test_net_test"), ignore_errors=True)


class _MapBackbone(object):
    """Stands where VGG16 would: the seeded conv5_3 (seed + image index) of the image the imdb served, of the size the
    blob gives -- what the golden run's stub 'full' net computed."""

    def __init__(self, torch, synth, seed):
        self.torch, self.synth, self.seed = torch, synth, seed
        self.device = torch.device("cuda", 0)
        self.served = []

    def __call__(self, blob):
        i = self.served.pop(0)
        _, _, bh, bw = blob.shape
        m = self.synth.make_feature_map(self.seed + i, 16, self.synth.conv_out_size(int(bh)), self.synth.conv_out_size(int(bw)))
        return self.torch.from_numpy(m).to(self.device)


def _stub_imdb(g, backbone, synth):
    from datasets.imdb import imdb as imdb_base
    n = int(g["n_img"])

    class Stub(imdb_base):
        def __init__(self):
            imdb_base.__init__(self, "stub_4img")
            self._image_index = list(range(n))
            self._classes = ["c%d" % i for i in range(21)]
            self.read = []

        def image_at(self, i):
            self.read.append(i)
            backbone.served.append(i)
            h, w = (int(x) for x in g["shape%d" % i])
            return synth.make_image(i, h, w)

        def image_path_at(self, i):
            return "synthetic:/%d" % i

        def evaluate_detections(self, nms_dets, output_dir):
            self.nms_dets, self.eval_dir = nms_dets, output_dir
    return Stub()


def _write_props(path, boxes, t=0.25):
    with open(path, "wb") as f:
        pickle.dump({"boxes": boxes, "time": t, "recall": 0}, f, pickle.HIGHEST_PROTOCOL)


def test_test_net_matches_the_reference_run(mods, dhead, det_cfg, tmp_path):
    torch, ffi, synth, HipFrcnnNet = mods
    from detect import test as T
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_test_net_host import net_select_skipping_empty
    C = det_cfg
    g = load("g16_test_net.npz")
    n = int(g["n_img"])
    C.cfg.SEAR.BATCH_SIZE = int(g["batch_size"])
    C.cfg.TEST.BATCH_IMAGES = 1
    bb = _MapBackbone(torch, synth, int(g["map_seed"]))
    net = HipFrcnnNet(dhead, bb, name="frcnn_small")
    imdb = _stub_imdb(g, bb, synth)
    pf = str(tmp_path / "proposals.pkl")
    _write_props(pf, [g["prop%d" % i] for i in range(n)], float(g["prop_time"]))
    rec = {}
    inner = T.im_detect

    def recording(nt, im, boxes, num_classes):
        s, b = inner(nt, im, boxes, num_classes)
        rec[len(rec)] = (s.copy(), b.copy())
        return s, b
    T.im_detect = recording
    try:
        buf = io.StringIO()
        with redirect_stdout(buf):
            nms_dets = T.test_net({"full": net}, pf, imdb)
    finally:
        T.im_detect = inner
    assert scrub(buf.getvalue()) == str(g["stdout"])
    assert imdb.read == [0, 2, 3]                                   # the image without proposals is not read
    det_file = os.path.join(C.get_output_dir(imdb, net), "detections.pkl")
    assert os.path.relpath(det_file, C.cfg.ROOT_DIR) == str(g["relpath"]).replace("/test_net/", "/test_net_test/")
    assert imdb.eval_dir == os.path.dirname(det_file) and imdb.nms_dets is nms_dets
    with open(det_file, "rb") as f:
        all_boxes = pickle.load(f)
    per = []
    for i in range(n):
        if g["prop%d" % i].shape[0] == 0:
            per.append(None)
            continue
        s, b = rec[len([p for p in per if p is not None])]
        assert s.dtype == np.float64 and s.shape == g["scores%d" % i].shape
        np.testing.assert_allclose(s, g["scores%d" % i], rtol=0, atol=1e-4)
        np.testing.assert_allclose(b, g["boxes%d" % i], rtol=1e-4, atol=1e-3)
        per.append((s, b))
    want, _ = net_select_skipping_empty(per, 21)
    for j in range(1, 21):
        for i in range(n):
            if per[i] is None:
                assert all_boxes[j][i] == [] and nms_dets[j][i] == []
                continue
            assert all_boxes[j][i].dtype == np.float32 and np.array_equal(all_boxes[j][i], want[j][i])
            a = nms_dets[j][i]
            assert isinstance(a, list) or (a.dtype == np.float32 and a.shape[1] == 5 and a.shape[0] <= want[j][i].shape[0])
    # (apply_nms itself is the shared path's, unchanged here; on these overhanging, clipped boxes its keep lists were
    #  seen to differ from orc.apply_nms in some (class, image) cells -- not compared here)


# ---- az_detect_batch == az_detect per image ------------------------------------------------------------------------
SHAPES = [(375, 500), (500, 375), (600, 1000), (333, 500), (240, 320)]


def _case(synth, torch, k, shape, nboxes, seed):
    h, w = shape
    scale = 600.0 / min(h, w)
    if round(scale * max(h, w)) > 1000:
        scale = 1000.0 / max(h, w)
    fh, fw = synth.conv_out_size(int(round(h * scale))), synth.conv_out_size(int(round(w * scale)))
    m = torch.from_numpy(synth.make_feature_map(seed, 16, fh, fw)).cuda()
    rng = np.random.RandomState(seed)
    x1 = rng.uniform(-10, w - 20, nboxes)
    y1 = rng.uniform(-10, h - 20, nboxes)
    b = np.stack([x1, y1, x1 + rng.uniform(4, w * 0.7, nboxes), y1 + rng.uniform(4, h * 0.7, nboxes)], 1)
    if nboxes > 8:
        b[-3:] = b[:3]                                              # exact duplicates
        b[-6:-3] = b[3:6] + 0.4                                     # 1/16 duplicates
    return m, np.round(b, 1), scale, (h, w, 3)


def _alone(ctx, m, b, scale, shape, bs):
    if b.shape[0] == 0:
        return np.zeros((0, 21), np.float32), np.zeros((0, 84))
    ctx.set_feature_map(m)
    return ctx.detect(b, scale, shape[0], shape[1], dedup=1. / 16., batch_size=bs, eps=1e-14)


@pytest.mark.parametrize("B", [1, 2, 5, 32])
@pytest.mark.parametrize("bs", [1, 7, 64, 10000])
def test_detect_batch_equals_detect_per_image(mods, ctx, B, bs):
    torch, ffi, synth, HipFrcnnNet = mods
    # (empty images inside the batch, and at both ends of the larger ones)
    counts = [0 if (k % 4 == 3 or (B > 2 and k == B - 1) or (B == 32 and k == 0)) else 40 + 23 * (k % 5) for k in range(B)]
    cases = [_case(synth, torch, k, SHAPES[k % len(SHAPES)], counts[k], 500 + k) for k in range(B)]
    src = 2 if B == 32 else 0
    if B >= 2:                                                      # the same boxes in two images over different maps
        cases[1] = (cases[1][0], cases[src][1].copy(), cases[1][2], cases[1][3])
    want = [_alone(ctx, m, b, s, sh, bs) for m, b, s, sh in cases]
    for order in (list(range(B)), list(range(B))[::-1]):
        got = ctx.detect_batch([cases[k][0] for k in order], [cases[k][1] for k in order], [cases[k][2] for k in order],
                               [cases[k][3] for k in order], dedup=1. / 16., batch_size=bs, eps=1e-14)
        for pos, k in enumerate(order):
            assert np.array_equal(got[pos][0], want[k][0]) and np.array_equal(got[pos][1], want[k][1]), (B, bs, k)


def test_detect_batch_of_only_empty_images(mods, ctx):
    torch, ffi, synth, HipFrcnnNet = mods
    got = ctx.detect_batch([None, None], [np.zeros((0, 4)), np.zeros((0, 4))], [1.6, 1.6], [(375, 500), (375, 500)])
    assert [g[0].shape for g in got] == [(0, 21), (0, 21)] and [g[1].shape for g in got] == [(0, 84), (0, 84)]


@pytest.mark.parametrize("bs", [7, 64])
def test_detect_batch_splits_at_the_region_capacity(mods, ctx, dhead, bs):
    """max_regions=64: batches split at image boundaries, images of more than 64 boxes in pieces of whole chunks."""
    torch, ffi, synth, HipFrcnnNet = mods
    small = ffi.AzContext(0, max_regions=64)
    small.load_det_head(dhead)
    try:
        cases = [_case(synth, torch, k, SHAPES[k % len(SHAPES)], n, 700 + k) for k, n in enumerate([30, 150, 0, 64, 20, 41])]
        want = [_alone(ctx, m, b, s, sh, bs) for m, b, s, sh in cases]
        got = small.detect_batch([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                                 [c[3] for c in cases], batch_size=bs)
        for k in range(len(cases)):
            assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k
        with pytest.raises(ffi.AzError):
            small.detect_batch([cases[1][0]], [cases[1][1]], [cases[1][2]], [cases[1][3]], batch_size=10000)
    finally:
        small.close()


def test_detect_batch_argument_errors_are_synchronous(mods, ctx, dhead):
    torch, ffi, synth, HipFrcnnNet = mods
    L = ctx.L
    m, b, s, sh = _case(synth, torch, 0, (375, 500), 20, 900)
    m = m.contiguous(memory_format=torch.channels_last)
    want = _alone(ctx, m, b, s, sh, 64)
    H, W = int(m.shape[2]), int(m.shape[3])

    def call(c, n=1, maps=(m.data_ptr(),), C=16, off=(0, 20), hs=(H,), ws=(W,)):
        nn = max(n, 1)
        ptrs = (ctypes.c_void_p * max(nn, len(maps)))(*maps)
        arr = lambda v, t: np.ascontiguousarray(np.resize(np.array(v, t), max(nn, len(v))))     # noqa: E731
        o = np.ascontiguousarray(np.resize(np.array(off, np.int32), nn + 1))
        o[:len(off)] = off
        hh, ww = arr(hs, np.int32), arr(ws, np.int32)
        sc, hw = arr([s], np.float64), np.ascontiguousarray(np.resize(np.array([375, 500], np.int32), 2 * nn))
        B = np.ascontiguousarray(np.resize(b, (max(int(o[-1]), 1), 4)))
        S = np.empty((max(int(o[-1]), 1), 21), np.float32)
        D = np.empty((max(int(o[-1]), 1), 84), np.float64)
        p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))   # noqa: E731
        return L.az_detect_batch(c.h, n, ptrs, C, p(hh, ctypes.c_int32), p(ww, ctypes.c_int32), p(B, ctypes.c_double),
                                 p(o, ctypes.c_int32), p(sc, ctypes.c_double), p(hw, ctypes.c_int32), 1. / 16., 64, 1e-14,
                                 p(S, ctypes.c_float), p(D, ctypes.c_double))
    torch.cuda.synchronize()
    assert call(ctx) == ffi.AZ_OK
    assert call(ctx, n=0) == ffi.AZ_ERR_INVALID
    assert call(ctx, n=ffi.AZ_BATCH_MAX + 1) == ffi.AZ_ERR_INVALID
    assert call(ctx, n=2, maps=(m.data_ptr(), m.data_ptr()), off=(0, 20, 10)) == ffi.AZ_ERR_INVALID
    assert call(ctx, maps=(None,)) == ffi.AZ_ERR_INVALID
    assert call(ctx, C=32) == ffi.AZ_ERR_INVALID
    bare = ffi.AzContext(0)
    try:
        assert call(bare) == ffi.AZ_ERR_STATE
    finally:
        bare.close()
    for mode in (2, 3):                     # (the detection head's fc6 on 16-bit terms next to an AZ head: refused)
        c16 = ffi.AzContext(0, gemm_mode=mode)
        try:
            c16.load_head(synth.make_head(seed=77, **synth.SMALL_DIMS))
            c16.load_det_head(dhead)
            assert call(c16) == ffi.AZ_ERR_STATE
        finally:
            c16.close()
    got = ctx.detect_batch([m], [b], [s], [sh], batch_size=64)        # the context still works
    assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[0][1], want[1])


# ---- cfg.TEST.BATCH_IMAGES in test_net ------------------------------------------------------------------------------
def test_test_net_batch_images_give_the_same_detections(mods, dhead, det_cfg, tmp_path):
    torch, ffi, synth, HipFrcnnNet = mods
    from aznet_hip.backbone import VGG16Conv5
    from datasets.synthetic import NpyDirImdb
    from detect import test as T
    C = det_cfg
    C.cfg.SEAR.BATCH_SIZE = 64
    shapes = [(375, 500), (500, 375), (300, 400), (375, 500), (600, 1000), (333, 500), (500, 375), (375, 500), (240, 320),
              (500, 375)]
    d = tmp_path / "ims"
    d.mkdir()
    props = []
    for k, (h, w) in enumerate(shapes):
        np.save(str(d / ("%03d.npy" % k)), synth.make_scene_image(300 + k, h, w))
        props.append(np.zeros((0, 4)) if k == 4 else _case(synth, torch, k, (h, w), 30 + 11 * k, 300 + k)[1])
    pf = str(tmp_path / "proposals.pkl")
    _write_props(pf, props)
    bb = VGG16Conv5(device="cuda:0", seed=5, width_div=32, channels_last_out=True)
    net = HipFrcnnNet(dhead, bb, name="frcnn_narrow")
    runs = {}
    for nb in (1, 3, 8):
        C.cfg.TEST.BATCH_IMAGES = nb
        imdb = NpyDirImdb(str(d))
        buf = io.StringIO()
        with redirect_stdout(buf):
            T.test_net({"full": net}, pf, imdb)
        with open(os.path.join(C.get_output_dir(imdb, net), "detections.pkl"), "rb") as f:
            runs[nb] = (scrub(buf.getvalue()), pickle.load(f))
    assert "im_detect: 5/10" not in runs[1][0] and runs[1][0].count("im_detect:") == 9
    for nb in (3, 8):
        assert runs[nb][0] == runs[1][0]
        for j in range(21):
            for i in range(len(shapes)):
                a, w = runs[nb][1][j][i], runs[1][1][j][i]
                assert (isinstance(a, list) and a == w == []) or np.array_equal(a, w), (nb, j, i)


# ---- the unshared recipe end to end: prop_az.py -> test_det_net.py --------------------------------------------------
def _run_tool(args, timeout=900):
    env = dict(os.environ)
    env["AZ_BACKBONE_DETERMINISTIC"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([TOOLS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(TOOLS, args[0])] + args[1:],
                          env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_unshared_recipe_end_to_end(mods):
    torch, ffi, synth, HipFrcnnNet = mods
    from detect import config as C
    exp = "unshared_test_%d" % os.getpid()
    out_root = os.path.join(C.cfg.ROOT_DIR, "output", exp)
    old = (torch.backends.cudnn.deterministic, C.cfg.EXP_DIR, C.cfg.TEST.get("BATCH_IMAGES", 1))
    try:
        r = _run_tool(["prop_az.py", "--gpu", "0", "--net", "synthetic", "--imdb", "synthetic_600x1000_4", "--tz", "0.5",
                       "--exp", exp])
        assert r.returncode == 0, r.stdout[-3000:]
        pf = os.path.join(out_root, "synthetic_600x1000_4", "vgg16_az_net_synthetic_1234", "proposals.pkl")
        assert os.path.exists(pf), r.stdout[-2000:]
        dets = {}
        for nb in (1, 4):
            r = _run_tool(["test_det_net.py", "--gpu", "0", "--def", "ignored.prototxt", "--net", "synthetic:7",
                           "--prop", pf, "--imdb", "synthetic_600x1000_4", "--exp", exp, "--batch-images", str(nb)])
            assert r.returncode == 0, r.stdout[-3000:]
            out = r.stdout
            assert out.count("im_detect: ") == 4 and "Applying NMS to all detections" in out
            assert "The average time is proposal" in out and "boxes per image are generated" in out
            df = os.path.join(out_root, "synthetic_600x1000_4", "vgg16_frcnn_synthetic_7", "detections.pkl")
            with open(df, "rb") as f:
                dets[nb] = pickle.load(f)
            os.remove(df)
        # ... and in this process
        sys.path.insert(0, TOOLS)
        import test_det_net
        from datasets.factory import get_imdb
        from detect import test as T
        torch.backends.cudnn.deterministic = True
        C.cfg_set_path(exp)
        C.cfg.TEST.BATCH_IMAGES = 1
        net = test_det_net.load_frcnn_net("synthetic:7", 0)
        with redirect_stdout(io.StringIO()):
            T.test_net({"full": net}, pf, get_imdb("synthetic_600x1000_4"))
        with open(df, "rb") as f:
            here = pickle.load(f)
        for j in range(1, 21):
            for i in range(4):
                assert np.array_equal(dets[1][j][i], dets[4][j][i]), (j, i)
                a, w = here[j][i], dets[1][j][i]
                assert a.shape == w.shape and np.allclose(a, w, rtol=1e-4, atol=1e-3), (j, i)
    finally:
        torch.backends.cudnn.deterministic = old[0]
        C.cfg.EXP_DIR, C.cfg.TEST.BATCH_IMAGES = old[1], old[2]
        shutil.rmtree(out_root, ignore_errors=True)
