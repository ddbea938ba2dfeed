"""GPU: az_voc_eval (imdb.evaluate_detections' VOCevaldet + xVOCap) against the NumPy walk of
tests/voc_eval_ref.py -- hand cases, seeded random sets, a VOC07-sized set -- its error codes, and
pascal_voc.evaluate_detections / tools/eval_det.py end to end on a fabricated devkit."""
import ctypes
import io
import math
import os
import pickle
import subprocess
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import pytest

from voc_cases import CASES
import voc_eval_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    c = ffi.AzContext(0)
    yield c
    c.close()


def _flat_from_case(gts, dets):
    n_img = len(gts)
    det_off = np.zeros(n_img + 1, np.int64)
    for d in dets:
        det_off[d[0] + 1] += 1
    det_off = np.cumsum(det_off)
    order = sorted(range(len(dets)), key=lambda k: dets[k][0])       # stable: file order within an image
    box = np.array([dets[k][2] for k in order], np.float64).reshape(-1, 4)
    conf = np.array([dets[k][1] for k in order], np.float64)
    gb = np.array([g[0] for im in gts for g in im], np.float64).reshape(-1, 4)
    gd = np.array([g[1] for im in gts for g in im], np.uint8)
    goff = np.cumsum([0] + [len(im) for im in gts])
    return 1, n_img, box, conf, det_off, gb, gd, goff


def _check(ctx, args, metric_07=True, rel=1e-12):
    got = ctx.voc_eval(*args, min_overlap=0.5, metric_07=metric_07)
    want = R.evaluate_flat(*args, min_overlap=0.5, metric_07=metric_07)
    assert np.array_equal(got["match"], want["match"])
    assert np.array_equal(got["npos"], want["npos"])
    assert np.array_equal(got["rec"], want["rec"], equal_nan=True)
    assert np.array_equal(got["prec"], want["prec"], equal_nan=True)
    if metric_07:
        assert np.array_equal(got["ap"], want["ap"], equal_nan=True)
    else:
        np.testing.assert_allclose(got["ap"], want["ap"], rtol=rel, atol=0)
    np.testing.assert_allclose(got["ap_auc"], want["ap_auc"], rtol=rel, atol=0)
    return got


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases(ctx, case):
    name, gts, dets, want = case
    got = _check(ctx, _flat_from_case(gts, dets))
    assert got["match"].tolist() == want["match"]
    assert got["ap"][0] == want["ap"]


def _random_set(seed, big=False):
    rng = np.random.RandomState(seed)
    C, N = rng.randint(1, 4), rng.randint(1, 6)
    grid = np.array([[x, y, x + w, y + h] for x in (1.0, 11.0, 21.0) for y in (1.0, 6.0) for w in (9.0, 19.0)
                     for h in (9.0, 4.0)])
    boxes, confs, dcnt, gboxes, gdiff, gcnt = [], [], [], [], [], []
    q = rng.choice([1, 20, 1000])                                     # coarse scores: many ties
    for c in range(C):
        for i in range(N):
            k = rng.randint(0, 9)
            n = rng.randint(0, 30)
            if big and c == 0 and i == 0:
                k, n = 100, 1500                                     # > 64 gt boxes, > 1024 detections
            g = grid[rng.randint(0, len(grid), k)] + rng.randint(0, 3, (k, 1)) * (big * 10.0)
            gboxes.append(g)
            gdiff.append((rng.rand(k) < 0.2).astype(np.uint8))
            gcnt.append(k)
            src = rng.rand(n) < 0.7
            b = np.where(src[:, None] & (k > 0), g[rng.randint(0, max(k, 1), n)] if k else 0,
                         grid[rng.randint(0, len(grid), n)]) + rng.choice([0.0, 0.5, 1.0, 3.0], (n, 4))
            boxes.append(b)
            confs.append(np.round(rng.rand(n) * q) / q)
            dcnt.append(n)
    det_off = np.cumsum([0] + dcnt)
    goff = np.cumsum([0] + gcnt)
    return (C, N, np.vstack(boxes), np.concatenate(confs), det_off, np.vstack([np.zeros((0, 4))] + gboxes),
            np.concatenate(gdiff), goff)


@pytest.mark.parametrize("block", range(6))
def test_random_sets(ctx, block):
    for seed in range(block * 50, block * 50 + 50):
        args = _random_set(seed, big=(seed % 50 == 7))
        _check(ctx, args, metric_07=(seed % 3 != 0))


def test_many_gt_boxes_past_the_register_bits(ctx):
    """A segment of 2100 ground-truth boxes (claims past 2048 live in HBM) and 3000 detections."""
    rng = np.random.RandomState(5)
    G = 2100
    x = rng.randint(0, 4000, G).astype(np.float64)
    g = np.stack([x, x, x + 20, x + 20], 1)
    pick = rng.randint(0, G, 3000)
    b = g[pick] + rng.choice([0.0, 1.0, 8.0], (3000, 1))
    conf = np.round(rng.rand(3000), 2)
    args = (1, 1, b, conf, np.array([0, 3000]), g, (rng.rand(G) < 0.1).astype(np.uint8), np.array([0, G]))
    _check(ctx, args)


def test_voc07_scale(ctx, tmp_path):
    """4952 images x 20 classes, ~40 detections per (image, class): the device against the walk on two classes."""
    rng = np.random.RandomState(2007)
    C, N = 20, 4952
    dcnt = rng.poisson(40, C * N)
    gcnt = rng.poisson(1.2, C * N)
    D, G = int(dcnt.sum()), int(gcnt.sum())
    det_off, goff = np.concatenate([[0], np.cumsum(dcnt)]), np.concatenate([[0], np.cumsum(gcnt)])
    gx = rng.uniform(0, 400, (G, 2))
    gw = rng.uniform(20, 200, (G, 2))
    gb = np.round(np.concatenate([gx, gx + gw], 1), 0) + 1
    gd = (rng.rand(G) < 0.1).astype(np.uint8)
    dx = rng.uniform(0, 400, (D, 2))
    dw = rng.uniform(20, 200, (D, 2))
    db = np.round(np.concatenate([dx, dx + dw], 1), 1) + 1
    seg = np.repeat(np.arange(C * N), dcnt)
    near = (rng.rand(D) < 0.3) & (gcnt[seg] > 0)
    gi = goff[seg[near]] + (rng.rand(int(near.sum())) * gcnt[seg[near]]).astype(np.int64)
    db[near] = np.round(gb[gi] + rng.normal(0, 4, (int(near.sum()), 4)), 1)
    conf = np.round(rng.rand(D), 3)
    args = (C, N, db, conf, det_off, gb, gd, goff)
    ctx.voc_eval(*args)                                                  # warm (scratch grows once)
    t0 = time.perf_counter()
    got = ctx.voc_eval(*args)
    t_dev = time.perf_counter() - t0
    sub = 2
    lo, hi = int(det_off[sub * N]), int(goff[sub * N])
    sargs = (sub, N, db[:lo], conf[:lo], det_off[:sub * N + 1], gb[:hi], gd[:hi], goff[:sub * N + 1])
    t0 = time.perf_counter()
    want = R.evaluate_flat(*sargs)
    t_ref = time.perf_counter() - t0
    # the host side around the call: reading one class's results file (~200k lines)
    path = os.path.join(str(tmp_path), "res.txt")
    lo0, hi0 = int(det_off[0]), int(det_off[N])
    names = ["%06d" % i for i in range(N)]
    with open(path, "w") as f:
        f.write("".join("%s %.3f %.1f %.1f %.1f %.1f\n" % ((names[i], c) + tuple(b)) for i, c, b in
                        zip(seg[lo0:hi0].tolist(), conf[lo0:hi0].tolist(), db[lo0:hi0].tolist())))
    from datasets import voc_eval
    t0 = time.perf_counter()
    voc_eval.read_results_file(path, names)
    t_read = time.perf_counter() - t0
    print("\nreading one class's results file (%d lines): %.3f s" % (hi0 - lo0, t_read))
    print("\nVOC07-sized set: %d detections, %d gt; az_voc_eval %.3f s (whole call); restatement %.1f s for %d of %d "
          "classes" % (D, G, t_dev, t_ref, sub, C))
    assert np.array_equal(got["match"][:lo], want["match"])
    assert np.array_equal(got["rec"][:lo], want["rec"]) and np.array_equal(got["prec"][:lo], want["prec"])
    assert np.array_equal(got["ap"][:sub], want["ap"])
    np.testing.assert_allclose(got["ap_auc"][:sub], want["ap_auc"], rtol=1e-12, atol=0)
    assert np.array_equal(got["npos"], np.array([int((gd[goff[c * N]:goff[(c + 1) * N]] == 0).sum()) for c in range(C)]))


def test_errors_and_null_outputs(ctx):
    from aznet_hip import ffi
    L, h = ctx.L, ctx.h
    dp = ctypes.POINTER(ctypes.c_double)
    box = np.zeros((2, 4))
    conf = np.zeros(2)
    gb = np.zeros((1, 4))
    gd = np.zeros(1, np.uint8)
    npos = np.zeros(1, np.int64)
    ap = np.zeros(1)
    auc = np.zeros(1)

    def call(doff, goff, nc=1, ni=1):
        doff = np.asarray(doff, np.int32)
        goff = np.asarray(goff, np.int32)
        return L.az_voc_eval(h, nc, ni, box.ctypes.data_as(dp), conf.ctypes.data_as(dp),
                             doff.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), gb.ctypes.data_as(dp),
                             gd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                             goff.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 0.5, 1, None, None, None,
                             npos.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ap.ctypes.data_as(dp),
                             auc.ctypes.data_as(dp))
    assert call([0, 2], [0, 1]) == ffi.AZ_OK                           # NULL match / rec / prec
    assert npos[0] == 1 and ap[0] > 0.99 and auc[0] == 1.0              # both boxes on the gt box: TP then FP
    assert call([1, 2], [0, 1]) == ffi.AZ_ERR_INVALID                  # does not start at 0
    assert call([0, 2, 1], [0, 1, 1], ni=2) == ffi.AZ_ERR_INVALID      # descends
    assert call([0, 2], [0, 1], nc=-1) == ffi.AZ_ERR_INVALID
    assert call([0, 2], [0, 1], nc=65536, ni=65536) == ffi.AZ_ERR_CAPACITY
    assert call([0, 2], [0, 1]) == ffi.AZ_OK                           # the context is still usable


def _fabricated_voc(root, n_img=5, seed=3):
    from PIL import Image
    rng = np.random.RandomState(seed)
    dk = os.path.join(root, "VOCdevkit2007")
    v = os.path.join(dk, "VOC2007")
    for sub in ("ImageSets/Main", "Annotations", "JPEGImages"):
        os.makedirs(os.path.join(v, sub))
    index = ["%06d" % (k * 3 + 1) for k in range(n_img)]
    open(os.path.join(v, "ImageSets/Main/test.txt"), "w").write("\n".join(index) + "\n")
    classes = ["dog", "cat", "person", "car"]
    gts = []
    for ix in index:
        Image.fromarray(rng.randint(0, 255, (120, 160, 3), dtype=np.uint8)).save(os.path.join(v, "JPEGImages", ix + ".jpg"))
        objs = []
        xml = ["<annotation>"]
        for k in range(rng.randint(1, 5)):
            x1, y1 = rng.randint(1, 100), rng.randint(1, 70)
            b = [x1, y1, x1 + rng.randint(10, 60), y1 + rng.randint(10, 50)]
            cls = classes[rng.randint(0, len(classes))]
            diff = int(rng.rand() < 0.25)
            tag = "" if k == 0 else "<difficult>%d</difficult>" % diff
            diff = 0 if k == 0 else diff
            xml.append("<object><name>%s</name>%s<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax>"
                       "</bndbox></object>" % (cls, tag, b[0], b[1], b[2], b[3]))
            objs.append((cls, b, diff))
        xml.append("</annotation>")
        open(os.path.join(v, "Annotations", ix + ".xml"), "w").write("".join(xml))
        gts.append(objs)
    return dk, index, gts


def _all_boxes(d, gts, seed=4):
    rng = np.random.RandomState(seed)
    out = [[[] for _ in d.image_index] for _ in d.classes]
    for j, cls in enumerate(d.classes):
        if j == 0:
            continue
        for i, objs in enumerate(gts):
            mine = [o for o in objs if o[0] == cls]
            n = rng.randint(0, 4) + 2 * len(mine)
            if n == 0:
                continue
            b = np.zeros((n, 5), np.float32)
            for k in range(n):
                if k < 2 * len(mine):
                    g = np.array(mine[k // 2][1], np.float32) - 1 + rng.normal(0, 3, 4).astype(np.float32)
                else:
                    x, y = rng.uniform(0, 100, 2)
                    g = np.array([x, y, x + 30, y + 20], np.float32)
                b[k, :4] = g
                b[k, 4] = rng.rand()
            out[j][i] = b
    return out


def test_evaluate_detections_end_to_end(ctx, tmp_path):
    import scipy.io as sio
    from datasets import voc_eval
    from datasets.pascal_voc import pascal_voc
    dk, index, gts = _fabricated_voc(str(tmp_path))
    d = pascal_voc("test", "2007", dk)
    all_boxes = _all_boxes(d, gts)
    out_dir = str(tmp_path / "out")
    res = os.path.join(dk, "results", "VOC2007", "Main")
    # competition mode first: the results files stay, so the APs can be checked against the walk over them
    d.competition_mode(True)
    buf = io.StringIO()
    with redirect_stdout(buf):
        aps, aucs = d.evaluate_detections(all_boxes, out_dir, ctx=ctx)
    text = buf.getvalue()
    classes = [c for c in d.classes if c != "__background__"]
    recs = [voc_eval.read_record(os.path.join(dk, "VOC2007", "Annotations", ix + ".xml")) for ix in index]
    for k, cls in enumerate(classes):
        img, conf, box = voc_eval.read_results_file(os.path.join(res, "comp4_det_test_%s.txt" % cls), index)
        gb = [np.array([o[1] for o in r if o[0] == cls], np.float64).reshape(-1, 4) for r in recs]
        gd = [np.array([o[2] for o in r if o[0] == cls], bool) for r in recs]
        w = R.evaldet(img, conf, box, gb, gd)
        assert aps[k] == w["ap"] or (math.isnan(aps[k]) and math.isnan(w["ap"])), cls
        assert aucs[k] == pytest.approx(w["ap_auc"], rel=1e-12, nan_ok=True), cls
        m = sio.loadmat(os.path.join(out_dir, cls + "_pr.mat"))
        assert float(m["ap"].ravel()[0]) == aps[k] or math.isnan(aps[k])
        assert np.array_equal(m["recall"].ravel(), w["rec"], equal_nan=True)
        assert "res" in m
    lines, tail = voc_eval.report(classes, aps, aucs)
    want = "\n".join(lines) + "\n" + "\n".join(tail) + "\n"
    assert want in text
    assert "!!! dog : " in text and "Results:" in text
    assert len(os.listdir(res)) == len(classes)                         # kept under competition_mode(True)
    for f in os.listdir(res):
        os.remove(os.path.join(res, f))
    d.competition_mode(False)
    with redirect_stdout(io.StringIO()):
        aps2, _ = d.evaluate_detections(all_boxes, out_dir, ctx=ctx)
    assert np.array_equal(aps2, aps, equal_nan=True)
    assert os.listdir(res) == []                                        # cleaned up by default
    # tools/eval_det.py on the same detections (saved as test_net saves them), without NMS
    det = tmp_path / "detections.pkl"
    with open(det, "wb") as f:
        pickle.dump(all_boxes, f, pickle.HIGHEST_PROTOCOL)
    env = dict(os.environ)
    code = ("import _init_paths, sys, datasets.factory as F; from datasets.pascal_voc import pascal_voc;"
            "F._makers['voc_2007_test'] = lambda: pascal_voc('test', '2007', %r);"
            "sys.argv = ['eval_det.py', %r, '--no-nms', '--out', %r];"
            "import runpy; runpy.run_path(%r, run_name='__main__')"
            % (dk, str(det), str(tmp_path / "out2"), os.path.join(REPO, "az-net_amd", "tools", "eval_det.py")))
    p = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(REPO, "az-net_amd", "tools"), env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "\n".join(lines) in p.stdout and "\n".join(tail) in p.stdout
    assert os.path.exists(tmp_path / "out2" / "dog_pr.mat")
