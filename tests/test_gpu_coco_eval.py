"""GPU: az_coco_eval (COCOeval, iouType 'bbox') against the NumPy restatement -- hand cases, 300 seeded random sets,
a val2014-sized set -- its error codes, and coco.evaluate_detections / tools/eval_det.py end to end."""
import json
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

import coco_cases
import coco_eval_ref as R
from coco_cases import CASES

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from aznet_hip import ffi
    return ffi.AzContext(0)


def _run(ctx, c, want_matches=True):
    return ctx.coco_eval(c["n_classes"], c["n_images"], c["det_box"], c["det_score"], c["det_off"], c["gt_box"],
                         c["gt_area"], c["gt_crowd"], c["gt_off"], want_matches=want_matches)


def _ref(c):
    return R.coco_eval(c["n_classes"], c["n_images"], c["det_box"], c["det_score"], c["det_off"], c["gt_box"],
                       c["gt_area"], c["gt_crowd"], c["gt_off"])


def _same(got, ref, what):
    for key in ("precision", "recall", "stats", "dt_match", "dt_ignore"):
        if key not in got:
            continue
        a, b = np.asarray(got[key]), np.asarray(ref[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8) if a.dtype == np.float64 else a,
                              b.view(np.uint8) if b.dtype == np.float64 else b), (what, key)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases_equal_the_restatement(ctx, name):
    _same(_run(ctx, CASES[name]), _ref(CASES[name]), name)


def test_random_sets_equal_the_restatement(ctx):
    for seed in range(300):
        c = coco_cases.random_set(seed)
        _same(_run(ctx, c), _ref(c), "seed %d" % seed)


def _subset(c, cats, n_img):
    """Categories `cats`, images [0, n_img) of a packed set."""
    N = c["n_images"]
    dsl, gsl, doff, goff = [], [], [0], [0]
    for k in cats:
        for i in range(n_img):
            s = k * N + i
            dsl.append(np.arange(c["det_off"][s], c["det_off"][s + 1]))
            gsl.append(np.arange(c["gt_off"][s], c["gt_off"][s + 1]))
            doff.append(doff[-1] + dsl[-1].size)
            goff.append(goff[-1] + gsl[-1].size)
    di, gi = np.concatenate(dsl), np.concatenate(gsl)
    return {"n_classes": len(cats), "n_images": n_img, "det_box": c["det_box"][di], "det_score": c["det_score"][di],
            "det_off": np.array(doff), "gt_box": c["gt_box"][gi], "gt_area": c["gt_area"][gi],
            "gt_crowd": c["gt_crowd"][gi], "gt_off": np.array(goff)}


def test_val2014_sized_set(ctx):
    c = coco_cases.big_set()
    assert c["n_images"] == 40504 and c["n_classes"] == 80
    _run(ctx, c, want_matches=False)                          # warm: arena allocated
    t0 = time.perf_counter()
    r = _run(ctx, c, want_matches=False)
    dt = time.perf_counter() - t0
    print("\nval2014-sized: %d detections, %d boxes, az_coco_eval %.1f ms, stats %s"
          % (c["det_off"][-1], c["gt_off"][-1], dt * 1e3, np.round(r["stats"], 4).tolist()))
    assert ((r["stats"] > 0) & (r["stats"] < 1)).all()
    assert np.array_equal(r["stats"], R.summarize(r["precision"], r["recall"]))
    # a category's result depends on its own segments only: two categories evaluated alone give the same slices
    sub = _subset(c, [3, 41], c["n_images"])
    rs = _run(ctx, sub)
    assert np.array_equal(rs["precision"], r["precision"][:, :, [3, 41]])
    assert np.array_equal(rs["recall"], r["recall"][:, [3, 41]])
    # ... and equal the restatement
    _same(rs, _ref(sub), "val2014, categories 3 and 41")


def test_errors_and_null_outputs(ctx):
    from aznet_hip import ffi
    import ctypes
    L, h = ctx.L, ctx.h
    c = CASES["crowd_twice"]
    stats = np.zeros(12)
    dp = ctypes.POINTER(ctypes.c_double)

    def call(doff, goff, K=1, N=1, stats_p=True, mp=None, ip_=None):
        doff = np.ascontiguousarray(doff, np.int32)
        goff = np.ascontiguousarray(goff, np.int32)
        bx, sc = np.ascontiguousarray(c["det_box"]), np.ascontiguousarray(c["det_score"])
        gb, ga = np.ascontiguousarray(c["gt_box"]), np.ascontiguousarray(c["gt_area"])
        gc = np.ascontiguousarray(c["gt_crowd"])
        return L.az_coco_eval(h, K, N, bx.ctypes.data_as(dp), sc.ctypes.data_as(dp),
                              doff.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), gb.ctypes.data_as(dp),
                              ga.ctypes.data_as(dp), gc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                              goff.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None,
                              stats.ctypes.data_as(dp) if stats_p else None, mp, ip_)

    assert call([0, 3], [0, 2]) == ffi.AZ_OK                   # precision / recall / matches all NULL
    assert np.array_equal(stats, _ref(c)["stats"])
    assert call([1, 3], [0, 2]) == ffi.AZ_ERR_INVALID          # offsets must start at 0
    assert call([0, 3], [0, 2, 1], N=2) == ffi.AZ_ERR_INVALID  # and ascend
    assert call([0, 3], [0, 2], stats_p=False) == ffi.AZ_ERR_INVALID
    m = np.zeros(120, np.int32)
    assert call([0, 3], [0, 2], mp=m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == ffi.AZ_ERR_INVALID
    assert call([0, 3], [0, 2], K=1 << 16, N=1 << 15) == ffi.AZ_ERR_CAPACITY
    with pytest.raises(ffi.AzError):
        ctx.coco_eval(1, 1, c["det_box"], c["det_score"], [0, 2], c["gt_box"], c["gt_area"], c["gt_crowd"], [0, 2])
    # no images: every entry -1
    r = ctx.coco_eval(3, 0, np.zeros((0, 4)), np.zeros(0), [0], np.zeros((0, 4)), np.zeros(0), np.zeros(0), [0])
    assert (r["precision"] == -1).all() and (r["recall"] == -1).all() and (r["stats"] == -1).all()


def _all_boxes(db, seed=5):
    """test_net-style all_boxes (float32 [n,5] or []) near the devkit's ground truth."""
    rng = np.random.RandomState(seed)
    roidb = db.gt_roidb()
    out = [[[] for _ in range(db.num_images)] for _ in range(db.num_classes)]
    for i, e in enumerate(roidb):
        for b, k in zip(e["boxes"].astype(np.float32), e["gt_classes"]):
            d = np.zeros((2, 5), np.float32)
            d[:, :4] = b + rng.normal(0, 2, (2, 4)).astype(np.float32)
            d[:, 2:4] = np.maximum(d[:, 2:4], d[:, 0:2] + 1)
            d[:, 4] = rng.rand(2)
            out[k][i] = d if isinstance(out[k][i], list) else np.vstack([out[k][i], d])
        k = 1 + rng.randint(db.num_classes - 1)
        if isinstance(out[k][i], list):
            out[k][i] = np.array([[5, 5, 60, 70, 0.3]], np.float32)
    return out


def test_evaluate_detections_end_to_end(ctx, tmp_path, capsys):
    from datasets.coco import coco
    from datasets import coco_eval
    devkit = coco_cases.make_devkit(tmp_path)
    db = coco("val", "2014", devkit)
    all_boxes = _all_boxes(db)
    out_dir = str(tmp_path / "out")
    r = db.evaluate_detections(all_boxes, out_dir, ctx=ctx)
    lines = capsys.readouterr().out.splitlines()
    assert lines == coco_eval.summary_lines(r["stats"])
    assert lines[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = ")
    assert lines[11].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = ")
    # the same numbers as the restatement on the results file as written
    res = json.load(open(os.path.join(out_dir, "instances_val2014_results.json")))
    p = coco_eval.pack(db._coco[0], res)
    ref = R.coco_eval(p["n_classes"], p["n_images"], p["det_box"], p["det_score"], p["det_off"], p["gt_box"],
                      p["gt_area"], p["gt_crowd"], p["gt_off"])
    assert np.array_equal(r["stats"], ref["stats"]) and np.array_equal(r["precision"], ref["precision"])
    # trainval: no file, no evaluation; test: the file only
    assert coco("trainval", "2014", devkit).evaluate_detections(all_boxes, str(tmp_path / "tv")) is None
    assert not os.path.exists(str(tmp_path / "tv"))


def test_eval_det_tool_on_a_coco_devkit(tmp_path):
    from datasets.coco import coco
    devkit = coco_cases.make_devkit(tmp_path / "data" / "COCO")
    db = coco("val", "2014", devkit)
    pkl = tmp_path / "detections.pkl"
    with open(str(pkl), "wb") as f:
        pickle.dump(_all_boxes(db), f, pickle.HIGHEST_PROTOCOL)
    # the factory's devkit is <ROOT_DIR>/data/COCO; a fresh process with ROOT_DIR at tmp_path
    tools = os.path.join(REPO, "az-net_amd", "tools")
    code = ("import _init_paths, sys, runpy, datasets; datasets.ROOT_DIR = %r;"
            "sys.argv = ['eval_det.py', %r, '--imdb', 'coco_2014_val', '--no-nms'];"
            "runpy.run_path(%r, run_name='__main__')" % (str(tmp_path), str(pkl), os.path.join(tools, "eval_det.py")))
    out = subprocess.run([sys.executable, "-c", code], cwd=tools, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(" Average")]
    assert len(lines) == 12
    assert os.path.exists(str(tmp_path / "instances_val2014_results.json"))
