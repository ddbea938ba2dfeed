"""CPU: the COCO imdb (factory names, missing data, the loader, flipped boxes and both results writers against the
reference's own output, g18), tools/coco_submit.py, and the NumPy restatement of COCOeval on hand cases whose
numbers are worked out here."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import coco_cases
import coco_eval_ref as R
from coco_cases import CASES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.spacing(1)
P1 = 1 / (1 + EPS)          # precision of one TP and no FP: tp / (fp + tp + eps)


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_coco.npz"))


def _devkit(tmp, g18):
    root = coco_cases.make_devkit(tmp)
    # the fixture's annotation file is the one the reference read
    assert open(os.path.join(root, "annotations", "instances_val2014.json"), "rb").read() == bytes(g18["ann_json"])
    return root


def _g18_all_boxes(z, n_classes, n_images):
    kinds, bx, off = z["kinds"], z["boxes_in"], z["boxes_in_off"]
    out, f = [], 0
    for j in range(n_classes):
        row = []
        for i in range(n_images):
            row.append(bx[off[f]:off[f + 1]] if kinds[j, i] else [])
            f += 1
        out.append(row)
    return out


def test_factory_names_and_missing_data(tmp_path):
    from datasets.factory import get_imdb, list_imdbs
    names = list_imdbs()
    for n in ("coco_2014_train", "coco_2014_val", "coco_2014_test", "coco_2014_trainval", "coco_2015_test",
              "coco_2015_test-dev"):
        assert n in names
    import datasets
    old = datasets.ROOT_DIR
    try:
        datasets.ROOT_DIR = str(tmp_path)          # no data/COCO here
        for n in ("coco_2014_val", "coco_2014_trainval", "coco_2015_test-dev"):
            with pytest.raises(KeyError) as e:
                get_imdb(n)
            assert "annotations" in str(e.value)
        coco_cases.make_devkit(tmp_path / "data" / "COCO")
        db = get_imdb("coco_2015_test-dev")
        assert db.name == "coco_2015_test-dev" and db.num_images == 3 and db.num_classes == 81
        tv = get_imdb("coco_2014_trainval")
        assert tv.num_images == 4 + 7 and tv._set_index == [0] * 4 + [1] * 7          # train, then val
        assert tv.image_path_at(8).endswith(tv._coco[1].loadImgs(tv.image_index[8])[0]["file_name"])
    finally:
        datasets.ROOT_DIR = old
    with pytest.raises(KeyError):
        get_imdb("coco_2016_val")


def test_loader_matches_the_reference(tmp_path, g18):
    from datasets.coco import coco
    db = coco("val", "2014", _devkit(tmp_path, g18))
    assert db.image_index == [int(v) for v in g18["image_index"]]
    assert db._set_index == [int(v) for v in g18["set_index"]]
    n = db.num_images
    for i, e in enumerate(db.roidb):
        assert e["boxes"].dtype == np.uint16 and np.array_equal(e["boxes"], g18["boxes_%d" % i])
        assert e["gt_classes"].dtype == np.int32 and np.array_equal(e["gt_classes"], g18["classes_%d" % i])
        ovl = e["gt_overlaps"].toarray()
        assert ovl.dtype == np.float32 and np.array_equal(ovl, g18["ovl_%d" % i])
        assert e["flipped"] is False
    # crowd boxes stay in, boxes are clipped to the image
    anns = json.loads(bytes(g18["ann_json"]).decode())["annotations"]
    assert any(a["iscrowd"] for a in anns)
    assert sum(len(e["boxes"]) for e in db.roidb) == len(anns)
    for i in range(n):
        h, w = db.image_size(i)
        assert (db.roidb[i]["boxes"][:, [0, 2]] <= w - 1).all() and (db.roidb[i]["boxes"][:, [1, 3]] <= h - 1).all()
    db.append_flipped_images()
    assert db.num_images == 2 * n and db.image_index[n:] == db.image_index[:n] and db._set_index == [0] * (2 * n)
    for i in range(n):
        e = db.roidb[n + i]
        assert e["flipped"] is True and np.array_equal(e["boxes"], g18["fboxes_%d" % i])
        w = db.image_size(i)[1]
        b = db.roidb[i]["boxes"].astype(np.int64)
        assert np.array_equal(e["boxes"][:, 0], w - b[:, 2] - 1) and np.array_equal(e["boxes"][:, 2], w - b[:, 0] - 1)
    assert db.image_path_at(n + 2) == db.image_path_at(2)
    db.competition_mode(True)                                      # a no-op, as in the reference


def test_writers_match_the_reference(tmp_path, g18):
    from datasets.coco import coco
    db = coco("val", "2014", _devkit(tmp_path, g18))
    all_boxes = _g18_all_boxes(g18, db.num_classes, db.num_images)
    out = tmp_path / "res"
    out.mkdir()
    fn = db._write_coco_results_file(all_boxes, str(out))
    assert os.path.basename(fn) == "instances_val2014_results.json"
    got = json.load(open(fn))
    assert got == json.loads(str(g18["results"]))
    assert any(d["bbox"][2] == 10.0 for d in got)                 # w = x2 - x1 + 1 on a whole number
    os.remove(fn)
    db.write_coco_multiple_files(all_boxes, 3, str(out))
    names = sorted(os.listdir(str(out)))
    multi = sorted(k for k in g18.files if k.startswith("multi_"))
    assert names == ["instances_val2014_results_%d.json" % k for k in range(len(multi))]
    for k in range(len(multi)):
        assert json.load(open(str(out / names[k]))) == json.loads(str(g18["multi_%d" % k]))


def test_coco_submit_splits(tmp_path, g18):
    root = tmp_path / "root"
    _devkit(root / "data" / "COCO", g18)
    from datasets.coco import coco
    db = coco("val", "2014", str(root / "data" / "COCO"))
    pkl = tmp_path / "run" / "detections.pkl"
    pkl.parent.mkdir()
    with open(str(pkl), "wb") as f:
        pickle.dump(_g18_all_boxes(g18, db.num_classes, db.num_images), f, pickle.HIGHEST_PROTOCOL)
    tools = os.path.join(REPO, "az-net_amd", "tools")
    code = ("import _init_paths, sys, runpy, datasets; datasets.ROOT_DIR = %r;"
            "sys.argv = ['coco_submit.py', '--size', '3', '--file', %r, '--split', 'val', '--year', '2014'];"
            "runpy.run_path(%r, run_name='__main__')" % (str(root), str(pkl), os.path.join(tools, "coco_submit.py")))
    p = subprocess.run([sys.executable, "-c", code], cwd=tools, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    names = sorted(n for n in os.listdir(str(pkl.parent)) if n.endswith(".json"))
    assert names == ["instances_val2014_results_%d.json" % k for k in range(3)]     # 7 images by 3
    for k in range(3):
        assert json.load(open(str(pkl.parent / names[k]))) == json.loads(str(g18["multi_%d" % k]))
    p = subprocess.run([sys.executable, os.path.join(tools, "coco_submit.py")], cwd=tools, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 1 and "--size" in p.stdout                               # no arguments: the help


def _ev(name):
    return R.coco_eval(**CASES[name])


def test_iou_exactly_half_and_three_quarters():
    d = CASES["iou_edges"]
    o = R.bb_iou(d["det_box"], d["gt_box"], [0])
    assert o[0, 0] == 0.75 and o[1, 0] == 0.5
    r = _ev("iou_edges")
    # det a (IoU .75) is a TP for t = .5 ... .75 and an FP above; det b (IoU .5) finds the box taken: FP
    assert (r["dt_match"][0, :6, 0] == 0).all() and (r["dt_match"][0, 6:, 0] == -1).all()
    assert (r["dt_match"][0, :, 1] == -1).all()
    assert np.array_equal(r["recall"][:, 0, 0, 2], [1.0] * 6 + [0.0] * 4)
    assert (r["precision"][:6, :, 0, 0, :] == P1).all() and (r["precision"][6:, :, 0, 0, :] == 0).all()
    assert (r["recall"][:, 0, 2:, :] == -1).all()                  # the box is small: no medium / large ground truth
    assert r["stats"][0] == pytest.approx(0.6 * P1, abs=1e-15) and r["stats"][1] == r["stats"][2] == pytest.approx(P1)
    assert r["stats"][4] == r["stats"][5] == -1 and r["stats"][8] == pytest.approx(0.6)


def test_crowd_box_matched_twice():
    r = _ev("crowd_twice")
    assert (r["dt_match"][0, :, 0] == 0).all() and (r["dt_match"][0, :, 1] == 0).all()
    assert (r["dt_ignore"][0, :, :2] == 1).all() and (r["dt_ignore"][0, :, 2] == 0).all()
    # one box counts (npig = 1), matched by the third detection: the two before it are neither TP nor FP
    assert (r["recall"][:, 0, 0, 2] == 1).all() and (r["precision"][:, :, 0, 0, 2] == P1).all()
    # maxDets 1 keeps only the first (ignored) detection: recall 0, precision 0 at every threshold
    assert (r["recall"][:, 0, 0, 0] == 0).all() and (r["precision"][:, :, 0, 0, 0] == 0).all()


def test_plain_box_before_an_ignored_box_of_higher_iou():
    r = _ev("ignored_first")
    # IoU with the plain box 100/120 = .833: matched there up to t = .8; above, the crowd box (IoU 1) takes it
    assert np.array_equal(r["dt_match"][0, :, 0], [1] * 7 + [0] * 3)
    assert np.array_equal(r["dt_ignore"][0, :, 0], [0] * 7 + [1] * 3)
    assert np.array_equal(r["recall"][:, 0, 0, 2], [1.0] * 7 + [0.0] * 3)
    assert (r["precision"][:7, :, 0, 0, 2] == P1).all() and (r["precision"][7:, :, 0, 0, 2] == 0).all()


def test_areas_exactly_32_and_96_squared():
    r = _ev("area_edges")
    # 1024 is small and medium, 9216 medium and large: both boxes count in medium, one each in small and large
    for a, p in ((1, P1), (2, 2 / (2 + EPS)), (3, P1)):         # medium: TP, TP -> the envelope's 2/(2+eps) == 1
        assert (r["recall"][:, 0, a, 2] == 1).all() and (r["precision"][:, :, 0, a, 2] == p).all()
    # in small, the big detection matches the big box, which small ignores; in large the small one likewise
    assert (r["dt_ignore"][1, :, 1] == 1).all() and (r["dt_ignore"][3, :, 0] == 1).all()
    assert (r["dt_ignore"][2, :, :] == 0).all()
    assert r["stats"][6] == 0.5 and r["stats"][7] == 1.0           # AR@1: one of the two boxes


def test_more_than_100_detections():
    r = _ev("over_100")
    d = CASES["over_100"]
    assert d["det_off"][-1] == 120
    # the best-scored detection (file position 110) is the TP; the lowest-scored one, on the second box, is past
    # the first 100 and not evaluated
    assert (r["dt_match"][0, :, 110] == 0).all() and (r["dt_ignore"][:, :, 119] == -1).all()
    assert ((r["dt_ignore"][0] == -1).sum(axis=1) == 20).all()
    assert (r["recall"][:, 0, 0, :] == 0.5).all()
    # recall 0.5 at the first detection (precision 1/(1+eps)); thresholds above 0.5 unreached
    assert (r["precision"][:, :51, 0, 0, :] == P1).all() and (r["precision"][:, 51:, 0, 0, :] == 0).all()


def test_score_ties_across_images():
    r = _ev("tie_images")
    # both score .5: image 0's FP ranks first, then image 1's TP: tp [0, 1], fp [1, 1], rc [0, .5]
    p = 1 / (2 + EPS)
    assert (r["precision"][:, :51, 0, 0, 2] == p).all() and (r["precision"][:, 51:, 0, 0, 2] == 0).all()
    assert (r["recall"][:, 0, 0, 2] == 0.5).all()


def test_category_without_ground_truth():
    r = _ev("no_gt_class")
    assert (r["precision"][:, :, 1] == -1).all() and (r["recall"][:, 1] == -1).all()
    assert (r["precision"][:, :, 0, 0, :] == P1).all()
    assert r["stats"][0] == np.mean(np.full(10 * 101, P1)) and r["stats"][8] == 1.0


def test_detections_on_an_image_without_ground_truth():
    r = _ev("dets_no_gt_image")
    # image 1's detection (.95) is an FP ranked before image 0's TP (.9)
    p = 1 / (2 + EPS)
    assert (r["dt_match"][0, :, 1] == -1).all() and (r["dt_ignore"][0, :, 1] == 0).all()
    assert (r["precision"][:, :, 0, 0, 2] == p).all() and (r["recall"][:, 0, 0, 2] == 1).all()


def test_recall_exactly_on_a_threshold():
    r = _ev("rc_on_threshold")
    # TP, FP, TP over 2 boxes: rc [.5, .5, 1], pr [1/(1+eps), 1/(2+eps), 2/(3+eps)], envelope [1/(1+eps), 2/(3+eps),
    # 2/(3+eps)]; recThrs[50] = 0.5 = rc[0] exactly, so searchsorted('left') gives 0 there
    assert R.REC_THRS[50] == 0.5
    assert (r["precision"][:, :51, 0, 0, 2] == P1).all()
    assert (r["precision"][:, 51:, 0, 0, 2] == 2 / (3 + EPS)).all()
    assert (r["recall"][:, 0, 0, 2] == 1).all() and (r["recall"][:, 0, 0, 0] == 0.5).all()


def test_summary_lines_format():
    from datasets import coco_eval
    lines = coco_eval.summary_lines([0.5, 0.25, -1, 0.125, 0.0, 1.0, 0.1234, 0.2, 0.3, 0.4, 0.5, 0.6])
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.250"
    assert lines[2] == " Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ] = -1.000"
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 0.125"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.123"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 0.600"


def test_pack_follows_load_res(tmp_path):
    from datasets.coco import COCOIndex
    from datasets import coco_eval
    root = coco_cases.make_devkit(tmp_path)
    gt = COCOIndex(os.path.join(root, "annotations", "instances_val2014.json"))
    img = sorted(gt.getImgIds())
    res = [{"image_id": img[2], "category_id": 3, "bbox": [1, 2, 3, 4], "score": .5},
           {"image_id": img[0], "category_id": 999, "bbox": [1, 2, 3, 4], "score": .9},     # not a category: dropped
           {"image_id": img[2], "category_id": 3, "bbox": [5, 6, 7, 8], "score": .7}]
    p = coco_eval.pack(gt, res)
    assert p["n_classes"] == 80 and p["n_images"] == 7 and list(p["img_ids"]) == img
    s = 2 * 7 + 2                                                  # category 3 is the third id
    assert p["det_off"][s] == 0 and p["det_off"][s + 1] == 2 and p["det_off"][-1] == 2
    assert np.array_equal(p["det_box"], [[1, 2, 3, 4], [5, 6, 7, 8]])
    assert p["gt_off"][-1] == len(gt.dataset["annotations"])
    with pytest.raises(ValueError):
        coco_eval.pack(gt, [{"image_id": -5, "category_id": 1, "bbox": [0, 0, 1, 1], "score": 1.0}])
