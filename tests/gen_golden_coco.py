#!/usr/bin/env python3
"""g18_coco.npz: what the REFERENCE's own lib/datasets/coco.py computes on a fabricated COCO devkit
(tests/coco_cases.fabricate_annotations): _load_coco_annotation for every image, append_flipped_images, and the
parsed JSON that _write_coco_results_file and write_coco_multiple_files write for seeded all_boxes.  The reference
is imported from a temp copy (2to3, an empty `datasets` package, and a stub `pycocotools` whose COCO answers the
five queries coco.py makes the way pycocotools answers them); nothing of it is copied into the repository.

  ann_json                 the instances_val2014.json the devkit holds (bytes)
  image_index, set_index   the imdb's order
  boxes_<i> / classes_<i> / ovl_<i>   roidb entry i: uint16 boxes, gt_classes, gt_overlaps.toarray() (float32)
  fboxes_<i>               roidb entry num_images + i after append_flipped_images
  results                  _write_coco_results_file's file, json.dumps of the parsed list
  multi_<k>                write_coco_multiple_files(size=3): file k, json.dumps of the parsed list
  kinds [C, N]             the input all_boxes[j][i]: 0 = [] (skipped), 1 = array (possibly (0,5))
  boxes_in / boxes_in_off  those arrays, concatenated in (j, i) order, and their offsets

Run:  python tests/gen_golden_coco.py REFERENCE_ROOT    (needs the reference tree)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "g18_coco.npz")
sys.path.insert(0, HERE)

import coco_cases  # noqa: E402


class _OldEq(np.ndarray):
    """An array whose `!= []` is True, as it was under the NumPy the reference was written for."""

    def __ne__(self, other):
        if isinstance(other, list):
            return True
        return np.ndarray.__ne__(self, other)


class _StubCOCO(object):
    """pycocotools.coco.COCO's answers to getCatIds / getImgIds / loadImgs / getAnnIds(imgIds=) / loadAnns."""

    def __init__(self, path):
        d = json.load(open(path))
        self.dataset = d
        self.imgs = {im["id"]: im for im in d["images"]}
        self.anns = {a["id"]: a for a in d.get("annotations", [])}
        self.img_to_anns = {}
        for a in d.get("annotations", []):
            self.img_to_anns.setdefault(a["image_id"], []).append(a)

    def getCatIds(self):
        return [c["id"] for c in self.dataset["categories"]]

    def getImgIds(self):
        return list(self.imgs.keys())

    def loadImgs(self, ids):
        return [self.imgs[i] for i in (ids if isinstance(ids, list) else [ids])]

    def getAnnIds(self, imgIds=[]):
        ids = imgIds if isinstance(imgIds, list) else [imgIds]
        return [a["id"] for i in ids for a in self.img_to_anns.get(i, [])]

    def loadAnns(self, ids):
        return [self.anns[i] for i in (ids if isinstance(ids, list) else [ids])]


def make_all_boxes(n_classes, n_images, seed=18):
    rng = np.random.RandomState(seed)
    all_boxes, kinds = [], []
    for j in range(n_classes):
        row, krow = [], []
        for i in range(n_images):
            r = rng.randint(0, 8)
            if j == 0 or r < 5:
                row.append([])
                krow.append(0)
                continue
            n = 0 if r == 5 else int(rng.randint(1, 5))
            b = np.zeros((n, 5), np.float32)
            if n:
                x1 = rng.uniform(0, 300, n)
                y1 = rng.uniform(0, 300, n)
                b[:, 0] = x1
                b[:, 1] = y1
                b[:, 2] = x1 + rng.uniform(0, 150, n)
                b[:, 3] = y1 + rng.uniform(0, 150, n)
                b[:, 4] = rng.uniform(0, 1, n)
                # values on the int(v * 100) edges: x.005 / x.995, whole hundredths, w = x2 - x1 + 1 exactly whole
                b[0, 0] = np.float32(rng.randint(0, 200)) + np.float32(0.29)
                b[0, 1] = np.float32(rng.randint(0, 200)) + np.float32(0.57)
                b[0, 2] = b[0, 0] + np.float32(9.0)
                b[-1, 3] = b[-1, 1] + np.float32(0.995)
            row.append(b)
            krow.append(1)
        all_boxes.append(row)
        kinds.append(krow)
    return all_boxes, kinds


def main(ref_root):
    tmp = tempfile.mkdtemp(prefix="azcoco_")
    try:
        lib = os.path.join(tmp, "lib")
        os.makedirs(os.path.join(lib, "datasets"))
        files = []
        for f in ("imdb.py", "coco.py"):
            dst = os.path.join(lib, "datasets", f)
            shutil.copy(os.path.join(ref_root, "lib", "datasets", f), dst)
            files.append(dst)
        subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n"] + files,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in files:
            src = open(f).read().expandtabs(8)
            open(f, "w").write(src)
        pkg = types.ModuleType("datasets")
        pkg.__path__ = [os.path.join(lib, "datasets")]
        pkg.ROOT_DIR = tmp
        sys.modules["datasets"] = pkg
        utils = types.ModuleType("utils")
        utils.__path__ = []
        cb = types.ModuleType("utils.cython_bbox")
        cb.bbox_overlaps = None
        sys.modules["utils"] = utils
        sys.modules["utils.cython_bbox"] = cb
        pc = types.ModuleType("pycocotools")
        pc.__path__ = []
        pcc = types.ModuleType("pycocotools.coco")
        pcc.COCO = _StubCOCO
        pce = types.ModuleType("pycocotools.cocoeval")
        pce.COCOeval = None
        sys.modules.update({"pycocotools": pc, "pycocotools.coco": pcc, "pycocotools.cocoeval": pce})
        sys.path.insert(0, lib)
        import datasets.imdb as I
        pkg.imdb = I.imdb
        pkg.coco = None
        import datasets.coco as C
        assert C.__file__.startswith(tmp)

        devkit = coco_cases.make_devkit(os.path.join(tmp, "COCO"))
        d = C.coco("val", "2014", devkit)
        out = {"ann_json": np.frombuffer(open(os.path.join(devkit, "annotations", "instances_val2014.json"), "rb").read(),
                                         np.uint8),
               "image_index": np.array(d.image_index, np.int64), "set_index": np.array(d._set_index, np.int64)}
        n = d.num_images
        d._roidb = d.gt_roidb()
        for i, e in enumerate(d._roidb):
            out["boxes_%d" % i] = e["boxes"]
            out["classes_%d" % i] = e["gt_classes"]
            out["ovl_%d" % i] = e["gt_overlaps"].toarray()
            assert e["flipped"] is False
        d.append_flipped_images()
        assert len(d.roidb) == 2 * n and d.image_index == list(out["image_index"]) * 2
        for i in range(n):
            assert d.roidb[n + i]["flipped"] is True
            out["fboxes_%d" % i] = d.roidb[n + i]["boxes"]
        d2 = C.coco("val", "2014", devkit)
        all_boxes, kinds = make_all_boxes(d2.num_classes, n)
        wrapped = [[b if isinstance(b, list) else b.view(_OldEq) for b in row] for row in all_boxes]
        res_dir = os.path.join(tmp, "res")
        os.makedirs(res_dir)
        fn = d2._write_coco_results_file(wrapped, res_dir)
        assert os.path.basename(fn) == "instances_val2014_results.json"
        out["results"] = np.array(json.dumps(json.load(open(fn))))
        os.remove(fn)
        d2.write_coco_multiple_files(wrapped, 3, res_dir)
        names = sorted(os.listdir(res_dir))
        assert names == ["instances_val2014_results_%d.json" % k for k in range(len(names))], names
        for k, nm in enumerate(names):
            out["multi_%d" % k] = np.array(json.dumps(json.load(open(os.path.join(res_dir, nm)))))
        out["kinds"] = np.array(kinds, np.int8)
        flat = [b for row in all_boxes for b in row]
        out["boxes_in"] = np.vstack([np.zeros((0, 5), np.float32)] + [b for b in flat if not isinstance(b, list)])
        out["boxes_in_off"] = np.concatenate([[0], np.cumsum([0 if isinstance(b, list) else b.shape[0] for b in flat])])
        np.savez_compressed(OUT, **out)
        print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AZ_REFERENCE_ROOT", ""))
