#!/usr/bin/env python3
"""g17_voc_results.npz: the VOC results files that the REFERENCE's own
pascal_voc._write_voc_results_file (lib/datasets/pascal_voc.py:147-170) writes, with and without
competition_mode, for seeded all_boxes on a fabricated devkit.  The reference is imported from a
temp copy (2to3, an empty `datasets` package so its __init__ does not demand MATLAB, a stub
utils.cython_bbox the writer never calls); nothing of it is copied into the repository.

  names       file names relative to <devkit>/results/VOC2007/Main, competition mode (comp4_...)
  salted      the first file name of a salted run with the pid replaced by {pid}
  body_<k>    bytes of file k of `names`
  boxes_<j>_<i> / kind_<j>_<i>   the input: kind 0 = [] (skipped), 1 = array (possibly (0,5))
  image_index, classes

Run:  python tests/gen_golden_voc.py REFERENCE_ROOT    (needs the reference tree)
"""
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "g17_voc_results.npz")


class _OldEq(np.ndarray):
    """An array whose `== []` is False, as it was under the NumPy the reference was written for
    (NumPy 2 raises on the broadcast instead)."""

    def __eq__(self, other):
        if isinstance(other, list):
            return False
        return np.ndarray.__eq__(self, other)


def make_all_boxes(n_classes, image_index, seed=17):
    rng = np.random.RandomState(seed)
    all_boxes, kinds = [], []
    for j in range(n_classes):
        row, krow = [], []
        for i in range(len(image_index)):
            r = rng.randint(0, 6)
            if j == 0 or r == 0:
                row.append([])
                krow.append(0)
                continue
            n = 0 if r == 1 else int(rng.randint(1, 7))
            b = np.zeros((n, 5), np.float32)
            if n:
                x1 = rng.uniform(0, 300, n)
                y1 = rng.uniform(0, 300, n)
                b[:, 0] = x1
                b[:, 1] = y1
                b[:, 2] = x1 + rng.uniform(5, 150, n)
                b[:, 3] = y1 + rng.uniform(5, 150, n)
                b[:, 4] = rng.uniform(0, 1, n)
                # values on the rounding edges of '%.1f' (x + 1) and '%.3f' (score)
                b[0, 0] = np.float32(rng.randint(0, 200)) + np.float32(0.25)
                b[0, 1] = np.float32(rng.randint(0, 200)) + np.float32(0.15)
                b[-1, 4] = np.float32(rng.randint(0, 1000) / 1000.0 + 0.0005)
                if n > 2:
                    b[1, 4] = np.float32(0.0125)
                    b[2, 2] = np.float32(b[2, 0]) + np.float32(10.05)
            row.append(b)
            krow.append(1)
        all_boxes.append(row)
        kinds.append(krow)
    return all_boxes, kinds


def main(ref_root):
    tmp = tempfile.mkdtemp(prefix="azvoc_")
    try:
        lib = os.path.join(tmp, "lib")
        os.makedirs(os.path.join(lib, "datasets"))
        files = []
        for f in ("imdb.py", "pascal_voc.py"):
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
        pkg.MATLAB = "matlab"
        sys.modules["datasets"] = pkg
        utils = types.ModuleType("utils")
        utils.__path__ = []
        cb = types.ModuleType("utils.cython_bbox")
        cb.bbox_overlaps = None
        sys.modules["utils"] = utils
        sys.modules["utils.cython_bbox"] = cb
        sys.path.insert(0, lib)
        import datasets.imdb as I
        pkg.imdb = I.imdb
        import datasets.pascal_voc as P
        assert P.__file__.startswith(tmp)

        devkit = os.path.join(tmp, "VOCdevkit2007")
        main_dir = os.path.join(devkit, "VOC2007", "ImageSets", "Main")
        os.makedirs(main_dir)
        image_index = ["%06d" % k for k in (1, 4, 5, 12, 33, 70, 101)]
        open(os.path.join(main_dir, "test.txt"), "w").write("\n".join(image_index) + "\n")
        res_dir = os.path.join(devkit, "results", "VOC2007", "Main")
        os.makedirs(res_dir)
        d = P.pascal_voc("test", "2007", devkit)
        all_boxes, kinds = make_all_boxes(d.num_classes, image_index)
        wrapped = [[b if isinstance(b, list) else b.view(_OldEq) for b in row] for row in all_boxes]

        out = {"image_index": np.array(image_index), "classes": np.array(d.classes)}
        d.competition_mode(True)
        comp = d._write_voc_results_file(wrapped)
        names = sorted(os.listdir(res_dir))
        assert all(n.startswith(comp + "_det_test_") for n in names), (comp, names)
        out["names"] = np.array(names)
        for k, n in enumerate(names):
            out["body_%d" % k] = np.frombuffer(open(os.path.join(res_dir, n), "rb").read(), np.uint8)
            os.remove(os.path.join(res_dir, n))
        d.competition_mode(False)
        comp = d._write_voc_results_file(wrapped)
        salted = sorted(os.listdir(res_dir))[0]
        out["salted"] = np.array(salted.replace(str(os.getpid()), "{pid}"))
        for j, row in enumerate(all_boxes):
            for i, b in enumerate(row):
                out["kind_%d_%d" % (j, i)] = np.array(kinds[j][i], np.int8)
                if kinds[j][i]:
                    out["boxes_%d_%d" % (j, i)] = b
        np.savez_compressed(OUT, **out)
        print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AZ_REFERENCE_ROOT", ""))
