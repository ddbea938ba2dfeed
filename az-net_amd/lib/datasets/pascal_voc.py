"""PASCAL VOC image set (reference: lib/datasets/pascal_voc.py): the index file, image paths and XML
ground truth of VOCdevkit<year>/VOC<year>, the results files, and evaluate_detections -- the
reference's MATLAB step, run natively by datasets.voc_eval (az_voc_eval on the GPU)."""
import os
import pickle
import xml.etree.ElementTree as ET

import numpy as np

import datasets
from datasets.imdb import imdb

VOC_CLASSES = ("__background__", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat",
               "chair", "cow", "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep",
               "sofa", "train", "tvmonitor")


class pascal_voc(imdb):
    def __init__(self, image_set, year, devkit_path=None):
        imdb.__init__(self, "voc_" + year + "_" + image_set)
        self._year = year
        self._image_set = image_set
        self._devkit_path = devkit_path or os.path.join(datasets.ROOT_DIR, "data", "VOCdevkit" + year)
        self._data_path = os.path.join(self._devkit_path, "VOC" + year)
        self._classes = VOC_CLASSES
        self._class_to_ind = {c: i for i, c in enumerate(VOC_CLASSES)}
        self._image_ext = ".jpg"
        self.config = {"cleanup": True, "use_salt": True}
        if not os.path.isdir(self._data_path):
            raise IOError("VOC data path does not exist: %s" % self._data_path)
        self._image_index = self._read_index()

    def _read_index(self):
        # <devkit>/VOC<year>/ImageSets/Main/<set>.txt: one image id per line
        path = os.path.join(self._data_path, "ImageSets", "Main", self._image_set + ".txt")
        if not os.path.exists(path):
            raise IOError("image set file does not exist: %s" % path)
        with open(path) as f:
            return [line.strip() for line in f if line.strip()]

    def image_path_from_index(self, index):
        path = os.path.join(self._data_path, "JPEGImages", index + self._image_ext)
        if not os.path.exists(path):
            raise IOError("image does not exist: %s" % path)
        return path

    def image_path_at(self, i):
        return self.image_path_from_index(self._image_index[i])

    @property
    def cache_path(self):
        p = os.path.join(datasets.ROOT_DIR, "data", "cache")
        if not os.path.isdir(p):
            os.makedirs(p)
        return p

    def gt_roidb(self, use_cache=True):
        cache = os.path.join(self.cache_path, self.name + "_gt_roidb.pkl") if use_cache else None
        if cache and os.path.exists(cache):
            with open(cache, "rb") as f:
                return pickle.load(f)
        roidb = [self._load_annotation(ix) for ix in self._image_index]
        if cache:
            with open(cache, "wb") as f:
                pickle.dump(roidb, f, pickle.HIGHEST_PROTOCOL)
        return roidb

    def _load_annotation(self, index):
        """One Annotations/<index>.xml -> 0-based uint16 boxes + class ids (pascal_voc.py:106-143;
        every object is kept, 'difficult' ones included, as in the reference)."""
        tree = ET.parse(os.path.join(self._data_path, "Annotations", index + ".xml"))
        objs = tree.findall("object")
        boxes = np.zeros((len(objs), 4), dtype=np.uint16)
        gt_classes = np.zeros((len(objs),), dtype=np.int32)
        for k, obj in enumerate(objs):
            bb = obj.find("bndbox")
            boxes[k, :] = [float(bb.find(t).text) - 1 for t in ("xmin", "ymin", "xmax", "ymax")]
            gt_classes[k] = self._class_to_ind[obj.find("name").text.lower().strip()]
        return {"boxes": boxes, "gt_classes": gt_classes, "flipped": False}

    # -- detection evaluation (pascal_voc.py:145-190) -----------------------------------------
    def _get_comp_id(self):
        return "comp4" + ("-{}".format(os.getpid()) if self.config["use_salt"] else "")

    def _results_path(self, comp_id, cls):
        # VOCdevkit/results/VOC2007/Main/comp4-44503_det_test_aeroplane.txt (VOCopts.detrespath)
        return os.path.join(self._devkit_path, "results", "VOC" + self._year, "Main",
                            comp_id + "_det_" + self._image_set + "_" + cls + ".txt")

    def _write_voc_results_file(self, all_boxes):
        """One results file per class, lines '<id> <score %.3f> <x1+1 %.1f> ...' (the devkit's 1-based
        boxes); [] entries are skipped.  Returns the comp_id."""
        comp_id = self._get_comp_id()
        d = os.path.dirname(self._results_path(comp_id, "x"))
        if not os.path.isdir(d):
            os.makedirs(d)
        for cls_ind, cls in enumerate(self.classes):
            if cls == "__background__":
                continue
            print("Writing {} VOC results file".format(cls))
            parts = []
            for im_ind, index in enumerate(self.image_index):
                dets = all_boxes[cls_ind][im_ind]
                if isinstance(dets, list) and len(dets) == 0:
                    continue
                b = dets[:, 0:4] + 1
                for k in range(dets.shape[0]):
                    parts.append("{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}\n".format(
                        index, dets[k, -1], b[k, 0], b[k, 1], b[k, 2], b[k, 3]))
            with open(self._results_path(comp_id, cls), "wt") as f:
                f.write("".join(parts))
        return comp_id

    def evaluate_detections(self, all_boxes, output_dir, ctx=None):
        from datasets import voc_eval
        comp_id = self._write_voc_results_file(all_boxes)
        return voc_eval.voc_eval(self, comp_id, output_dir, self.config["cleanup"], ctx=ctx)

    def competition_mode(self, on):
        self.config["use_salt"] = not on
        self.config["cleanup"] = not on
