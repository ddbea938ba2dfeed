"""MS COCO image set (reference: lib/datasets/coco.py): the annotation JSON of <devkit>/annotations, image paths
under <devkit>/images, the ground-truth roidb, the results-file writers, and evaluate_detections -- the reference's
pycocotools COCOeval, run natively with box IoU by datasets.coco_eval (az_coco_eval on the GPU).

pycocotools is not used: COCOIndex reads the JSON with the standard library and answers the five queries the
reference makes of it."""
import json
import os

import numpy as np

import datasets
from datasets.imdb import imdb

COCO_CLASSES = ("__background__", "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck",
                "boat", "traffic light", "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog",
                "horse", "sheep", "cow", "elephant", "bear", "zebra", "giraffe", "backpack", "umbrella", "handbag", "tie",
                "suitcase", "frisbee", "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove",
                "skateboard", "surfboard", "tennis racket", "bottle", "wine glass", "cup", "fork", "knife", "spoon",
                "bowl", "banana", "apple", "sandwich", "orange", "broccoli", "carrot", "hot dog", "pizza", "donut",
                "cake", "chair", "couch", "potted plant", "bed", "dining table", "toilet", "tv", "laptop", "mouse",
                "remote", "keyboard", "cell phone", "microwave", "oven", "toaster", "sink", "refrigerator", "book",
                "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush")


class COCOIndex(object):
    """The part of pycocotools.coco.COCO the reference uses.  Images keep the order of the file's `images` array
    (COCO.getImgIds() under Python 3); an image's annotations keep the order of `annotations`."""

    def __init__(self, path):
        with open(path) as f:
            self.dataset = json.load(f)
        self.imgs = {}
        for img in self.dataset.get("images", []):
            self.imgs[img["id"]] = img
        self.anns = {}
        self.img_to_anns = {}
        for ann in self.dataset.get("annotations", []):
            self.anns[ann["id"]] = ann
            self.img_to_anns.setdefault(ann["image_id"], []).append(ann)
        self._cat_ids = sorted(c["id"] for c in self.dataset.get("categories", []))

    def getCatIds(self):
        """Category ids in ascending order."""
        return list(self._cat_ids)

    def getImgIds(self):
        return list(self.imgs.keys())

    def loadImgs(self, ids):
        return [self.imgs[i] for i in (ids if isinstance(ids, (list, tuple)) else [ids])]

    def getAnnIds(self, imgIds=()):
        ids = imgIds if isinstance(imgIds, (list, tuple)) else [imgIds]
        return [a["id"] for i in ids for a in self.img_to_anns.get(i, [])]

    def loadAnns(self, ids):
        return [self.anns[i] for i in (ids if isinstance(ids, (list, tuple)) else [ids])]


def _result_entry(cls_dets, k, index, cat_id):
    # coco.py:_write_coco_results_file's conversion, operation for operation
    x = float(cls_dets[k, 0])
    y = float(cls_dets[k, 1])
    width = float(cls_dets[k, 2] - cls_dets[k, 0] + 1.0)
    height = float(cls_dets[k, 3] - cls_dets[k, 1] + 1.0)
    score = float(cls_dets[k, -1])
    x = int(x * 100) / 100.0
    y = int(y * 100) / 100.0
    width = int(width * 100) / 100.0
    height = int(height * 100) / 100.0
    return {"image_id": index, "category_id": cat_id, "bbox": [x, y, width, height], "score": score}


def _is_empty(dets):
    return isinstance(dets, list) and len(dets) == 0


class coco(imdb):
    def __init__(self, image_set, year, devkit_path=None):
        imdb.__init__(self, "coco_" + year + "_" + image_set)
        self._year = year
        self._image_set = image_set
        self._devkit_path = devkit_path or os.path.join(datasets.ROOT_DIR, "data", "COCO")
        self._data_path = os.path.join(self._devkit_path, "images")
        ann = os.path.join(self._devkit_path, "annotations")
        if image_set == "trainval":
            self._annFile = [os.path.join(ann, "instances_" + s + year + ".json") for s in ("train", "val")]
        elif image_set in ("train", "val"):
            self._annFile = [os.path.join(ann, "instances_" + image_set + year + ".json")]
        else:
            self._annFile = [os.path.join(ann, "image_info_" + image_set + year + ".json")]
        for f in self._annFile:
            if not os.path.exists(f):
                raise KeyError("COCO annotation file does not exist: %s" % f)
        self._coco = [COCOIndex(f) for f in self._annFile]
        self._classes = COCO_CLASSES
        self._class_to_ind = dict(zip(self.classes, range(self.num_classes)))
        self._image_index, self._set_index = self._load_image_set_index()
        self._pos = None
        self.config = {}

    def _load_image_set_index(self):
        img_idx, set_idx = [], []
        for i, c in enumerate(self._coco):
            ids = c.getImgIds()
            img_idx = img_idx + ids
            set_idx = set_idx + [i] * len(ids)
        return img_idx, set_idx

    def _position(self, index):
        """self._image_index.index(index), through a dict of first positions (append_flipped_images keeps them)."""
        if self._pos is None:
            self._pos = {}
            for i, ix in enumerate(self._image_index):
                self._pos.setdefault(ix, i)
        return self._pos[index]

    def image_path_at(self, i):
        return self.image_path_from_index(self._image_index[i])

    def image_path_from_index(self, index):
        set_id = self._set_index[self._position(index)]
        path = os.path.join(self._data_path, self._coco[set_id].loadImgs(index)[0]["file_name"])
        assert os.path.exists(path), "Path does not exist: {}".format(path)
        return path

    def image_size(self, i):
        img = self._coco[self._set_index[i]].loadImgs(self._image_index[i])[0]
        return (img["height"], img["width"])

    # -- ground truth (coco.py:gt_roidb, _load_coco_annotation) ---------------------------------
    def gt_roidb(self):
        return [self._load_coco_annotation(index) for index in self.image_index]

    def _load_coco_annotation(self, index):
        import scipy.sparse
        set_id = self._set_index[self._position(index)]
        anns = self._coco[set_id].loadAnns(self._coco[set_id].getAnnIds(imgIds=index))
        num_objs = len(anns)
        boxes = np.zeros((num_objs, 4), dtype=np.uint16)
        gt_classes = np.zeros((num_objs), dtype=np.int32)
        overlaps = np.zeros((num_objs, self.num_classes), dtype=np.float32)
        img = self._coco[set_id].loadImgs(index)[0]
        height = img["height"]
        width = img["width"]
        cat_ids = self._coco[0].getCatIds()
        for ix in range(num_objs):
            bbox = anns[ix]["bbox"]
            x1 = min(width - 1.0, max(0.0, float(bbox[0])))
            y1 = min(height - 1.0, max(0.0, float(bbox[1])))
            x2 = min(width - 1.0, x1 + max(0.0, float(bbox[2])))
            y2 = min(height - 1.0, y1 + max(0.0, float(bbox[3])))
            cls = cat_ids.index(anns[ix]["category_id"]) + 1
            boxes[ix, :] = [x1, y1, x2, y2]
            gt_classes[ix] = cls
            overlaps[ix, cls] = 1.0
        return {"boxes": boxes, "gt_classes": gt_classes, "gt_overlaps": scipy.sparse.csr_matrix(overlaps),
                "flipped": False}

    def append_flipped_images(self):
        num_images = self.num_images
        widths = [self._coco[self._set_index[i]].loadImgs(self._image_index[i])[0]["width"] for i in range(num_images)]
        for i in range(num_images):
            boxes = self.roidb[i]["boxes"].copy()
            oldx1 = boxes[:, 0].copy()
            oldx2 = boxes[:, 2].copy()
            boxes[:, 0] = widths[i] - oldx2 - 1.0
            boxes[:, 2] = widths[i] - oldx1 - 1.0
            assert (boxes[:, 2] >= boxes[:, 0]).all()
            self.roidb.append({"boxes": boxes, "gt_overlaps": self.roidb[i]["gt_overlaps"],
                               "gt_classes": self.roidb[i]["gt_classes"], "flipped": True})
        self._image_index = self._image_index * 2
        self._set_index = self._set_index * 2

    # -- results files (coco.py:_write_coco_results_file, write_coco_multiple_files) -----------
    def _results_path(self, output_dir, split_id=None):
        tail = "_results.json" if split_id is None else "_results_" + str(split_id) + ".json"
        return os.path.join(output_dir, "instances_" + self._image_set + self._year + tail)

    def _write_coco_results_file(self, all_boxes, output_dir):
        """Every detection, class-major, as COCO results json ([x, y, w, h] truncated to 1/100).  Returns the path."""
        cat_ids = self._coco[0].getCatIds()
        dets = []
        for cls_ind in range(1, len(self.classes)):
            for im_ind, index in enumerate(self.image_index):
                cls_dets = all_boxes[cls_ind][im_ind]
                if not _is_empty(cls_dets):
                    for k in range(cls_dets.shape[0]):
                        dets.append(_result_entry(cls_dets, k, index, cat_ids[cls_ind - 1]))
        filename = self._results_path(output_dir)
        with open(filename, "wt") as f:
            json.dump(dets, f)
        return filename

    def write_coco_multiple_files(self, all_boxes, size, output_dir):
        """The same entries image-major, a new file instances_<set><year>_results_<k>.json every `size` images."""
        cat_ids = self._coco[0].getCatIds()
        dets = []
        split_id = 0
        for im_ind, index in enumerate(self.image_index):
            for cls_ind in range(1, len(self.classes)):
                cls_dets = all_boxes[cls_ind][im_ind]
                if not _is_empty(cls_dets):
                    for k in range(cls_dets.shape[0]):
                        dets.append(_result_entry(cls_dets, k, index, cat_ids[cls_ind - 1]))
            if (im_ind + 1) % size == 0 or im_ind == len(self.image_index) - 1:
                with open(self._results_path(output_dir, split_id), "wt") as f:
                    json.dump(dets, f)
                split_id = split_id + 1
                dets = []

    # -- evaluation (coco.py:_do_coco_eval, evaluate_detections) -------------------------------
    def _do_coco_eval(self, dt_file, output_dir, ctx=None):
        if self._image_set == "train" or self._image_set == "val":
            from datasets import coco_eval
            return coco_eval.evaluate_results_file(self._coco[0], dt_file, ctx=ctx)
        return None

    def evaluate_detections(self, all_boxes, output_dir, ctx=None):
        """Writes the results file (not for trainval) and, for train / val, prints COCOeval's 12 summary lines.
        Returns az_coco_eval's dict (stats, precision, recall) or None."""
        if self._image_set != "trainval":
            if not os.path.isdir(output_dir):
                os.makedirs(output_dir)
            dt_file = self._write_coco_results_file(all_boxes, output_dir)
            return self._do_coco_eval(dt_file, output_dir, ctx=ctx)
        return None

    def competition_mode(self, on):
        pass
