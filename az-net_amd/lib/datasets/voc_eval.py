"""PASCAL VOC detection evaluation: what pascal_voc._do_matlab_eval hands to MATLAB
(VOCdevkit-matlab-wrapper/voc_eval.m -> the devkit's VOCevaldet.m + xVOCap.m), run natively.  The
results files are read back (their rounded values are what the devkit evaluates), the ground truth
comes from the XML annotations, and the ranking / matching / AP of every class runs on the GPU in one
az_voc_eval call.  Prints voc_eval.m's lines and saves <cls>_pr.mat as it does."""
import math
import os
import pickle
import xml.etree.ElementTree as ET

import numpy as np

from aznet_hip import ffi

MIN_OVERLAP = 0.5                   # VOCopts.minoverlap


def read_results_file(path, image_index):
    """A VOC results file ('<id> <conf> <x1> <y1> <x2> <y2>' per line, boxes 1-based) -> (image number [n] int64,
    conf [n] f64, boxes [n,4] f64) in file order.  Vectorised: one split of the whole file."""
    with open(path, "rb") as f:
        tok = f.read().split()
    if len(tok) % 6:
        raise ValueError("%s: not 6 fields per line" % path)
    n = len(tok) // 6
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros((0, 4))
    vals = np.array(tok, dtype=object).reshape(n, 6)
    num = vals[:, 1:].astype(np.bytes_).astype(np.float64)
    ids, inv = np.unique(vals[:, 0].astype(np.bytes_), return_inverse=True)
    where = {k.encode() if isinstance(k, str) else k: i for i, k in enumerate(image_index)}
    try:
        img_of_id = np.array([where[k] for k in ids.tolist()], np.int64)
    except KeyError as e:
        raise ValueError('%s: unrecognized image "%s"' % (path, e.args[0].decode()))
    return img_of_id[inv.ravel()], num[:, 0].copy(), np.ascontiguousarray(num[:, 1:])


def read_record(xml_path):
    """PASreadrecord's objects: [(class name, [x1, y1, x2, y2] 1-based as written, difficult)]; a missing
    <difficult> tag is 0."""
    objs = []
    for obj in ET.parse(xml_path).findall("object"):
        bb = obj.find("bndbox")
        d = obj.find("difficult")
        objs.append((obj.find("name").text.strip(), [float(bb.find(t).text) for t in ("xmin", "ymin", "xmax", "ymax")],
                     int(d.text) if d is not None and d.text and d.text.strip() else 0))
    return objs


def load_records(imdb):
    """Every image's objects of an image set, cached per image set under the devkit's local/VOC<year>/, where
    VOCevaldet keeps its annocachepath."""
    local = os.path.join(imdb._devkit_path, "local", "VOC" + imdb._year)
    if not os.path.isdir(local):
        os.makedirs(local)
    cache = os.path.join(local, imdb._image_set + "_anno.pkl")
    if os.path.exists(cache):
        with open(cache, "rb") as f:
            return pickle.load(f)
    recs = [read_record(os.path.join(imdb._data_path, "Annotations", ix + ".xml")) for ix in imdb.image_index]
    with open(cache, "wb") as f:
        pickle.dump(recs, f, pickle.HIGHEST_PROTOCOL)
    return recs


def gt_segments(classes, recs):
    """Per-class, per-image ground truth in az_voc_eval's class-major layout -> (boxes [G,4], difficult [G], off)."""
    n_img = len(recs)
    buckets = {c: [[] for _ in range(n_img)] for c in classes}
    for i, objs in enumerate(recs):
        for name, box, diff in objs:
            if name in buckets:
                buckets[name][i].append(box + [diff])
    rows, off = [], [0]
    for c in classes:
        for i in range(n_img):
            rows.extend(buckets[c][i])
            off.append(len(rows))
    a = np.array(rows, np.float64).reshape(-1, 5)
    return np.ascontiguousarray(a[:, :4]), a[:, 4].astype(np.uint8), np.array(off, np.int64)


def rounded(dets):
    """('%.3f' score, '%.1f' of x + 1) of [n,5] detections parsed back: the values a results file carries."""
    sc = np.array(["{:.3f}".format(v) for v in dets[:, -1].tolist()], dtype=object).astype(np.bytes_).astype(np.float64)
    b = dets[:, 0:4] + 1
    bx = np.array(["{:.1f}".format(v) for v in b.ravel().tolist()], dtype=object).astype(np.bytes_).astype(np.float64)
    return sc, bx.reshape(-1, 4)


def roidb_records(imdb):
    """load_records' layout from any imdb's gt_roidb: 1-based boxes, difficult taken as 0, background rows left out."""
    roidb = imdb.gt_roidb()
    recs = []
    for i in range(imdb.num_images):
        e = roidb[i]
        recs.append([(imdb.classes[int(k)], [float(v) + 1 for v in b], 0)
                     for b, k in zip(np.asarray(e["boxes"], np.float64), e["gt_classes"]) if int(k) > 0])
    return recs


def all_boxes_dets(imdb, all_boxes):
    """test_net's all_boxes[class][image] ([n,5] or []) -> per class (image number, conf, boxes), rounded as the
    class's results file would hold them and in its order; [] and empty entries are skipped, as the file skips them."""
    dets = []
    for j in range(1, imdb.num_classes):
        img, conf, box = [], [], []
        for i in range(imdb.num_images):
            d = all_boxes[j][i]
            if isinstance(d, list) or d.shape[0] == 0:
                continue
            sc, bx = rounded(np.asarray(d))
            img.append(np.full(sc.size, i, np.int64))
            conf.append(sc)
            box.append(bx)
        dets.append((np.concatenate([np.zeros(0, np.int64)] + img), np.concatenate([np.zeros(0)] + conf),
                     np.vstack([np.zeros((0, 4))] + box)))
    return dets


def det_segments(n_images, dets):
    """dets: per class (image number, conf, boxes) as read_results_file returns them -> (boxes [D,4], conf [D], off) in
    az_voc_eval's class-major layout.  Detections are grouped by image with a stable sort (a results file written by
    image order is unchanged by it)."""
    boxes, confs, off = [], [], [0]
    for img, conf, box in dets:
        o = np.argsort(img, kind="stable")
        boxes.append(box[o])
        confs.append(conf[o])
        off.extend((off[-1] + np.cumsum(np.bincount(img, minlength=n_images)[:n_images])).tolist())
    return np.vstack([np.zeros((0, 4))] + boxes), np.concatenate([np.zeros(0)] + confs), np.array(off, np.int64)


def evaluate(n_images, classes, dets, gt_box, gt_diff, gt_off, metric_07=True, min_overlap=MIN_OVERLAP, ctx=None):
    """dets: per class (image number, conf, boxes) as read_results_file returns them (det_segments lays them out).
    -> az_voc_eval's dict, with per-class slices of rec / prec."""
    det_box, det_conf, det_off = det_segments(n_images, dets)
    if det_off[-1] >= 2 ** 31 or gt_off[-1] >= 2 ** 31:
        raise ffi.AzError(ffi.AZ_ERR_CAPACITY, "voc_eval: more than int32 detections")
    ctx = ctx or ffi.default_context()
    r = ctx.voc_eval(len(classes), n_images, det_box, det_conf, det_off, gt_box, gt_diff, gt_off, min_overlap, metric_07)
    r["class_off"] = det_off[::n_images] if n_images else np.zeros(len(classes) + 1, np.int64)
    return r


def mfmt(spec, x):
    """MATLAB's fprintf of a double: NaN / Inf / -Inf spelled as MATLAB spells them."""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    return spec % x


def report(classes, aps, ap_aucs):
    """voc_eval.m's printed lines: '!!! cls : ap ap_auc' per class, then the results block."""
    lines = ["!!! %s : %s %s" % (c, mfmt("%.4f", a), mfmt("%.4f", u)) for c, a, u in zip(classes, aps, ap_aucs)]
    tail = ["", "~~~~~~~~~~~~~~~~~~~~", "Results:"] + [mfmt("%.1f", a * 100) for a in aps]
    s = 0.0
    for a in aps:
        s += a
    tail += [mfmt("%.1f", s / len(aps) * 100) if len(aps) else "NaN", "~~~~~~~~~~~~~~~~~~~~"]
    return lines, tail


def save_pr(output_dir, cls, rec, prec, ap, ap_auc):
    import scipy.io as sio
    rec = np.asarray(rec, np.float64).reshape(-1, 1) if len(rec) else np.zeros((0, 0))
    prec = np.asarray(prec, np.float64).reshape(-1, 1) if len(prec) else np.zeros((0, 0))
    res = {"recall": rec, "prec": prec, "ap": float(ap), "ap_auc": float(ap_auc)}
    sio.savemat(os.path.join(output_dir, cls + "_pr.mat"),
                {"res": res, "recall": rec, "prec": prec, "ap": float(ap), "ap_auc": float(ap_auc)})


def voc_eval(imdb, comp_id, output_dir, rm_results, ctx=None):
    """voc_eval.m for a pascal_voc imdb whose results files `comp_id` were just written.  Returns (aps, ap_aucs)."""
    classes = [c for c in imdb.classes if c != "__background__"]
    year = int(imdb._year)
    do_eval = year <= 2007 or imdb._image_set != "test"
    paths = [imdb._results_path(comp_id, c) for c in classes]
    aps = np.zeros(len(classes))
    aucs = np.zeros(len(classes))
    curves = [((), ())] * len(classes)
    if do_eval:
        recs = load_records(imdb)
        gb, gd, goff = gt_segments(classes, recs)
        dets = [read_results_file(p, imdb.image_index) for p in paths]
        r = evaluate(imdb.num_images, classes, dets, gb, gd, goff, metric_07=year <= 2007, ctx=ctx)
        aps, aucs = r["ap"], r["ap_auc"]
        co = r["class_off"]
        curves = [(r["rec"][co[k]:co[k + 1]], r["prec"][co[k]:co[k + 1]]) for k in range(len(classes))]
    if not os.path.isdir(output_dir):
        os.makedirs(output_dir)
    lines, tail = report(classes, aps, aucs)
    for k, c in enumerate(classes):
        print(lines[k])
        save_pr(output_dir, c, curves[k][0], curves[k][1], aps[k], aucs[k])
        if rm_results:
            os.remove(paths[k])
    print("\n".join(tail))
    return aps, aucs
