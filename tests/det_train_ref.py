"""A NumPy restatement of the detection net's training data layer (test infrastructure): the box-regression targets of an
image, the per-class statistics over a set and their normalisation, and the sampling of a minibatch.  Written from the
behaviour the issue lists (and checked against tests/golden/g21_train_det.npz, which the reference itself produced), with the
explicit loops that make the ORDER of every float operation visible: that order is what the device code has to reproduce.
`RefBackend` answers roi_data_layer.roidb's two device entry points with these functions, so that the host layers can be
tested without a GPU."""
import numpy as np
import numpy.random as npr

EPS = 1e-14


class DetCfg(object):
    def __init__(self, **kw):
        self.eps, self.bbox_thresh, self.fg_thresh, self.bg_hi, self.bg_lo = EPS, 0.5, 0.5, 0.5, 0.1
        self.batch_size, self.fg_fraction = 128, 0.25
        self.__dict__.update(kw)


def iou_matrix(ex, gt):
    """bbox_overlaps in f64, pair by pair in its operation order: [E, G]."""
    ex, gt = np.asarray(ex, np.float64), np.asarray(gt, np.float64)
    out = np.zeros((ex.shape[0], gt.shape[0]), np.float64)
    for k in range(gt.shape[0]):
        area = (gt[k, 2] - gt[k, 0] + 1) * (gt[k, 3] - gt[k, 1] + 1)
        iw = np.minimum(ex[:, 2], gt[k, 2]) - np.maximum(ex[:, 0], gt[k, 0]) + 1
        ih = np.minimum(ex[:, 3], gt[k, 3]) - np.maximum(ex[:, 1], gt[k, 1]) + 1
        ok = (iw > 0) & (ih > 0)
        ua = (ex[:, 2] - ex[:, 0] + 1) * (ex[:, 3] - ex[:, 1] + 1) + area - iw * ih
        out[ok, k] = (iw * ih / ua)[ok]
    return out


def compute_targets(ex32, gt32, labels, c=None):
    """(targets f32 [E,5], max_overlaps) of one image; max_overlaps is f64, or f32 = BG_THRESH_LO without objects."""
    c = c or DetCfg()
    ex, gt = np.asarray(ex32, np.float32).astype(np.float64), np.asarray(gt32, np.float32).astype(np.float64)
    E = ex.shape[0]
    targets = np.zeros((E, 5), np.float32)
    if gt.shape[0] == 0:
        return targets, c.bg_lo * np.ones(E, np.float32)
    ov = iou_matrix(ex, gt)
    mo = ov.max(axis=1)
    first = ov.argmax(axis=1)                        # the FIRST maximum
    for e in np.where(mo >= c.bbox_thresh)[0]:
        p, t = ex[e], gt[first[e]]
        pw, ph = p[2] - p[0] + c.eps, p[3] - p[1] + c.eps
        pcx, pcy = p[0] + 0.5 * pw, p[1] + 0.5 * ph
        tw, th = t[2] - t[0] + c.eps, t[3] - t[1] + c.eps
        tcx, tcy = t[0] + 0.5 * tw, t[1] + 0.5 * th
        pw, ph, tw, th = max(1.0, pw), max(1.0, ph), max(1.0, tw), max(1.0, th)
        targets[e] = (labels[first[e]], (tcx - pcx) / pw, (tcy - pcy) / ph, np.log(tw / pw), np.log(th / ph))
    return targets, mo


def target_stats(targets_list, num_classes, c=None, normalise=True):
    """(counts [K], means [K,4], stds [K,4]) over the images' un-normalised targets, which are normalised IN PLACE when asked.
    Per image and class: float32 sums of t and of t * t row by row; across the images: float64 in image order."""
    c = c or DetCfg()
    f32 = np.float32
    counts = np.zeros(num_classes, np.float64) + c.eps
    sums = np.zeros((num_classes, 4), np.float64)
    sq = np.zeros((num_classes, 4), np.float64)
    for t in targets_list:
        for cls in range(1, num_classes):
            rows = np.where(t[:, 0] == cls)[0]
            if rows.size == 0:
                continue
            s, q = np.zeros(4, f32), np.zeros(4, f32)
            for r in rows:
                v = t[r, 1:].astype(f32)
                s = (s + v).astype(f32)
                q = (q + (v * v).astype(f32)).astype(f32)
            counts[cls] += rows.size
            sums[cls] += s
            sq[cls] += q
    means = sums / counts[:, None]
    with np.errstate(invalid="ignore"):
        stds = np.sqrt(sq / counts[:, None] - means * means)
    if normalise:
        with np.errstate(divide="ignore", invalid="ignore"):
            for t in targets_list:
                for r in range(t.shape[0]):
                    cls = int(t[r, 0])
                    if cls >= 1 and cls == t[r, 0] and cls < num_classes:
                        a = (t[r, 1:].astype(np.float64) - means[cls]).astype(f32)
                        t[r, 1:] = (a.astype(np.float64) / stds[cls]).astype(f32)
    return counts, means, stds


def flip_boxes(boxes, width):
    out = boxes.copy()
    out[:, 0] = width - boxes[:, 2] - 1
    out[:, 2] = width - boxes[:, 0] - 1
    return out


def expand_targets(compact, num_classes):
    """The 4-of-4K expansion: (bbox_targets, bbox_loss_weights) f32 [n, 4K]."""
    n = compact.shape[0]
    t = np.zeros((n, 4 * num_classes), np.float32)
    w = np.zeros((n, 4 * num_classes), np.float32)
    for r in range(n):
        cls = int(compact[r, 0])
        if cls > 0:
            t[r, 4 * cls:4 * cls + 4] = compact[r, 1:]
            w[r, 4 * cls:4 * cls + 4] = 1.0
    return t, w


def sample_rois(entry, fg_per_image, per_image, num_classes, c=None):
    """One image's share of a minibatch, drawing from np.random what the reference draws, in its order."""
    c = c or DetCfg()
    labels = entry["bbox_targets"][:, 0]
    ov = entry["max_overlaps"]
    fg = np.where(ov >= c.fg_thresh)[0]
    n_fg = int(min(fg_per_image, fg.size))
    if fg.size > 0:
        fg = npr.choice(fg, size=n_fg, replace=False)
    bg = np.where((ov < c.bg_hi) & (ov >= c.bg_lo))[0]
    if bg.size == 0:
        bg = np.where(ov < c.fg_thresh)[0]
    n_bg = int(min(per_image - n_fg, bg.size))
    if bg.size > 0:
        bg = npr.choice(bg, size=n_bg, replace=False)
    keep = np.append(fg, bg).astype(np.int64)
    labels = labels[keep].copy()
    labels[n_fg:] = 0
    t, w = expand_targets(entry["bbox_targets"][keep], num_classes)
    return labels, ov[keep], entry["ex_boxes"].astype(np.float32)[keep], t, w


def minibatch(entries, num_classes, im_scales, n_scales=1, c=None):
    """rois / labels / bbox_targets / bbox_loss_weights of get_minibatch (the image blob aside), as float32."""
    c = c or DetCfg()
    npr.randint(0, high=n_scales, size=len(entries))
    per = c.batch_size // len(entries)
    fg = int(np.round(c.fg_fraction * per))
    rois, labs, tg, lw = [], [], [], []
    for j, e in enumerate(entries):
        l, _, r, t, w = sample_rois(e, fg, per, num_classes, c)
        r = r * im_scales[j]
        rois.append(np.hstack((j * np.ones((r.shape[0], 1)), r)))
        labs.append(l), tg.append(t), lw.append(w)
    return {"rois": np.vstack(rois).astype(np.float32), "labels": np.hstack(labs).astype(np.float32),
            "bbox_targets": np.vstack(tg).astype(np.float32), "bbox_loss_weights": np.vstack(lw).astype(np.float32)}


class RefBackend(object):
    """AzContext's det_targets / det_target_stats answered on the CPU (roi_data_layer.roidb.set_backend)."""

    def det_targets(self, ex_boxes, ex_off, gt_list, label_list, bbox_thresh, bg_thresh_lo, eps):
        c = DetCfg(bbox_thresh=bbox_thresh, bg_lo=bg_thresh_lo, eps=eps)
        ts, ms = [np.zeros((0, 5), np.float32)], [np.zeros(0, np.float64)]
        for i in range(len(gt_list)):
            t, m = compute_targets(ex_boxes[ex_off[i]:ex_off[i + 1]], gt_list[i], label_list[i], c)
            ts.append(t), ms.append(m.astype(np.float64))
        return np.vstack(ts), np.concatenate(ms)

    def det_target_stats(self, targets, ex_off, num_classes, eps, normalise=True):
        views = [targets[ex_off[i]:ex_off[i + 1]] for i in range(len(ex_off) - 1)]
        return target_stats(views, num_classes, DetCfg(eps=eps), normalise)


# ---- synthetic_375x500_8 with flips on the golden's recorded proposals (host and GPU tests) -------------------------------
class FakeNet(object):
    name = "recorded_az_net"

    def __getitem__(self, k):                      # the reference's {'full': net, 'fc': net}
        return self


def synthetic_roidb(rdl, g, tmp_path, monkeypatch, n_images=8):
    """prepare_roidb + add_bbox_regression_targets (rdl = roi_data_layer.roidb, with whatever backend it has) on
    synthetic_375x500_<n> with flips; the proposals of image i are the golden's syn_prop<i>, handed over as the proposals.pkl
    of a net that is never asked.  Returns (imdb, means, stds)."""
    import os
    import pickle
    from datasets.synthetic import SyntheticImdb
    from detect import config
    from detect.train_det import get_training_roidb
    monkeypatch.setattr(config.cfg, "ROOT_DIR", str(tmp_path))
    monkeypatch.setattr(config.cfg, "EXP_DIR", "det_host")
    imdb = SyntheticImdb(375, 500, n_images)
    net = FakeNet()
    out = config.get_output_dir(imdb, net)
    os.makedirs(out)
    with open(os.path.join(out, "proposals.pkl"), "wb") as f:
        pickle.dump([g["syn_prop%d" % i] for i in range(n_images)], f, pickle.HIGHEST_PROTOCOL)
    roidb = get_training_roidb(imdb, {"full": net, "fc": net})
    assert roidb is imdb.roidb and len(roidb) == 2 * n_images
    means, stds = rdl.add_bbox_regression_targets(roidb, imdb.num_classes)
    return imdb, means, stds
