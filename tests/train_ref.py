"""NumPy restatement of the reference's training data layer (lib/az_data_layer/roidb.py, minibatch.py;
lib/utils/bbox.pyx:20-60), test infrastructure shared by the training tests and tests/perf_train_roidb.py.  The noise
is an explicit array of uniform doubles (the reference draws them from np.random inside the level loop); the native
pieces the reference has in Cython (divide_region, bbox_overlaps) are the oracle's C restatements.

  TrainCfg                                the cfg.SEAR / cfg.TRAIN / cfg.EPS keys this path reads
  zoom_labels(rois, gt, ratio, obj)       _compute_zoom_labels (roidb.py:313-341)
  compute_ex_rois(size, gt, noise, c)     _compute_ex_rois (roidb.py:230-299) -> (boxes f64, labels bool, doubles used)
  compute_targets(gt, ex, c)              _compute_targets (roidb.py:146-204) -> [T,7] f64
  target_stats(list of targets, c)        roidb.py:110-134 -> (means [S,4], stds [S,4]); normalises in place
  RefBackend                              the device entry points of aznet_hip.ffi.AzContext, answered by the above
"""
import numpy as np

from oracle import az_oracle as orc

SUBREGION = [[0, 0, 1, 1],
             [-0.5, 0, 0.5, 1], [0.5, 0, 1.5, 1], [0, -0.5, 1, 0.5], [0, 0.5, 1, 1.5],
             [0, 0, 0.5, 1], [0.5, 0, 1, 1], [0, 0, 1, 0.5], [0, 0.5, 1, 1],
             [0.25, 0, 0.75, 1], [0, 0.25, 1, 0.75]]
ADDREGIONS = [[0, 0, 1, 1], [0, 0, 0.8, 0.8], [0, 0.2, 0.8, 1], [0.2, 0, 1, 0.8], [0.2, 0.2, 1, 1]]


class TrainCfg(object):
    def __init__(self, **kw):
        self.min_side = 10
        self.train_rep = 8
        self.zoom_err_prob = 0.3
        self.emb_obj_thresh = 0.5
        self.emb_reg_thresh = 0.25
        self.adj_thresh = 0.1
        self.eps = 1e-14
        self.addregions = ADDREGIONS
        self.subregion = SUBREGION
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


def zoom_labels(rois, gt, max_area_ratio, min_obj):
    rois = np.asarray(rois, dtype=np.float64).reshape(-1, 4)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    if rois.shape[0] == 0 or gt.shape[0] == 0:
        return np.zeros((rois.shape[0],), dtype=bool)
    gt_area = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    rois_area = (rois[:, 2] - rois[:, 0] + 1) * (rois[:, 3] - rois[:, 1] + 1)
    ratio = gt_area[None, :] / (rois_area[:, None] + 1e-14)
    iw = np.minimum(rois[:, None, 2], gt[None, :, 2]) - np.maximum(rois[:, None, 0], gt[None, :, 0]) + 1
    ih = np.minimum(rois[:, None, 3], gt[None, :, 3]) - np.maximum(rois[:, None, 1], gt[None, :, 1]) + 1
    ov = np.where((ratio <= max_area_ratio) & (iw > 0) & (ih > 0), iw * ih / (gt_area[None, :] + 1e-14), 0.0)
    return np.any((ratio <= max_area_ratio) & (ov >= min_obj), axis=1)


def num_levels(size, min_side):
    return int(np.log2(min(size[0], size[1]) / min_side) + 1.0)


def super_regions(ri, subregion):
    rt = np.array(subregion, dtype=np.float64)
    li = np.array([[ri[2] - ri[0] + 1.0, ri[3] - ri[1] + 1.0]])
    lt = np.hstack((rt[:, [2]] - rt[:, [0]], rt[:, [3]] - rt[:, [1]]))
    ls = li / lt
    ts = np.hstack((ri[0] - ls[:, [0]] * rt[:, [0]], ri[1] - ls[:, [1]] * rt[:, [1]]))
    return np.hstack((ts, ts[:, [0]] + ls[:, [0]] - 1, ts[:, [1]] + ls[:, [1]] - 1))


def children_per_parent(Z):
    """3 * num_long - 1 of every parent (div.pyx:32-45), 0 where divide_region makes none."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 4)
    L0, L1 = Z[:, 2] - Z[:, 0] + 1.0, Z[:, 3] - Z[:, 1] + 1.0
    short = np.minimum(L0, L1) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.maximum(L0, L1) / short
    nl = np.where((short > 0) & (q < 1.0e6), np.floor(q), 0).astype(np.int64)
    return np.where(nl > 0, 3 * nl - 1, 0)


def compute_ex_rois(size, gt, noise, c, stats=None):
    """stats (a dict), when given, receives per zoomed level (P, PZ, CH) in `levels` and the parents' indices in `zoomed`,
    the largest CH in `max_children` and the largest child count of one parent in `max_parent`."""
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    noise = np.asarray(noise, dtype=np.float64)
    sel, labs, used = [np.zeros((0, 4))], [np.zeros((0,), dtype=bool)], 0
    w, h = size[1] - 1.0, size[0] - 1.0
    lengths = np.array([[w, h, w, h]])
    K = num_levels(size, c.min_side)
    for _ in range(c.train_rep):
        B = lengths * np.array(c.addregions, dtype=np.float64)
        for _ in range(K):
            z = zoom_labels(B, gt, float(c.emb_reg_thresh), c.emb_obj_thresh)
            sel.append(B)
            labs.append(z)
            if used + B.shape[0] > noise.shape[0]:
                raise IndexError("noise too small: %d needed" % (used + B.shape[0]))
            err = noise[used:used + B.shape[0]] <= c.zoom_err_prob
            used += B.shape[0]
            Z = B[np.logical_xor(z, err)]
            if Z.shape[0] == 0:
                break
            if stats is not None:
                ch = orc.divide_children(Z).shape[0]
                stats["max_children"] = max(stats.get("max_children", 0), ch)
                stats.setdefault("levels", []).append((int(B.shape[0]), int(Z.shape[0]), int(ch)))   # P, PZ, CH
                stats["max_parent"] = max(stats.get("max_parent", 0), int(children_per_parent(Z).max()))
                stats.setdefault("zoomed", []).append(np.where(np.logical_xor(z, err))[0])
            B = orc.divide_region(Z, float(c.min_side))
    for n in range(gt.shape[0]):
        rs = super_regions(gt[n], c.subregion)
        sel.append(rs)
        labs.append(zoom_labels(rs, gt, float(c.emb_reg_thresh), c.emb_obj_thresh))
    B = np.vstack(sel)
    lab = np.hstack(labs)
    B[:, 0] = np.maximum(B[:, 0], 0)
    B[:, 1] = np.maximum(B[:, 1], 0)
    B[:, 2] = np.minimum(B[:, 2], size[1] - 1)
    B[:, 3] = np.minimum(B[:, 3], size[0] - 1)
    sides = np.minimum(B[:, 3] - B[:, 1] + 1, B[:, 2] - B[:, 0] + 1)
    keep = np.where(sides >= c.min_side)[0]
    return B[keep], lab[keep], used


def bbox_deltas(ex, gt, eps):
    ew = np.maximum(1, np.maximum(ex[2] - ex[0], 1) + eps)
    eh = np.maximum(1, np.maximum(ex[3] - ex[1], 1) + eps)
    # (the centres use the widths before the second clamp; the clamp never changes a value >= 1 + eps)
    ecx = ex[0] + 0.5 * (np.maximum(ex[2] - ex[0], 1) + eps)
    ecy = ex[1] + 0.5 * (np.maximum(ex[3] - ex[1], 1) + eps)
    gw = np.maximum(1, np.maximum(gt[2] - gt[0], 1) + eps)
    gh = np.maximum(1, np.maximum(gt[3] - gt[1], 1) + eps)
    gcx = gt[0] + 0.5 * (np.maximum(gt[2] - gt[0], 1) + eps)
    gcy = gt[1] + 0.5 * (np.maximum(gt[3] - gt[1], 1) + eps)
    return [(gcx - ecx) / ew, (gcy - ecy) / eh, np.log(gw / ew), np.log(gh / eh)]


def compute_targets(gt, ex, c, trace=None):
    gt = np.asarray(gt, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    ex = np.asarray(ex, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    K, N = ex.shape[0], gt.shape[0]
    out = []
    if K == 0 or N == 0:
        return np.zeros((0, 7))
    sub = np.array(c.subregion, dtype=np.float64)
    S = sub.shape[0]
    overlaps = orc.bbox_overlaps(ex, gt)
    mx = overlaps.max(axis=1)
    for k in np.where(mx >= c.adj_thresh)[0]:
        re = ex[k]
        L = np.array([[re[2] - re[0], re[3] - re[1], re[2] - re[0], re[3] - re[1]]])
        delta = np.array([[re[0], re[1], re[0], re[1]]])
        ov = orc.bbox_overlaps((L * sub) + delta, gt)
        adj = ov[0] >= c.adj_thresh
        ov[:, ~adj] = -1
        if trace is not None and int(adj.sum()) > S:
            trace["bound"] = trace.get("bound", 0) + 1
        for _ in range(min(S, int(adj.sum()))):
            s, n = np.unravel_index(ov.argmax(), ov.shape)
            if trace is not None:      # (what the golden generators assert their cases reach)
                trace.setdefault("argmax", []).append(int(ov.argmax()))
                trace["zero_rounds"] = trace.get("zero_rounds", 0) + int(ov[s, n] == 0)
                trace["ties"] = trace.get("ties", 0) + int(ov[s, n] > 0 and (ov == ov[s, n]).sum() > 1)
            out.append(bbox_deltas(ex[k], gt[n], c.eps) + [float(k), float(s), overlaps[k, n]])
            ov[s, :] = -1
            ov[:, n] = -1
    return np.array(out, dtype=np.float64).reshape(-1, 7)


def target_stats(targets_list, c, normalise=True):
    S = len(c.subregion)
    counts = np.zeros((S, 1)) + c.eps
    sums = np.zeros((S, 4))
    sq = np.zeros((S, 4))
    for t in targets_list:
        for cls in range(S):
            ix = np.where(t[:, -2] == cls)[0]
            if len(ix) > 0:
                counts[cls] += len(ix)
                sums[cls, :] += t[ix, 0:4].sum(axis=0)
                sq[cls, :] += (t[ix, 0:4] ** 2).sum(axis=0)
    means = sums / counts
    stds = np.sqrt(sq / counts - means ** 2)
    if normalise:
        for t in targets_list:
            for cls in range(S):
                ix = np.where(t[:, -2] == cls)[0]
                t[ix, 0:4] -= means[cls, :]
                t[ix, 0:4] /= stds[cls, :]
    return means, stds


class RefBackend(object):
    """Stands in for aznet_hip.ffi.AzContext on the training entry points (same signatures, same results up to the
    documented tolerances), so the host logic above them runs without a GPU."""

    @staticmethod
    def _cfg(tp):
        return TrainCfg(**tp)

    def zoom_labels(self, rois, gt, max_area_ratio, min_obj):
        return zoom_labels(rois, gt, max_area_ratio, min_obj)

    def train_ex_rois(self, tp, sizes, gt_list, noise, cap=None):
        c = self._cfg(tp)
        ex, zl, off, used, at = [], [], [0], [], 0
        for size, gt in zip(sizes, gt_list):
            try:
                b, z, u = compute_ex_rois(size, gt, noise[at:], c)
            except IndexError:
                from aznet_hip import ffi
                e = ffi.AzError(ffi.AZ_ERR_CAPACITY, "noise too small")
                e.needed = 2 * len(noise) + 1024
                raise e
            at += u
            ex.append(b.astype(np.float32))
            zl.append(z.astype(np.uint8))
            off.append(off[-1] + b.shape[0])
            used.append(u)
        return (np.vstack(ex + [np.zeros((0, 4), np.float32)]), np.hstack(zl + [np.zeros((0,), np.uint8)]),
                np.array(off, dtype=np.int32), np.array(used, dtype=np.int64))

    def train_adj_targets(self, tp, ex_boxes, ex_off, gt_list, cap=None):
        c = self._cfg(tp)
        out, off = [], [0]
        for i, gt in enumerate(gt_list):
            t = compute_targets(gt, ex_boxes[ex_off[i]:ex_off[i + 1]], c)
            out.append(t)
            off.append(off[-1] + t.shape[0])
        return np.vstack(out + [np.zeros((0, 7))]), np.array(off, dtype=np.int32)

    def train_target_stats(self, n_sub, eps, targets, normalise=True):
        c = TrainCfg(eps=eps, subregion=[[0, 0, 1, 1]] * int(n_sub))      # (target_stats reads only its length)
        m, s = target_stats([targets], c, normalise)
        return m, s
