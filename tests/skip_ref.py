"""NumPy restatement of the skip-connection detector's front (models/COCO/VGG16_skip/frcnn/test_fc.prototxt) and of the
detection head behind it; the yardstick of tests/test_skip_host.py and tests/test_gpu_skip.py (test infrastructure).

    roi_pool3/4/5   Caffe ROIPooling 7x7 of conv3_3 / conv4_3 / conv5_3 at spatial_scale 1/4, 1/8, 1/16 (train_step_ref.roi_pool:
                    the arithmetic of the oracle's RoIPool with the scale and the map size as parameters)
    roi_norm3/4/5   GRN, as this project defines it: y[c] = x[c] / sqrt(sum_c x[c]^2 + eps) per roi, bin and source
    concat5, scale5 the three blocks side by side, times `gain`
    conv_pool5      1x1 convolution sum Cs -> Cout with bias, relu_pool; then fc6 .. cls_prob / bbox_pred

Every stage exists in float64 (on the exact float32 pooled values) and in float32 (each operation rounded to float32, the
sums by NumPy); tolerances are train_step_ref.bound of the float32 figure: 8 x its error against float64, floor 1e-6.
Rows of the concatenated blob are (roi, bin): row = roi * 49 + ph * 7 + pw, as the device holds them."""
import numpy as np

import train_step_ref as R

SCALES = (0.25, 0.125, 0.0625)
NAMES = ("conv3_3", "conv4_3", "conv5_3")
FULL_CS = (256, 512, 512)
SMALL_CS = (20, 36, 12)          # no source a multiple of the wave width
IM_H, IM_W = 96, 128             # scaled pixels: maps of 24 x 32, 12 x 16 and 6 x 8 cells
MAP_HW = ((24, 32), (12, 16), (6, 8))


def restore_tree(dst, src):
    """dst (an EasyDict tree such as detect.config.cfg) back to the deep copy `src`, in place: other modules hold
    references into it."""
    for k in list(dst.keys()):
        if k not in src:
            del dst[k]
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            restore_tree(dst[k], v)
        else:
            dst[k] = v


def skip_model_layers(seed=7, width_div=16, n6=260, n7=516, num_classes=21):
    """{layer name: [blobs]} of a seeded skip Fast R-CNN model as a .caffemodel holds it: conv1_1 .. conv5_3 of a VGG16 at
    1 / width_div of its width (conv5_3 rescaled to unit RMS on a constant blob), conv_pool5, fc6, fc7, cls_score,
    bbox_pred."""
    from aznet_hip import synth
    from aznet_hip.backbone import VGG16Conv5
    bk = VGG16Conv5(device="cpu", seed=seed + 1, width_div=width_div)
    bk.normalize_output(np.ones((1, 3, IM_H, IM_W), dtype=np.float32))
    conv = {layer[0]: layer for layer in bk.layers if layer is not None}
    Cs = tuple(int(conv[n][1].shape[0]) for n in NAMES)
    head = synth.make_det_head(seed=seed, C=Cs[2], n6=n6, n7=n7, ncls=num_classes)
    front = synth.make_skip_front(seed=seed + 2, Cs=Cs, Cout=Cs[2])
    layers = {name: [w.numpy(), b.numpy()] for name, w, b in conv.values()}
    layers["conv_pool5"] = [front["Wp"].reshape(Cs[2], sum(Cs), 1, 1), front["bp"]]
    for name, w, b in (("fc6", "W6", "b6"), ("fc7", "W7", "b7"), ("cls_score", "Wc", "bc"), ("bbox_pred", "Wb", "bb")):
        layers[name] = [head[w], head[b]]
    return layers


def make_maps(seed, Cs, zero=()):
    """Post-ReLU-like maps [1, C, H, W] f32 (~half zeros); the sources listed in `zero` are all-zero (what an all-negative
    pre-ReLU map is stored as)."""
    from aznet_hip import synth
    maps = [synth.make_feature_map(seed + 17 * i, C, h, w) for i, (C, (h, w)) in enumerate(zip(Cs, MAP_HW))]
    for i in zero:
        maps[i][:] = 0.0
    return maps


def hostile_rois():
    """[R, 5] f32 rois in scaled pixels of the 96 x 128 image: outside the map, negative corners, zero area, one cell, the
    whole map, bins that are empty at 1/16 but not at 1/4, x2 < x1 -- and a few ordinary ones."""
    r = [
        (300.0, 200.0, 420.0, 260.0),      # wholly outside (right / below)
        (-90.0, -70.0, -20.0, -10.0),      # wholly outside (negative)
        (-30.5, -12.25, 40.0, 33.0),       # negative corner, partly inside
        (50.0, 40.0, 50.0, 40.0),          # zero area
        (17.0, 9.0, 18.0, 10.0),           # one cell at every scale
        (0.0, 0.0, 127.0, 95.0),           # the whole map
        (0.0, 0.0, 200.0, 150.0),          # the whole map and beyond
        (116.0, 84.0, 140.0, 110.0),       # 1/16: bins past the map's edge are empty; 1/4: they are not
        (100.0, 70.0, 163.0, 133.0),       # the same with a longer overhang
        (80.0, 30.0, 20.0, 60.0),          # x2 < x1
        (30.0, 80.0, 90.0, 10.0),          # y2 < y1
        (5.5, 6.5, 77.5, 41.5),            # ties in roundf
        (33.0, 21.0, 64.0, 52.0),
        (2.0, 3.0, 125.0, 12.0),           # a flat strip
        (60.0, 1.0, 66.0, 94.0),           # a tall strip
    ]
    a = np.zeros((len(r), 5), np.float32)
    a[:, 1:] = np.asarray(r, np.float32)
    return a


def random_rois(n, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    x1 = rng.uniform(0, IM_W - 12, n)
    y1 = rng.uniform(0, IM_H - 12, n)
    x2 = np.minimum(x1 + rng.uniform(4, 0.9 * IM_W, n), IM_W - 1)
    y2 = np.minimum(y1 + rng.uniform(4, 0.9 * IM_H, n), IM_H - 1)
    return np.stack([np.zeros(n), x1, y1, x2, y2], 1).astype(np.float32)


def random_boxes(n, seed=4, scale=1.0):
    """[n, 4] f64 proposals in ORIGINAL image pixels of an image whose scaled size is 96 x 128."""
    return random_rois(n, seed)[:, 1:].astype(np.float64) / scale


def roi_pool(fmap, rois, spatial_scale):
    """ROIPooling 7x7 of one map [1, C, H, W] -> [R, 49, C] f32 (bin-major, as the device holds pool5)."""
    p = R.roi_pool(fmap, rois, spatial_scale)[0]
    Rn, C = rois.shape[0], fmap.shape[1]
    return np.ascontiguousarray(p.reshape(Rn, C, 49).transpose(0, 2, 1))


def pooled_blocks(maps, rois, scales=SCALES):
    return [roi_pool(m, rois, s) for m, s in zip(maps, scales)]


def cat_raw(maps, rois, scales=SCALES):
    """The raw maxima side by side, [R * 49, sum Cs] f32."""
    return np.concatenate(pooled_blocks(maps, rois, scales), axis=2).reshape(rois.shape[0] * 49, -1)


def grn(x, eps, dtype):
    """y[c] = x[c] / sqrt(sum_c x[c]^2 + eps) along the last axis, every operation in `dtype`."""
    x = np.asarray(x, dtype)
    ss = (x * x).sum(axis=-1, keepdims=True, dtype=dtype)
    return (x / np.sqrt(ss + dtype(eps))).astype(dtype)


def cat_norm(maps, rois, gain=1000.0, eps=1e-10, dtype=np.float64, scales=SCALES):
    """concat5 after scale5, [R * 49, sum Cs] in `dtype`."""
    blocks = [grn(b, eps, dtype) * dtype(gain) for b in pooled_blocks(maps, rois, scales)]
    return np.concatenate(blocks, axis=2).reshape(rois.shape[0] * 49, -1).astype(dtype)


def conv1x1(cat, Wp, bp, dtype):
    """relu(cat . Wp^T + bp), [rows, Cout] in `dtype`."""
    Wp = np.asarray(Wp).reshape(np.asarray(Wp).shape[0], -1)
    y = np.asarray(cat, dtype) @ Wp.astype(dtype).T + np.asarray(bp, dtype)
    return np.maximum(y, 0).astype(dtype)


def pool5(front, maps, rois, dtype):
    """The `pool5` blob [R, Cout, 7, 7] flattened Caffe's way ([R, Cout * 49], column c * 49 + p) in `dtype`."""
    y = conv1x1(cat_norm(maps, rois, front.get("gain", 1000.0), front.get("eps", 1e-10), dtype, front["scales"]),
                front["Wp"], front["bp"], dtype)
    Rn, Cout = rois.shape[0], y.shape[1]
    return np.ascontiguousarray(y.reshape(Rn, 49, Cout).transpose(0, 2, 1)).reshape(Rn, Cout * 49)


def _fc(x, W, b, relu, dtype, block=512):
    """InnerProduct in `dtype`, the weight rows converted a block at a time (the full-size W6 is 411 MB in float32)."""
    x = np.asarray(x, dtype)
    y = np.empty((x.shape[0], W.shape[0]), dtype)
    for o in range(0, W.shape[0], block):
        y[:, o:o + block] = x @ W[o:o + block].astype(dtype).T
    y += np.asarray(b, dtype)
    return np.maximum(y, 0) if relu else y


def det_head(head, p5, dtype):
    """(cls_prob, bbox_pred) of fc6 -> fc7 -> {cls_score + Softmax, bbox_pred} on pooled rows [R, C * 49] in `dtype`
    (float32: Caffe's Softmax as the oracle states it)."""
    h7 = _fc(_fc(p5, head["W6"], head["b6"], True, dtype), head["W7"], head["b7"], True, dtype)
    s = _fc(h7, head["Wc"], head["bc"], False, dtype)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True, dtype=dtype)).astype(dtype), _fc(h7, head["Wb"], head["bb"], False, dtype)


def det_forward(front, head, maps, rois, dtype):
    return det_head(head, pool5(front, maps, rois, dtype), dtype)


class SkipOracleNet(object):
    """pycaffe-shaped skip Fast R-CNN net for the oracle's _frcnn_forward (oracle.az_oracle.frcnn_forward, which hands
    every entry of its `conv` dict to forward as a keyword): forward(rois=, conv3_3=, conv4_3=, conv5_3=)."""

    class _Blob(object):
        def reshape(self, *shape):
            self.shape = shape

    def __init__(self, front, head, dtype=np.float32, names=NAMES):
        self.front, self.head, self.dtype, self.names = front, head, dtype, names
        self.blobs = {k: SkipOracleNet._Blob() for k in ("data", "rois") + tuple(names)}
        self.name = "skip_oracle"

    def forward(self, blobs=None, **kw):
        maps = [np.asarray(kw[n], np.float32) for n in self.names]
        p, b = det_forward(self.front, self.head, maps, np.asarray(kw["rois"], np.float32), self.dtype)
        return {"cls_prob": p, "bbox_pred": b}


def detect(orc, front, head, maps, boxes, scale, im_shape, dedup, dtype, names=NAMES, batch_size=10000, eps=1e-14):
    """_frcnn_forward (lib/detect/test.py:259-318) with the skip net, through the oracle's line-by-line restatement:
    (scores [P, ncls], boxes [P, 4 * ncls])."""
    class Cfg(object):
        BATCH_SIZE = batch_size
        DEDUP_BOXES = dedup
        EPS = eps
    net = SkipOracleNet(front, head, dtype, names)
    conv = {n: m for n, m in zip(names, maps)}
    return orc.frcnn_forward({"fc": net}, im_shape, scale, boxes, head["Wc"].shape[0], conv, Cfg)


# ---- the configurations of tests/test_skip_edges_host.py and tests/test_gpu_skip_edges.py ----------------------------------------
# channel sets of the pool kernels' quad partition (nqb = min(256, quads left), G = 256 / nqb): one quad (G = 256), 130 (G = 1,
# idle lanes), 256 (one full pass), 257 (a second pass of one quad), 300 (a second pass of 44: G = 5), 1024 (four passes, the
# cap AZ_SKIP_MAX_SUMC) and three regimes side by side at non-zero offsets
CHANNEL_SETS = ((4,), (520,), (1024,), (1028,), (1200,), (4096,), (1028, 4, 520))
# one and two sources, scales that are no power of two on maps of odd width, maps that are not image * scale
SOURCE_CASES = {
    "one": dict(Cs=(20,), scales=(0.0625,), hw=((6, 8),)),
    "two": dict(Cs=(36, 12), scales=(0.125, 0.0625), hw=((12, 16), (6, 8))),
    "odd": dict(Cs=SMALL_CS, scales=(0.5, 0.3, 1.0 / 32.0), hw=((48, 64), (29, 39), (3, 4))),
    "tiny": dict(Cs=SMALL_CS, scales=SCALES, hw=((5, 9), (1, 16), (1, 1))),
}


def geometry(Cs):
    """(scales, map sizes) of a channel set: a single source is conv5_3's 6 x 8 map at 1/16."""
    return ((SCALES[2],), (MAP_HW[2],)) if len(Cs) == 1 else (SCALES[:len(Cs)], MAP_HW[:len(Cs)])


def tie_map(seed, C, h, w, N=1):
    """[N, C, h, w] f32 of values drawn from {0, 1, 2, 3}, about half of them zeroed: every window holds ties (which fall in
    different cell groups and, past 1024 channels, in both passes of the pool kernels), and every sum of squares is a whole
    number."""
    rng = np.random.Generator(np.random.PCG64(20_000 + seed))
    return (rng.integers(0, 4, (N, C, h, w)) * (rng.random((N, C, h, w)) < 0.5)).astype(np.float32)


def perm_map(seed, C, h, w, N=1):
    """[N, C, h, w] f32: per image and channel a permutation of 1 .. h * w (no two cells equal)."""
    rng = np.random.Generator(np.random.PCG64(21_000 + seed))
    return np.stack([np.stack([rng.permutation(h * w) + 1 for _ in range(C)]) for _ in range(N)]).reshape(N, C, h, w).astype(np.float32)


def edge_maps(kind, seed, Cs, hw, N=1):
    """kind "relu": synth.make_feature_map per source and image (make_maps' and skip_train_ref.make_batch_maps' seeds);
    "ties": tie_map; "perm": perm_map."""
    from aznet_hip import synth
    if kind == "relu":
        return [np.concatenate([synth.make_feature_map(seed + 17 * i + 101 * n, C, h, w) for n in range(N)], axis=0)
                for i, (C, (h, w)) in enumerate(zip(Cs, hw))]
    f = {"ties": tie_map, "perm": perm_map}[kind]
    return [f(seed + 17 * i, C, h, w, N) for i, (C, (h, w)) in enumerate(zip(Cs, hw))]


def channel_rois():
    """The hostile rois and five ordinary ones."""
    return np.vstack([hostile_rois(), random_rois(5, seed=31)])


def tiny_rois():
    """Rois for maps of 5 x 9 (1/4), 1 x 16 (1/8) and 1 x 1 (1/16) cells: a roi of one cell at 1/16 at the origin has all 49
    bins on the 1 x 1 map's only cell; strips along the 1 x 16 map; boxes over the 5 x 9 map."""
    r = [(0.0, 0.0, 7.0, 7.0), (0.0, 0.0, 35.0, 19.0), (0.0, 0.0, 127.0, 7.0), (-20.0, -12.0, 6.0, 5.0), (4.0, 2.0, 30.0, 16.0),
         (10.0, 0.0, 90.0, 6.0), (0.0, 0.0, 16.0, 16.0), (2.0, 1.0, 5.0, 3.0)]
    a = np.zeros((len(r), 5), np.float32)
    a[:, 1:] = np.asarray(r, np.float32)
    return a


def source_rois(name):
    """[R, 5] rois (R of 6 to 9) of a SOURCE_CASES entry, image 0."""
    return tiny_rois() if name == "tiny" else random_rois({"one": 6, "two": 7, "odd": 9}[name], seed=33)


def empty_share(arg, Cs):
    """Per source: (share of empty bins, number of non-empty bins) of an arg-max [R * 49, sum Cs]."""
    off = np.concatenate([[0], np.cumsum(Cs)]).astype(int)
    return [(float((arg[:, off[i]] < 0).mean()), int((arg[:, off[i]] >= 0).sum())) for i in range(len(Cs))]


# the gather's sweep: one source of C = 4 at scale 1.0 on a 9 x 11 map; every integer range [start, start + width) per axis
SWEEP = dict(C=4, H=9, W=11, widths=tuple(range(1, 10)) + (13, 14, 15, 20, 29), R=2048)


def sweep_rois(x_starts=range(-3, 9), y_starts=range(-3, 7)):
    """2048 integer rois whose x-ranges are every start with every width of SWEEP, the y-ranges likewise; roi i takes x-range
    i mod nx and y-range (5 i + i // nx) mod ny, so every x-range and every y-range occurs.  The starts are trimmed from the
    -3 .. W and -3 .. H of the full sweep, which leaves 62 % of the bins empty; with starts up to W - 1 and H - 1 it is
    still 57 %, with these under half are.  The trim drops the all-empty ranges that begin past the map and also the x
    starts 9, 10 and the y starts 7, 8, which lie on it: wider windows from start 8 or 6 still reach the last column and
    row, clipped, but no window of one or two cells would sit there, so the last eight rois are those, added by hand."""
    xs = [(s, s + w - 1) for s in x_starts for w in SWEEP["widths"]]
    ys = [(s, s + w - 1) for s in y_starts for w in SWEEP["widths"]]
    a = np.zeros((SWEEP["R"], 5), np.float32)
    for i in range(SWEEP["R"]):
        x, y = xs[i % len(xs)], ys[(5 * i + i // len(xs)) % len(ys)]
        a[i, 1:] = (x[0], y[0], x[1], y[1])
    W, H = SWEEP["W"], SWEEP["H"]
    a[-8:, 1:] = [(W - 1, H - 1, W - 1, H - 1), (W - 2, H - 2, W - 1, H - 1), (W - 1, 0, W - 1, H - 1), (0, H - 1, W - 1, H - 1),
                  (W - 2, 3, W - 1, 4), (3, H - 2, 4, H - 1), (W - 1, 2, W - 1, 2), (5, H - 1, 5, H - 1)]
    return a, xs, ys


def source_case(name):
    """A SOURCE_CASES entry for the inference head: dict(Cs, scales, front, head, maps [1, C, H, W], rois, boxes) at Cout 12,
    the reduced fc sizes and 21 classes; the boxes are the rois and copies of the first three (the dedup merges them)."""
    from aznet_hip import synth
    d = SOURCE_CASES[name]
    rois = source_rois(name)
    return dict(Cs=d["Cs"], scales=d["scales"], head=synth.make_det_head(seed=9, C=12, n6=260, n7=516, ncls=21),
                front=synth.make_skip_front(seed=1, Cs=d["Cs"], Cout=12, scales=d["scales"]), maps=edge_maps("relu", 14, d["Cs"], d["hw"]),
                rois=rois, boxes=np.vstack([rois[:, 1:], rois[:3, 1:]]).astype(np.float64))
