"""A small reader for the two protobuf TEXT files the reference hands to caffe.SGDSolver (lib/detect/train_az.py:41-49):
the solver prototxt (flat `key: value`) and, from the `train_net` it names, per layer only what training on this backend
needs -- `param { lr_mult decay_mult }`, `dropout_ratio` and the weight filler's `std`.  The layer GRAPH is fixed here
(VGG16 conv1_1 .. conv5_3, roi_pool5, int6, int7_1 / int7_2, adj_score / adj_bbox / zoom_score): a net whose learnable
layers are not exactly these is refused.  `write_train_prototxt` / `write_solver_prototxt` emit such files from a layer
table (the synthetic runs of tools/train_az_net.py and the tests; the reference's own files are not shipped)."""
import os
import re

CONV_LAYERS = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2",
               "conv4_3", "conv5_1", "conv5_2", "conv5_3")
HEAD_LAYERS = ("int6", "int7_1", "int7_2", "adj_score", "adj_bbox", "zoom_score")
DROPOUT_OF = {"int6": 0, "int7_1": 1, "int7_2": 2}
FILLER_STD = {"int6": 1e-4, "int7_1": 1e-4, "int7_2": 1e-3, "adj_score": 1e-2, "adj_bbox": 1e-3, "zoom_score": 1e-2}
# the detection net (models/*/VGG16/frcnn/train.prototxt): fc6 / fc7 carry no filler (they come from the pretrained model)
DET_HEAD_LAYERS = ("fc6", "fc7", "cls_score", "bbox_pred")
DET_DROPOUT_OF = {"fc6": 0, "fc7": 1}
DET_FILLER_STD = {"fc6": None, "fc7": None, "cls_score": 1e-2, "bbox_pred": 1e-3}
DET_FILLER_DEFAULT = 5e-3          # fc6 / fc7 without a pretrained model
# the skip-connection detector (models/COCO/VGG16_skip/frcnn/{finetune,frozen}/train.prototxt): conv_pool5, a 1x1 Convolution
# (xavier filler) behind roi_pool3/4/5 -> roi_norm3/4/5 (GRN) -> concat5 -> scale5 (Power), in front of fc6
SKIP_HEAD_LAYERS = ("conv_pool5",) + DET_HEAD_LAYERS
SKIP_SOURCES = ("conv3_3", "conv4_3", "conv5_3")
SKIP_SCALES = (0.25, 0.125, 0.0625)
SKIP_GAIN = 1000.0
SOLVER_DEFAULTS = dict(base_lr=0.001, lr_policy="step", gamma=0.1, stepsize=120000, momentum=0.9, weight_decay=0.0005,
                       clip_gradients=-1.0, display=20, average_loss=1, snapshot_prefix="vgg16_az_net", train_net=None,
                       iter_size=1)

_TOKEN = re.compile(r"""\s*(?:(\#[^\n]*)|([{}:])|"((?:[^"\\]|\\.)*)"|'((?:[^'\\]|\\.)*)'|([^\s{}:#"']+))""")


def _tokens(text):
    pos, out = 0, []
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            if text[pos:].strip() == "":
                break
            raise ValueError("prototxt: cannot read %r" % text[pos:pos + 20])
        pos = m.end()
        if m.group(1) is not None:
            continue
        if m.group(2) is not None:
            out.append((m.group(2), None))
        elif m.group(3) is not None or m.group(4) is not None:
            out.append(("str", m.group(3) if m.group(3) is not None else m.group(4)))
        else:
            out.append(("word", m.group(5)))
    return out


def _scalar(kind, v):
    if kind == "str":
        return v
    for cast in (int, float):
        try:
            return cast(v)
        except ValueError:
            pass
    return {"true": True, "false": False}.get(v, v)


def parse_text(text):
    """Protobuf text format -> a list of (key, value) pairs; a message value is itself such a list."""
    toks = _tokens(text)

    def block(i, top):
        items = []
        while i < len(toks):
            kind, v = toks[i]
            if kind == "}":
                if top:
                    raise ValueError("prototxt: unbalanced '}'")
                return items, i + 1
            if kind != "word":
                raise ValueError("prototxt: expected a field name, got %r" % (v or kind))
            key = v
            i += 1
            if i < len(toks) and toks[i][0] == ":":
                i += 1
            if i >= len(toks):
                raise ValueError("prototxt: field %s has no value" % key)
            if toks[i][0] == "{":
                val, i = block(i + 1, False)
            else:
                val = _scalar(*toks[i])
                i += 1
            items.append((key, val))
        if not top:
            raise ValueError("prototxt: missing '}'")
        return items, i
    return block(0, True)[0]


def _get(items, key, default=None):
    for k, v in items:
        if k == key:
            return v
    return default


def read_solver(path):
    """The solver prototxt as a dict over SOLVER_DEFAULTS' keys (other fields, e.g. `snapshot: 0`, are ignored)."""
    with open(path) as f:
        items = parse_text(f.read())
    out = dict(SOLVER_DEFAULTS)
    for k, v in items:
        if isinstance(v, list):
            raise ValueError("solver prototxt: %s is a message; expected flat `key: value` lines" % k)
        if k in out:
            out[k] = v
    if out["train_net"] is None:
        raise ValueError("solver prototxt %s names no train_net" % path)
    if out["lr_policy"] not in ("step", "fixed"):
        raise ValueError("lr_policy %r: this backend implements \"step\" and \"fixed\"" % (out["lr_policy"],))
    out["iter_size"] = check_iter_size(out["iter_size"])
    return out


def check_iter_size(v):
    """Caffe's iter_size (minibatches accumulated per iteration): an integer >= 1, else a ValueError."""
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError("iter_size %r: an integer >= 1" % (v,))
    return v


def read_train_net(path):
    """{layer name: {"lr_mult": [w, b], "decay_mult": [w, b], "dropout_ratio": r or None, "std": s or None}} for the
    thirteen convolutions and the six InnerProduct layers.  Caffe's defaults (1 / 1) stand where a `param` block is absent."""
    return _read_net(path, HEAD_LAYERS, DROPOUT_OF, "AZ-net")


def read_det_train_net(path):
    """The same table for the detection net (frcnn/train.prototxt): the thirteen convolutions, fc6, fc7, cls_score,
    bbox_pred, with Dropout on fc6 / fc7."""
    return _read_net(path, DET_HEAD_LAYERS, DET_DROPOUT_OF, "detection net")


def _all(items, key):
    return [v for k, v in items if k == key]


def read_skip_train_net(path):
    """(table, front) of the skip-connection detector's train net: read_det_train_net's table plus a `conv_pool5` row, and
    the front's settings as the file states them: {"sources": the ROIPooling layers' map bottoms in concat order, "scales":
    their spatial_scale, "gain": the Power layer's scale}.  Refused (ValueError): a Power layer with power != 1 or shift != 0,
    a pooled size other than 7x7, a pooled blob without a GRN layer on it, a Concat whose bottoms are not the pooled blobs in
    the ROIPooling layers' order."""
    table = _read_net(path, SKIP_HEAD_LAYERS, DET_DROPOUT_OF, "skip-connection detection net", conv_heads=("conv_pool5",))
    with open(path) as f:
        items = parse_text(f.read())
    layers = [v for k, v in items if k in ("layer", "layers") and isinstance(v, list)]
    pools, normed, concat, gain = [], set(), None, 1.0
    for L in layers:
        name, typ = _get(L, "name"), str(_get(L, "type", ""))
        if typ == "ROIPooling":
            rp = _get(L, "roi_pooling_param")
            rp = rp if isinstance(rp, list) else []
            if int(_get(rp, "pooled_w", 0)) != 7 or int(_get(rp, "pooled_h", 0)) != 7:
                raise ValueError("%s: %s pools to %sx%s; this backend pools 7x7" % (path, name, _get(rp, "pooled_h", 0), _get(rp, "pooled_w", 0)))
            bottoms = _all(L, "bottom")
            if len(bottoms) != 2 or _get(L, "top") is None:
                raise ValueError("%s: %s needs a map and a rois bottom and a top" % (path, name))
            pools.append((_get(L, "top"), bottoms[0], float(_get(rp, "spatial_scale", 1.0))))
        elif typ == "GRN":
            if _get(L, "top") != _get(L, "bottom"):
                raise ValueError("%s: GRN layer %s is not in place" % (path, name))
            normed.add(_get(L, "bottom"))
        elif typ == "Concat":
            if concat is not None:
                raise ValueError("%s: more than one Concat layer" % path)
            cp = _get(L, "concat_param")
            if isinstance(cp, list) and int(_get(cp, "axis", 1)) != 1:
                raise ValueError("%s: %s concatenates along axis %s, not the channels" % (path, name, _get(cp, "axis")))
            concat = (_all(L, "bottom"), _get(L, "top"))
        elif typ == "Power":
            pp = _get(L, "power_param")
            pp = pp if isinstance(pp, list) else []
            if float(_get(pp, "power", 1.0)) != 1.0 or float(_get(pp, "shift", 0.0)) != 0.0:
                raise ValueError("%s: Power layer %s with power %s, shift %s; this backend has power 1, shift 0 (a plain scale)"
                                 % (path, name, _get(pp, "power", 1.0), _get(pp, "shift", 0.0)))
            gain = float(_get(pp, "scale", 1.0))
    if not pools or concat is None:
        raise ValueError("%s: not the skip-connection detection net (no ROIPooling layers or no Concat)" % path)
    if len(pools) > 3:
        raise ValueError("%s: %d ROIPooling layers; this backend takes up to 3" % (path, len(pools)))
    for top, _, _ in pools:
        if top not in normed:
            raise ValueError("%s: no GRN layer on the pooled blob %r" % (path, top))
    if list(concat[0]) != [top for top, _, _ in pools]:
        raise ValueError("%s: the Concat layer joins %s, the ROIPooling layers give %s in this order"
                         % (path, list(concat[0]), [top for top, _, _ in pools]))
    return table, {"sources": [b for _, b, _ in pools], "scales": [sc for _, _, sc in pools], "gain": gain}


def _read_net(path, HEAD_LAYERS, DROPOUT_OF, what, conv_heads=()):
    with open(path) as f:
        items = parse_text(f.read())
    layers = [v for k, v in items if k in ("layer", "layers") and isinstance(v, list)]
    if not layers:
        raise ValueError("%s: no layers" % path)
    out, drops = {}, {}
    for L in layers:
        name, typ = _get(L, "name"), str(_get(L, "type", ""))
        if typ in ("Convolution", "InnerProduct"):
            if name not in CONV_LAYERS + HEAD_LAYERS or (typ == "Convolution") != (name in CONV_LAYERS + tuple(conv_heads)):
                raise ValueError("%s: learnable layer %r (%s) is not part of the %s this backend trains "
                                 "(conv1_1 .. conv5_3, %s)" % (path, name, typ, what, ", ".join(HEAD_LAYERS)))
            params = [v for k, v in L if k == "param" and isinstance(v, list)]
            lr = [float(_get(p, "lr_mult", 1.0)) for p in params] + [1.0, 1.0]
            dc = [float(_get(p, "decay_mult", 1.0)) for p in params] + [1.0, 1.0]
            std = None
            ip = _get(L, "inner_product_param")
            if isinstance(ip, list) and isinstance(_get(ip, "weight_filler"), list):
                std = _get(_get(ip, "weight_filler"), "std")
            out[name] = {"lr_mult": lr[:2], "decay_mult": dc[:2], "dropout_ratio": None,
                         "std": float(std) if std is not None else None}
        elif typ == "Dropout":
            dp = _get(L, "dropout_param")
            drops[_get(L, "bottom")] = float(_get(dp, "dropout_ratio", 0.5)) if isinstance(dp, list) else 0.5
    missing = [n for n in CONV_LAYERS + HEAD_LAYERS if n not in out]
    if missing:
        raise ValueError("%s: not the %s (missing %s)" % (path, what, ", ".join(missing)))
    for bottom, r in drops.items():
        if bottom not in DROPOUT_OF:
            raise ValueError("%s: Dropout on %r; this backend has it on %s" % (path, bottom, ", ".join(sorted(DROPOUT_OF, key=DROPOUT_OF.get))))
        out[bottom]["dropout_ratio"] = r
    return out


def resolve_train_net(solver_path, train_net):
    """Caffe opens train_net relative to the working directory; a file beside the solver is accepted as well."""
    for p in (train_net, os.path.join(os.path.dirname(os.path.abspath(solver_path)), os.path.basename(train_net))):
        if os.path.exists(p):
            return p
    raise IOError("train_net %s not found (from %s)" % (train_net, solver_path))


# ---- writers ------------------------------------------------------------------------------------------------------------
def _layer_rows(heads, filler_std, dropout_of, frozen, dropout):
    rows = []
    for n in CONV_LAYERS:
        f = n in frozen
        rows.append((n, "Convolution", 0.0 if f else 1.0, 0.0 if f else 2.0, 0.0 if f else 1.0, 0.0, None, None))
    for n in heads:
        rows.append((n, "InnerProduct", 1.0, 2.0, 1.0, 0.0, filler_std[n], dropout if n in dropout_of else None))
    return rows


def layer_table(frozen=("conv1_1", "conv1_2", "conv2_1", "conv2_2"), dropout=0.5):
    """The AZ-net's learnable layers as rows (name, type, lr_mult w, lr_mult b, decay_mult w, decay_mult b, std, dropout):
    train.prototxt freezes conv1_1 .. conv2_2, the shared variant all thirteen convolutions."""
    return _layer_rows(HEAD_LAYERS, FILLER_STD, DROPOUT_OF, frozen, dropout)


def det_layer_table(frozen=("conv1_1", "conv1_2", "conv2_1", "conv2_2"), dropout=0.5):
    """The detection net's learnable layers as layer_table's rows: frcnn/train.prototxt freezes conv1_1 .. conv2_2."""
    return _layer_rows(DET_HEAD_LAYERS, DET_FILLER_STD, DET_DROPOUT_OF, frozen, dropout)


def skip_layer_table(frozen=CONV_LAYERS, dropout=0.5):
    """The skip-connection detector's learnable layers as layer_table's rows: det_layer_table's with conv_pool5 in front of
    fc6.  The reference's frozen/ net holds all thirteen convolutions fixed (the default), its finetune/ net conv1_1 ..
    conv2_2 only."""
    rows = det_layer_table(frozen=frozen, dropout=dropout)
    k = [r[0] for r in rows].index("fc6")
    return rows[:k] + [("conv_pool5", "Convolution", 1.0, 2.0, 1.0, 0.0, None, None)] + rows[k:]


def _skip_front_text(sources, scales, gain):
    out, tops = [], []
    for src, sc in zip(sources, scales):
        tag = src[4] if src.startswith("conv") and len(src) > 4 else str(len(tops))
        top = "roi_pool%s" % tag
        tops.append(top)
        out.append('layer {\n  name: "%s"\n  type: "ROIPooling"\n  bottom: "%s"\n  bottom: "rois"\n  top: "%s"\n  roi_pooling_param {\n'
                   '    pooled_w: 7\n    pooled_h: 7\n    spatial_scale: %r\n  }\n}' % (top, src, top, float(sc)))
        out.append('layer {\n  name: "roi_norm%s"\n  type: "GRN"\n  bottom: "%s"\n  top: "%s"\n}' % (tag, top, top))
    out.append('layer {\n  name: "concat5"\n  type: "Concat"\n%s  top: "cat5"\n  concat_param {\n    axis: 1\n  }\n}'
               % "".join('  bottom: "%s"\n' % t for t in tops))
    out.append('layer {\n  name: "scale5"\n  type: "Power"\n  bottom: "cat5"\n  top: "cat5"\n  power_param {\n    power: 1\n'
               '    scale: %r\n    shift: 0\n  }\n}' % float(gain))
    return out


def write_skip_train_prototxt(path, rows, name="frcnn_skip_train", sources=SKIP_SOURCES, scales=SKIP_SCALES, gain=SKIP_GAIN):
    """write_train_prototxt for skip_layer_table's rows, with the front's layers (ROIPooling + GRN per source, Concat, Power)
    in front of conv_pool5: a file read_skip_train_net accepts."""
    write_train_prototxt(path, rows, name=name, before={"conv_pool5": _skip_front_text(sources, scales, gain)})


def write_train_prototxt(path, rows, name="az_net_train", before=None):
    """before: {layer name: [layer texts]} to put in front of that row."""
    out = ['name: "%s"' % name]
    for name, typ, lw, lb, dw, db, std, drop in rows:
        out.extend((before or {}).get(name, []))
        out.append('layer {\n  name: "%s"\n  type: "%s"\n  param {\n    lr_mult: %g\n    decay_mult: %g\n  }\n  param {\n'
                   '    lr_mult: %g\n    decay_mult: %g\n  }' % (name, typ, lw, dw, lb, db))
        if name == "conv_pool5":
            out.append('  convolution_param {\n    kernel_size: 1\n    stride: 1\n    weight_filler {\n      type: "xavier"\n    }\n'
                       '    bias_filler {\n      type: "constant"\n      value: 0\n    }\n  }')
        if std is not None:
            out.append('  inner_product_param {\n    weight_filler {\n      type: "gaussian"\n      std: %g\n    }\n'
                       '    bias_filler {\n      type: "constant"\n      value: 0\n    }\n  }' % std)
        out.append("}")
        if drop is not None:
            out.append('layer {\n  name: "drop_%s"\n  type: "Dropout"\n  bottom: "%s"\n  top: "%s"\n  dropout_param {\n'
                       '    dropout_ratio: %g\n  }\n}' % (name, name, name, drop))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def write_solver_prototxt(path, train_net, **kw):
    d = dict(SOLVER_DEFAULTS)
    d.update(kw)
    d["train_net"] = train_net
    with open(path, "w") as f:
        for k in ("train_net", "base_lr", "lr_policy", "gamma", "stepsize", "momentum", "weight_decay", "clip_gradients",
                  "display", "average_loss", "snapshot_prefix"):
            v = d[k]
            f.write('%s: %s\n' % (k, '"%s"' % v if isinstance(v, str) else repr(v)))
        if check_iter_size(d["iter_size"]) != 1:
            f.write("iter_size: %d\n" % d["iter_size"])
        f.write("# snapshots are written by SolverWrapper.snapshot\nsnapshot: 0\n")
