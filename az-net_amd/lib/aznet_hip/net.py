"""HipAZNet: the object that stands where the reference's pair of caffe.Net objects stood
(tools/prop_az.py:92-98 builds `nets = {'full': net, 'fc': net_fc}`).

Two ways to use it, both without any CPU compute path:
  * whole search on the GPU -- `detect.test.im_propose(HipAZNet, im)` calls `propose()`,
    i.e. az_propose (the level loop never returns to the host);
  * as a pycaffe-shaped net -- `.blobs[name].reshape(...)` and
    `.forward(blobs=[...], data=... | conv5_3=..., rois=...)` return `zoom_prob`,
    `adj_prob`, `adj_bbox` (and `conv5_3` when asked), which is exactly the surface
    lib/detect/test.py:221-242 drives.  The reference's own Python loop (or the oracle's)
    can therefore run on top of the HIP head unchanged; tests use that to check the fused
    loop against the per-level path.
"""
import numpy as np

from aznet_hip import ffi


def pyramid_blob(ctx, device, im, pixel_means, scales):
    """_get_image_blob of an image pyramid (lib/detect/test.py:27-59 with several cfg.TEST.SCALES) on the GPU: every
    scale's mean-subtracted, INTER_LINEAR-resized image (the front-end kernel, az_image_blob_dev_on) written into one
    zeroed [S,3,Hmax,Wmax] tensor at its top-left corner -- im_list_to_blob's padding at the bottom and right to the
    per-axis maximum of the scaled shapes.  Enqueued on torch's current stream."""
    import torch
    stream = torch.cuda.current_stream(device)
    sizes = [ctx.image_blob_size(im.shape[0], im.shape[1], s) for s in scales]
    Hm, Wm = max(h for h, _ in sizes), max(w for _, w in sizes)
    blob = torch.zeros((len(scales), 3, Hm, Wm), dtype=torch.float32, device=device)
    for i, (s, (oh, ow)) in enumerate(zip(scales, sizes)):
        part = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=device)
        ctx.image_blob(im, pixel_means, float(s), out=part, stream=stream.cuda_stream)
        blob[i, :, :oh, :ow].copy_(part[0])
    return blob


def pyramid_maps(backbone, blob):
    """conv5_3 of every level of a padded pyramid blob, each a [1,C,h,w] channels_last tensor (the layout RoIPool reads)
    of the padded size: the backbone sees the padded image, as Caffe's batch does."""
    import torch
    maps = []
    for i in range(blob.shape[0]):
        conv = backbone(blob[i:i + 1])
        if not conv.is_contiguous(memory_format=torch.channels_last) or conv.is_contiguous():
            conv = conv.contiguous(memory_format=torch.channels_last)
        maps.append(conv)
    return maps


def _skip_names(front):
    """The blob names of a skip front's sources, in concat5's order (default: the last ones of conv3_3, conv4_3, conv5_3)."""
    from aznet_hip import synth
    n = len(front["Cs"])
    names = tuple(front.get("names") or synth.SKIP_NAMES[len(synth.SKIP_NAMES) - n:])
    if len(names) != n:
        raise ValueError("skip front: %d names for %d sources" % (len(names), n))
    return names


class _Blob(object):
    def __init__(self):
        self.shape = None

    def reshape(self, *shape):
        self.shape = tuple(shape)


class _NetDict(object):
    """The reference's test loops take a dict of caffe.Nets ({'full': ..., 'fc': ...}); a net answers net[k], k in net and
    net.keys() with itself for each name in NAMES."""
    NAMES = ()

    def __getitem__(self, k):
        if k in self.NAMES:
            return self
        raise KeyError(k)

    def keys(self):
        return list(self.NAMES)

    def __contains__(self, k):
        return k in self.NAMES


class HipAZNet(_NetDict):
    NAMES = ("full", "fc")

    def __init__(self, head, backbone=None, device=0, name="vgg16_az_net_hip", ctx=None,
                 max_regions=None, gemm_mode=None):
        self.ctx = ctx or ffi.AzContext(device, max_regions=max_regions, gemm_mode=gemm_mode)
        self.ctx.load_head(head)
        if ffi._default_ctx is None or getattr(ffi._default_ctx, "h", None) is None:
            ffi.set_default_context(self.ctx)      # drop-in helpers (nms, divide_region) use this rank's GPU
        self.backbone = backbone
        self.name = name
        self.blobs = {k: _Blob() for k in ("data", "rois", "conv5_3")}
        self._conv = None          # what the last forward/set_image left in HBM
        self.taps = None           # layers compute_conv returns besides conv5_3 (set by a HipDetNet with a skip front)

    # ---- feature map -----------------------------------------------------------------
    def set_conv(self, conv, wait=True):
        """conv: NumPy [1,C,H,W] (copied to HBM) or a CUDA torch tensor (borrowed; torch's current
        stream is synchronised before the ctx stream reads it).  wait=False: see
        AzContext.set_feature_map."""
        self.ctx.set_feature_map(conv, wait=wait)
        self._conv = conv

    def image_blob(self, im, pixel_means, scale):
        """_get_image_blob (lib/detect/test.py:27-59) on the GPU for a uint8 BGR image: with a
        backbone, the blob is written straight into a CUDA tensor the backbone reads (no f32 host
        copy); without one, a NumPy array comes back."""
        if self.backbone is None:
            return self.ctx.image_blob(im, pixel_means, scale)
        import torch
        oh, ow = self.ctx.image_blob_size(im.shape[0], im.shape[1], scale)
        out = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=self.backbone.device)
        torch.cuda.current_stream(out.device).synchronize()
        return self.ctx.image_blob(im, pixel_means, scale, out=out)

    def image_blob_enqueue(self, im, pixel_means, scale):
        """As image_blob for a net with a backbone, without any host wait: upload and front-end kernel are enqueued on
        torch's current stream (where the backbone runs next), az_image_blob_dev_on."""
        import torch
        oh, ow = self.ctx.image_blob_size(im.shape[0], im.shape[1], scale)
        out = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=self.backbone.device)
        return self.ctx.image_blob(im, pixel_means, scale, out=out,
                                   stream=torch.cuda.current_stream(out.device).cuda_stream)

    def compute_conv(self, data_blob):
        """Run the torch backbone on a [1,3,H,W] blob and hand conv5_3 to the HIP context."""
        if self.backbone is None:
            raise RuntimeError("HipAZNet has no backbone: supply conv5_3 with set_conv()")
        import torch
        if self.taps:
            # the skip-connection detector on this context (HipDetNet with a skip front): the tapped maps as well, a dict
            # {name: channels_last map}; the AZ head reads the last one (conv5_3)
            maps = self.backbone(data_blob, taps=self.taps)
            self.set_conv(maps[list(maps)[-1]])
            return maps
        conv = self.backbone(data_blob)
        self.set_conv(conv)                                    # (synchronises torch's stream first)
        return conv

    def compute_pyramid(self, im, pixel_means, scales):
        """An image pyramid (several cfg.TEST.SCALES) through the front-end and the backbone: the S padded conv5_3 maps
        (channels_last CUDA tensors of one size), handed to the context as its pyramid set.  Returns the list of maps."""
        if self.backbone is None:
            raise RuntimeError("HipAZNet has no backbone: supply the pyramid maps with set_pyramid()")
        blob = pyramid_blob(self.ctx, self.backbone.device, im, pixel_means, scales)
        maps = pyramid_maps(self.backbone, blob)
        self.set_pyramid(maps)
        return maps

    def set_pyramid(self, maps):
        """Hand the S padded conv5_3 maps of a pyramid to the context (torch's stream is synchronised first)."""
        self.ctx.set_feature_pyramid(maps)
        self._conv = maps

    def propose_pyramid(self, params, scales, want_scores=False, want_stats=False):
        """im_propose over the pyramid set (az_propose_pyramid: the plain level loop)."""
        return self.ctx.propose_pyramid(params, scales, want_scores=want_scores, want_stats=want_stats)

    # ---- whole search ------------------------------------------------------------------
    def propose(self, params, want_scores=False, want_stats=False, stage=None):
        """stage (multi-GPU): a callable run between launch and fetch, e.g. DeviceGather.stage(j), which
        enqueues the device-to-device copy of the result record into the RCCL send buffer."""
        if stage is None:
            return self.ctx.propose(params, want_scores=want_scores, want_stats=want_stats)
        self.ctx.propose_launch(params)
        stage()
        return self.ctx.propose_fetch(want_scores=want_scores, want_stats=want_stats)

    # ---- pycaffe-shaped surface ----------------------------------------------------------
    def propose_batch(self, params, convs, want_scores=False, want_stats=False):
        """The images of consecutive iterations of the dataset loop (lib/detect/test.py:508-513), all of one shape, searched
        in lockstep (AzContext.batch_launch / batch_fetch): a list with every image's im_propose result."""
        self.ctx.batch_launch(params, convs)
        self._conv = convs[-1]
        return [self.ctx.batch_fetch(i, want_scores=want_scores, want_stats=want_stats) for i in range(len(convs))]

    def forward(self, blobs=None, **kw):
        rois = np.ascontiguousarray(kw["rois"], dtype=np.float32)
        if "conv5_3" in kw:
            conv = kw["conv5_3"]
            if conv is not self._conv:
                self.set_conv(conv)
        elif "data" in kw:
            self.compute_conv(kw["data"])
        z, p, d = self.ctx.head_forward(rois)
        out = {"zoom_prob": z, "adj_prob": p, "adj_bbox": d}
        if blobs:
            for b in blobs:
                out[b] = self._conv
        return out


class _DetNet(_NetDict):
    """What HipDetNet and HipFrcnnNet share: the detection head and the optional skip front in self.ctx, and `run`, the one
    place that binds the maps (HipDetNet | HipFrcnnNet) and chooses the AzContext entry of a detection call:
        several scales    set_pyramid | set_feature_pyramid(maps)            detect_pyramid (refine: refused by _frcnn_forward)
        one, skip front   set_skip_conv | set_skip_maps                      detect_skip, refine: detect_iter(skip=True)
        one               set_conv | refine: set_feature_pyramid([conv])     detect | one-image detect_batch, refine: detect_iter
    det_head may carry truncated-SVD factors (L6, U6 and / or L7, U7 in place of W6 / W7: aznet_hip.compress, or
    caffemodel.det_head_from_layers of a file written by tools/compress_net.py): it is loaded through
    az_load_det_head_lowrank and every entry runs the compressed layers (fp32 contexts only)."""

    def _load(self, det_head, skip_front, name):
        """skip_front: the skip-connection detector's front (synth.make_skip_front / caffemodel.skip_front_from_layers;
        default: det_head["skip_front"], which caffemodel.det_head_from_layers sets for a file with conv_pool5)."""
        self.ctx.load_det_head(det_head)           # (a dict with L / U factors: AzContext.load_det_head_lowrank)
        if skip_front is None:
            skip_front = det_head.get("skip_front") if isinstance(det_head, dict) else None
        self.num_classes = self.ctx.det_dims["ncls"]
        self.name = name
        self.blobs = {k: _Blob() for k in ("data", "rois", "conv5_3")}
        self.skip_front, self.skip_names, self._skip_maps = None, None, None
        if skip_front is not None:
            self.attach_skip_front(skip_front)

    def attach_skip_front(self, front):
        """Load `front` into the net's context; compute_conv then returns the maps it names."""
        self.ctx.load_skip_front(front)
        self.skip_front, self.skip_names, self._skip_maps = front, _skip_names(front), None

    def run(self, boxes, scales, im_shape, args, maps=None, refine=None, pyramid=None):
        """One detection call: (scores, boxes, extra-or-None).  scales: the list of test scales (several, or pyramid=True:
        over the pyramid set); args = (dedup, batch_size, eps); maps: what to bind first (_bind; None: what the context
        holds); refine = (rounds, min_score, max_rows): iterative localisation, extra as AzContext.detect_iter returns it."""
        dedup, batch_size, eps = args
        kw = dict(dedup=dedup, batch_size=batch_size, eps=eps)
        h, w = im_shape[0], im_shape[1]
        skip = self.skip_front is not None
        if pyramid is None:
            pyramid = len(scales) > 1
        if maps is not None:
            self._bind(maps, pyramid, refine is not None)
        if pyramid:
            s, b = self.ctx.detect_pyramid(boxes, scales, h, w, **kw)
        elif refine is not None:
            return self.ctx.detect_iter(boxes, scales[0], h, w, *refine, skip=skip, **kw)
        elif skip:
            s, b = self.ctx.detect_skip(boxes, scales[0], h, w, **kw)
        else:
            s, b = self._detect_one(maps, boxes, scales[0], im_shape, kw)
        return s, b, None


class HipDetNet(_DetNet):
    """Fast R-CNN detection net on the shared conv map: stands where the reference's
    `frcnn_nets = {'fc': caffe.Net(frcnn/test_fc.prototxt, ...)}` stood (tools/test_shared.py).
    It shares the AZ net's az_ctx, so both heads read the same channel-last map in HBM.
    Also pycaffe-shaped (`forward(rois=, conv5_3=)` -> cls_prob, bbox_pred; test.py:302-307)."""
    NAMES = ("fc",)

    def __init__(self, det_head, az_net, name="vgg16_frcnn_hip", skip_front=None):
        """With a skip front the head pools every roi from the maps the front names (cfg.SEAR.FRCNN_CONV) instead of
        conv5_3 alone, and the shared AZ net's compute_conv returns those maps."""
        self.ctx = az_net.ctx
        self.az_net = az_net
        self._load(det_head, skip_front, name)

    def attach_skip_front(self, front):
        """Load `front` into the shared context and make the AZ net's compute_conv return the maps it names."""
        _DetNet.attach_skip_front(self, front)
        self.az_net.taps = self.skip_names[:-1]
        self.blobs = {k: _Blob() for k in ("data", "rois") + self.skip_names}

    def set_skip_conv(self, conv):
        """conv: {name: map} with every map the front names; handed to the context (borrowed) unless it already holds
        these very tensors."""
        maps = [conv[n] for n in self.skip_names]
        if self._skip_maps is None or len(maps) != len(self._skip_maps) or any(a is not b for a, b in zip(maps, self._skip_maps)):
            self.ctx.set_skip_maps(maps)
            self._skip_maps = maps
            self.az_net._conv = maps[-1]

    def _bind(self, maps, pyramid, iterative):
        """maps: the {name: map} dict of the skip model, or conv5_3 / the pyramid's list of maps; bound unless it is bound."""
        if self.skip_front is not None:
            self.set_skip_conv(maps)
        elif maps is not self.az_net._conv:
            (self.az_net.set_pyramid if pyramid else self.az_net.set_conv)(maps)

    def _detect_one(self, maps, boxes, scale, im_shape, kw):
        return self.ctx.detect(boxes, scale, im_shape[0], im_shape[1], **kw)

    def detect(self, boxes, scale, im_shape, dedup, batch_size, eps):
        return self.run(boxes, [scale], im_shape, (dedup, batch_size, eps))[:2]

    def detect_iter(self, boxes, scale, im_shape, dedup, batch_size, eps, rounds, min_score, max_rows):
        """detect() followed by rounds - 1 rounds of iterative localisation: (scores, boxes, extra), see AzContext.detect_iter."""
        return self.run(boxes, [scale], im_shape, (dedup, batch_size, eps), refine=(rounds, min_score, max_rows))

    def detect_pyramid(self, boxes, scales, im_shape, dedup, batch_size, eps):
        """_frcnn_forward over the pyramid set the shared context holds (HipAZNet.compute_pyramid / set_pyramid)."""
        return self.run(boxes, scales, im_shape, (dedup, batch_size, eps), pyramid=True)[:2]

    def forward(self, blobs=None, **kw):
        rois = np.ascontiguousarray(kw["rois"], dtype=np.float32)
        if self.skip_front is not None:
            if all(n in kw for n in self.skip_names):
                self.set_skip_conv(kw)
            p, b = self.ctx.det_forward_skip(rois)
        else:
            if "conv5_3" in kw:
                self._bind(kw["conv5_3"], False, False)
            p, b = self.ctx.det_forward(rois)
        return {"cls_prob": p, "bbox_pred": b}


class HipFrcnnNet(_DetNet):
    """Fast R-CNN detection net with its OWN conv layers, for detection over saved proposals: stands where the
    reference's `nets = {'full': caffe.Net(frcnn/test.prototxt, caffemodel)}` stood (tools/test_det_net.py, used by
    test_net, lib/detect/test.py:541-668).  It owns an az_ctx with only the detection head loaded (fp32) and a backbone:
    any callable that maps the [1,3,H,W] data blob (a CUDA tensor) to conv5_3 -- normally a VGG16Conv5 with the
    detection net's conv weights (caffemodel.backbone_from_layers).
    `detect` / `detect_batch` run az_detect_batch."""
    NAMES = ("full",)

    def __init__(self, det_head, backbone, device=0, name="vgg16_frcnn_hip", max_regions=None, skip_front=None):
        """With a skip front the backbone must take `taps` (VGG16Conv5.forward), compute_conv returns the dict of maps
        and detect goes through az_detect_skip."""
        self.ctx = ffi.AzContext(device, max_regions=max_regions, gemm_mode=0)
        self._load(det_head, skip_front, name)
        if ffi._default_ctx is None or getattr(ffi._default_ctx, "h", None) is None:
            ffi.set_default_context(self.ctx)      # apply_nms and the other drop-in helpers use this GPU
        self.backbone = backbone
        self.device = int(device)

    def _torch_device(self):
        import torch
        dev = getattr(self.backbone, "device", None)
        return torch.device(dev) if dev is not None else torch.device("cuda", self.device)

    def image_blob_enqueue(self, im, pixel_means, scale):
        """_get_image_blob (lib/detect/test.py:27-59) into a CUDA tensor, enqueued on torch's current stream (where the
        backbone runs next): no host wait."""
        import torch
        dev = self._torch_device()
        oh, ow = self.ctx.image_blob_size(im.shape[0], im.shape[1], scale)
        out = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=dev)
        return self.ctx.image_blob(im, pixel_means, scale, out=out, stream=torch.cuda.current_stream(dev).cuda_stream)

    def compute_conv(self, data_blob):
        """conv5_3 of one data blob, enqueued on torch's current stream (channels_last: the layout RoIPool reads)."""
        import torch
        if self.skip_front is not None:
            maps = self.backbone(data_blob, taps=self.skip_names[:-1])
            return {n: maps[n] for n in self.skip_names}
        conv = self.backbone(data_blob)
        if not conv.is_contiguous(memory_format=torch.channels_last):
            conv = conv.contiguous(memory_format=torch.channels_last)
        return conv

    def compute_pyramid(self, im, pixel_means, scales):
        """An image pyramid through the front-end and this net's backbone; the S padded conv5_3 maps become the
        context's pyramid set.  Returns the list of maps."""
        dev = self._torch_device()
        maps = pyramid_maps(self.backbone, pyramid_blob(self.ctx, dev, im, pixel_means, scales))
        self.ctx.set_feature_pyramid(maps)
        return maps

    def _bind(self, maps, pyramid, iterative):
        """maps: the pyramid's list of maps, the {name: map} dict of the skip model, or conv5_3 -- which only the
        iterative route binds, as a pyramid of one level (set_feature_pyramid, whose level 0 is the context's single map:
        az_set_feature_map_* want an AZ head, which this context has not); the plain route hands it to az_detect_batch."""
        if pyramid:
            self.ctx.set_feature_pyramid(maps)
        elif self.skip_front is not None:
            self.ctx.set_skip_maps([maps[n] for n in self.skip_names])
        elif iterative:
            self.ctx.set_feature_pyramid([maps])

    def _detect_one(self, conv, boxes, scale, im_shape, kw):
        return self.ctx.detect_batch([conv], [boxes], [scale], [im_shape], **kw)[0]

    def detect(self, conv, boxes, scale, im_shape, dedup, batch_size, eps):
        """One image: az_detect_batch with its pieces, or (a skip front) az_detect_skip on the dict of maps `conv` -- the
        region capacity then bounds the proposals of one call, AZ_ERR_CAPACITY beyond it (as it does for detect_iter)."""
        return self.run(boxes, [scale], im_shape, (dedup, batch_size, eps), maps=conv)[:2]

    def detect_iter(self, conv, boxes, scale, im_shape, dedup, batch_size, eps, rounds, min_score, max_rows):
        """detect() followed by rounds - 1 rounds of iterative localisation: (scores, boxes, extra), see AzContext.detect_iter."""
        return self.run(boxes, [scale], im_shape, (dedup, batch_size, eps), maps=conv, refine=(rounds, min_score, max_rows))

    def detect_pyramid(self, maps, boxes, scales, im_shape, dedup, batch_size, eps):
        """_frcnn_forward of one image over its pyramid maps (az_detect_pyramid)."""
        return self.run(boxes, scales, im_shape, (dedup, batch_size, eps), maps=maps, pyramid=True)[:2]

    def detect_batch(self, convs, boxes_list, scales, im_shapes, dedup, batch_size, eps):
        if self.skip_front is not None:
            raise ValueError("the skip-connection detector runs one image per call (az_detect_skip): no az_detect_batch")
        return self.ctx.detect_batch(convs, boxes_list, scales, im_shapes, dedup=dedup, batch_size=batch_size, eps=eps)
