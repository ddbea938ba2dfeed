"""VGG16 conv1_1 .. conv5_3 forward in PyTorch-ROCm (fp32).

This is the one place torch computes anything: north_star keeps the backbone on
PyTorch-ROCm and the hand-written HIP path starts at its output.  Architecture per
models/Pascal/VGG16/az-net/test.prototxt:16-384: thirteen 3x3 pad-1 convs + ReLU, four
2x2/2 max-pools in Caffe's ceil mode (600x1000 -> 38x63), no pool5.  torchvision is not
available offline, so the stack is spelled out here; weights are seeded He-normal unless
a dict of Caffe-layout arrays is supplied.
"""
import numpy as np
import torch
import torch.nn.functional as F

# (name, out_channels) with 'P' = max-pool
VGG16_CONV = [("conv1_1", 64), ("conv1_2", 64), "P", ("conv2_1", 128), ("conv2_2", 128), "P",
              ("conv3_1", 256), ("conv3_2", 256), ("conv3_3", 256), "P",
              ("conv4_1", 512), ("conv4_2", 512), ("conv4_3", 512), "P",
              ("conv5_1", 512), ("conv5_2", 512), ("conv5_3", 512)]


class VGG16Conv5(object):
    def __init__(self, device="cuda:0", seed=4321, weights=None, width_div=1, channels_last_out=False,
                 channels_last_compute=None):
        """width_div > 1 shrinks every layer's channel count (fast tests); 1 = real VGG16.
        channels_last_out: return conv5_3 in torch.channels_last memory ([H][W][C], the layout RoIPool reads):
        the HIP context then borrows it without its own transpose.
        channels_last_compute (default off): weights and activations in channels_last memory.  With
        torch.backends.cudnn.benchmark = True set BEFORE the first forward, MIOpen then finds fp32 convolutions that run
        ~12 % faster on MI355X (4.09 -> 3.61 ms for a 600x1000 image); without the benchmark search the same layout
        falls on a slower default (6.0 ms), which is why it is opt-in.  Same arithmetic type either way."""
        self.device = torch.device(device)
        self.channels_last_out = bool(channels_last_out)
        self.cl_compute = bool(channels_last_compute) and self.device.type == "cuda"
        self.fused_epilogue = True          # (False: PyTorch's own bias / ReLU / pool launches -- tests compare the two)
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.layers = []
        cin = 3
        for item in VGG16_CONV:
            if item == "P":
                self.layers.append(None)
                continue
            name, cout = item
            cout = max(4, cout // width_div)
            if weights is not None and name in weights:
                w = torch.from_numpy(np.ascontiguousarray(weights[name][0], dtype=np.float32))
                b = torch.from_numpy(np.ascontiguousarray(weights[name][1], dtype=np.float32))
            else:
                w = torch.randn(cout, cin, 3, 3, generator=g) * float(np.sqrt(2.0 / (cin * 9)))
                b = torch.zeros(cout)
            w = w.to(self.device)
            if self.cl_compute:
                w = w.contiguous(memory_format=torch.channels_last)
            self.layers.append((name, w, b.to(self.device)))
            cin = int(w.shape[0])
        self.out_channels = cin

    @torch.no_grad()
    def forward(self, blob, taps=None):
        """blob: [1,3,H,W] float32 (BGR, mean-subtracted), NumPy or torch -> conv5_3 [1,C,h,w]
        contiguous fp32 tensor on the device.
        taps (the skip-connection detector: cfg.SEAR.FRCNN_CONV with several names), e.g. ("conv3_3", "conv4_3"): a dict
        {name: [1,C,h,w] map in torch.channels_last memory} of the named layers' post-ReLU outputs and of conv5_3."""
        taps = tuple(taps or ())
        x, kept = self._layers(blob, taps)
        if taps:
            kept[[layer[0] for layer in self.layers if layer is not None][-1]] = x.contiguous(memory_format=torch.channels_last)
            return kept
        if self.channels_last_out:
            return x.contiguous(memory_format=torch.channels_last)
        return x.contiguous()

    def _layers(self, blob, taps):
        """The layer stack on `blob`: (conv5_3 as the last layer left it, {name: channels_last copy} of the layers named in
        `taps`).  A tapped layer in front of a pool cannot take the fused bias + ReLU + pool epilogue (its pre-pool output
        must exist): bias + ReLU in place (az_bias_relu), then the pool -- the same fp32 operations, the same bits."""
        names = [layer[0] for layer in self.layers if layer is not None]
        for t in taps:
            if t not in names:
                raise ValueError("no layer %r to tap (layers: %s)" % (t, ", ".join(names)))
        kept = {}
        x = torch.as_tensor(blob, dtype=torch.float32, device=self.device)
        if self.cl_compute:
            x = x.contiguous(memory_format=torch.channels_last)
        # On the GPU: what follows a convolution -- bias, ReLU, and the pooling layer where there is one --
        # is ONE pass over its output (az_bias_relu / az_bias_relu_pool, az_epilogue.hip) instead of PyTorch's two or three
        # element-wise launches; same fp32 operations, same bits.  The convolutions are PyTorch-ROCm's either way.
        fused = self.fused_epilogue and x.is_cuda and x.shape[0] == 1
        skip_pool = False
        for li, layer in enumerate(self.layers):
            if layer is None:
                if not skip_pool:
                    x = F.max_pool2d(x, kernel_size=2, stride=2, ceil_mode=True)
                skip_pool = False
                continue
            x, skip_pool = self._conv_relu(x, li, layer, fused, layer[0] in taps)
            if layer[0] in taps:
                kept[layer[0]] = x.contiguous(memory_format=torch.channels_last)
        return x, kept

    def _conv_relu(self, x, li, layer, fused, tapped):
        """One convolution + bias + ReLU (+ the pool behind it when the fused epilogue takes it: second result True)."""
        if fused and (layer[1].shape[0] % 4 == 0 or not self.cl_compute):
            y = F.conv2d(x, layer[1], None, padding=1)
            if (y.is_contiguous(memory_format=torch.channels_last) if self.cl_compute else y.is_contiguous()) \
                    and y.data_ptr() % 16 == 0 and layer[2].data_ptr() % 16 == 0 and layer[2].is_contiguous():
                from . import ffi
                try:
                    if not tapped and li + 1 < len(self.layers) and self.layers[li + 1] is None:
                        return ffi.bias_relu_pool(y, layer[2]), True
                    return ffi.bias_relu_(y, layer[2]), False
                except ffi.AzError as e:
                    # (a layout the fused kernels decline -- AZ_ERR_INVALID, nothing was written: PyTorch's own ops)
                    if e.code != ffi.AZ_ERR_INVALID:
                        raise
            return F.relu_(y + layer[2].view(1, -1, 1, 1)), False
        return F.relu_(F.conv2d(x, layer[1], layer[2], padding=1)), False

    __call__ = forward

    def set_trainable(self, names):
        """The convolutions whose parameters take gradients in forward_train (train.prototxt: lr_mult > 0); every other
        layer is frozen.  Returns [(name, weight, bias)] of the trainable ones: leaf tensors whose .grad backward fills."""
        out = []
        for layer in self.layers:
            if layer is None:
                continue
            on = layer[0] in names
            layer[1].requires_grad_(on)
            layer[2].requires_grad_(on)
            if on:
                out.append(layer)
        return out

    def forward_train(self, blob, taps=()):
        """conv5_3 [N,C,h,w] of a training blob [N,3,H,W] with autograd through the layers set_trainable named: plain torch
        ops (the fused in-place bias / ReLU kernels of `forward` are not differentiable); the frozen layers in front of
        the first trainable one run under no_grad.  The solver calls conv5_3.backward(d conv5_3).
        taps: layer names (the skip-connection detector's conv3_3, conv4_3, conv5_3); with them the result is
        (conv5_3, [the post-ReLU map of every tap, in `taps` order]), the maps part of autograd's graph and all in one
        memory format: the solver calls torch.autograd.backward(maps, d maps)."""
        tapped = {}
        x = torch.as_tensor(blob, dtype=torch.float32, device=self.device)
        if self.cl_compute:
            x = x.contiguous(memory_format=torch.channels_last)
        for layer in self.layers:
            if layer is None:
                x = F.max_pool2d(x, kernel_size=2, stride=2, ceil_mode=True)
                continue
            _, w, b = layer
            with torch.set_grad_enabled(bool(x.requires_grad or w.requires_grad)):
                x = F.relu(F.conv2d(x, w, b, padding=1))
            if layer[0] in taps:
                tapped[layer[0]] = x
        x = x if (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)) else x.contiguous()
        if not taps:
            return x
        missing = [n for n in taps if n not in tapped]
        if missing:
            raise ValueError("forward_train: no layer named %s" % ", ".join(missing))
        # one memory format for all (the trainer takes the maps in one): conv5_3's when every tap already has it
        cl = all(t.is_contiguous(memory_format=torch.channels_last) for t in tapped.values()) and not \
            all(t.is_contiguous() for t in tapped.values())
        fmt = torch.channels_last if cl else torch.contiguous_format
        return x, [tapped[n].contiguous(memory_format=fmt) for n in taps]

    @torch.no_grad()
    def normalize_output(self, blob):
        """Synthetic (random-init) weights only: rescale conv5_3's filters so the map has
        unit RMS on `blob` -- stands in for what training would have done, and keeps the
        synthetic head's scores and box deltas in a sane range."""
        rms = float(self.forward(blob).pow(2).mean().sqrt())
        name, w, b = self.layers[-1]
        w = w / rms
        if self.cl_compute:
            w = w.contiguous(memory_format=torch.channels_last)
        self.layers[-1] = (name, w, b / rms)
        return rms
