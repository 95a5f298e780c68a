"""`HipUNet`: one UNet of the SuperSloMo model (model.py:158-300) on the convolution kernels of libv2e_amd.so.

The weights are repacked [Cin][k][k][Cout] in HBM once, per layer and conv math, into the `ConvDesc` array `v2e_unet_forward`
walks; a forward pass is one library call on the current stream, and under conv_math 'auto' a pass that met an inf / NaN
activation is redone with the exact split (`redo_if_flagged`).  `workspace_tensors`, `range_slots` and `walk_layers` are for
tests and diagnosis (v2e_amd.check_ckpt).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from ._capi import ConvDesc, check, ptr, stream_ptr

# forward order of the 23 convolutions of model.UNet (model.py:184-196, 198-226)
UNET_LAYERS = (["conv1", "conv2"] + ["down%d.conv%d" % (d, c) for d in range(1, 6) for c in (1, 2)] +
               ["up%d.conv%d" % (u, c) for u in range(1, 6) for c in (1, 2)] + ["conv3"])


def weight_scale_log2(wmax):
    """The exponent a two-float16-piece layer's weights are packed times 2^ of (v2e_pack_conv_weight_h2, ConvDesc.split_kind >> 8):
    the exact power of two that puts the layer's largest weight `wmax` in [2^12, 2^13) -- no piece of a weight that matters is a
    float16 subnormal, nothing overflows (65504) -- kept within 0 .. 40 (v2e_amd/csrc/slomo.hip act_scale: the convolution's
    epilogue divides it out again together with the activations' power of two, in one exact multiply)."""
    if not wmax > 0.0:
        return 0
    return max(0, min(40, 12 - math.frexp(wmax)[1] + 1))


class HipUNet:
    """One UNet's weights, repacked [Cin][k][k][Cout] in HBM, and its forward pass."""

    def __init__(self, state_dict, cin, cout, device, conv_math="bf16x3"):
        if conv_math not in ("auto", "bf16x3", "f32", "fp16x2"):
            raise ValueError("conv_math must be 'auto' (two float16 pieces and three products per multiply -- half the "
                             "matrix-core work, products good to ~2^-21; operands are staged times powers of two that keep them in "
                             "float16's normal range, and a forward pass that meets an inf / NaN activation is redone with the exact "
                             "split), 'bf16x3' (f32 operands split exactly into three "
                             "bf16 pieces, six piece products on the bf16 matrix cores, f32 accumulation), 'fp16x2' (the two-piece "
                             "math without the guard) or 'f32' (f32 matrix-core instructions)")
        self.conv_math = conv_math
        self.lib = _capi.lib()
        self.device = torch.device(device)
        self.cin, self.cout = cin, cout
        self._keep = []
        self.fallbacks = 0  # conv_math 'auto': forward passes redone with the exact split
        descs = (ConvDesc * 23)()        # what forward() runs first
        descs_exact = (ConvDesc * 23)() if conv_math == "auto" else None
        fast_ok = True
        for i, name in enumerate(UNET_LAYERS):
            fast_ok &= self._pack_layer(i, name, state_dict, descs, descs_exact)
        torch.cuda.synchronize(self.device)
        assert descs[0].cin == cin and descs[22].cout == cout
        self.descs, self.descs_exact = descs, descs_exact
        if conv_math == "auto" and not fast_ok:  # a weight beyond float16: the exact split throughout
            self.descs, self.descs_exact = descs_exact, None
        self._flag = torch.zeros(1, dtype=torch.int32, device=self.device) if self.descs_exact is not None else None
        self._ws = None
        self._pending = None

    def _pack_layer(self, i, name, state_dict, descs, descs_exact):
        """Layer i's weights and bias on the device, packed for this conv math, into descs[i] (and descs_exact[i]).  False: the
        layer has a weight beyond float16, so 'auto' cannot run it on two float16 pieces."""
        conv_math, stream = self.conv_math, stream_ptr(self.device)
        w = state_dict[name + ".weight"].detach().to(self.device, torch.float32).contiguous()
        b = state_dict[name + ".bias"].detach().to(self.device, torch.float32).contiguous()
        co, ci, kh, kw = w.shape
        assert kh == kw
        wp = torch.empty((ci, kh, kw, co), dtype=torch.float32, device=self.device)
        check(self.lib.v2e_pack_conv_weight(ptr(w), ptr(wp), co, ci, kh, stream), "v2e_pack_conv_weight")
        self._keep += [wp, b]
        for d in (descs, descs_exact):
            if d is not None:
                d[i].weight, d[i].bias = wp.data_ptr(), b.data_ptr()
                d[i].weight_s3, d[i].split_kind = None, 0
                d[i].cin, d[i].cout, d[i].ksize = ci, co, kh
        splittable = co % 32 == 0 and (ci % 16 == 0 or (kh == 7 and ci >= 8))
        fast_ok = True
        if conv_math in ("auto", "fp16x2") and splittable:
            # an exact power of two that puts the layer's largest weight in [2^12, 2^13): no piece of a weight that matters
            # is a float16 subnormal, nothing overflows (65504); the kernel divides it out again
            wmax = float(w.abs().max())
            if not wmax < 65504.0:
                if conv_math == "fp16x2":
                    raise ValueError("conv_math='fp16x2': layer %s has a weight of magnitude %g, beyond float16" % (name, wmax))
                fast_ok = False
            else:
                sl2 = weight_scale_log2(wmax)
                w2 = torch.empty((ci + 15) // 16 * 16 * kh * kw * co * 4, dtype=torch.uint8, device=self.device)
                check(self.lib.v2e_pack_conv_weight_h2(ptr(w), ptr(w2), co, ci, kh, sl2, stream), "v2e_pack_conv_weight_h2")
                self._keep.append(w2)
                descs[i].weight_s3 = w2.data_ptr()
                descs[i].split_kind = 2 | (sl2 << 8)
        if conv_math in ("auto", "bf16x3") and splittable:
            w3 = torch.empty((ci + 15) // 16 * 16 * kh * kw * co * 6, dtype=torch.uint8, device=self.device)
            check(self.lib.v2e_pack_conv_weight_s3(ptr(w), ptr(w3), co, ci, kh, stream), "v2e_pack_conv_weight_s3")
            self._keep.append(w3)
            d = descs_exact if conv_math == "auto" else descs
            d[i].weight_s3, d[i].split_kind = w3.data_ptr(), 0
        return fast_ok

    def _run(self, descs, x, out):
        """v2e_unet_forward of x into out with the layer descriptors `descs`, on the current stream."""
        n, c, h, w = x.shape
        check(self.lib.v2e_unet_forward(ptr(x), c, descs, self.cout, ptr(out), n, h, w, ptr(self._ws), stream_ptr(self.device)),
              "v2e_unet_forward")

    def forward(self, x, out=None, defer_check=False):
        """One forward pass on the current stream.  defer_check (conv_math 'auto'): do not read the range flag back now -- the
        caller enqueues whatever follows and calls `redo_if_flagged()` afterwards (one host synchronisation per batch instead of
        one per network; the flow UNet of a later batch can run on another stream meanwhile)."""
        n, c, h, w = x.shape
        assert c == self.cin and x.dtype == torch.float32 and x.is_contiguous()
        need = int(self.lib.v2e_unet_workspace_bytes(n, h, w, c))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty((n, self.cout, h, w), dtype=torch.float32, device=self.device)
        self._pending = None
        if self._flag is None:
            self._run(self.descs, x, out)
            return out
        # conv_math 'auto': the two-float16-piece convolutions report an inf / NaN activation (finite ones are scaled into
        # float16's range inside the kernels); such a pass is redone with the exact three-bf16-piece weights (one 4-byte
        # read-back per forward pass)
        self._flag.zero_()
        check(self.lib.v2e_conv_set_range_flag(ptr(self._flag)), "v2e_conv_set_range_flag")
        try:
            self._run(self.descs, x, out)
        finally:
            self.lib.v2e_conv_set_range_flag(None)
        self._pending = (x, out)
        if not defer_check:
            self.redo_if_flagged()
        return out

    def redo_if_flagged(self):
        """Read the range flag of the last forward pass (on the CURRENT stream, which must be ordered behind that pass) and redo
        the pass with the exact split if it was raised.  Returns True when it was redone (what consumed `out` must be redone too)."""
        if self._pending is None:
            return False
        x, out = self._pending
        self._pending = None
        if int(self._flag.item()) == 0:
            return False
        self.fallbacks += 1
        self._run(self.descs_exact, x, out)
        return True

    def workspace_tensors(self, n, h, w):
        """Read-only views of what the last forward pass of an [n, cin, h, w] input left in the workspace, by the layout of
        v2e_unet_forward (csrc/slomo.hip: s1 s2 s3 s4 s5 | tA tB tU | range slots): the skip tensors "s1" .. "s5" (the outputs of
        conv2 and down1 .. down4.conv2) and the two trunk tensors no later layer overwrote, "tA" (up5.conv1) and "tB" (up5.conv2).
        For tests and diagnosis; the views alias the workspace and change with the next pass."""
        hw = h * w
        f = self._ws[:int(self.lib.v2e_unet_workspace_bytes(n, h, w, self.cin))].view(torch.float32)
        out, off = {}, 0
        for k, c in enumerate((32, 64, 128, 256, 512)):
            hh, ww = h >> k, w >> k
            out["s%d" % (k + 1)] = f[off:off + n * c * hh * ww].view(n, c, hh, ww)
            off += n * c * hh * ww
        for name in ("tA", "tB"):
            out[name] = f[off:off + n * 32 * hw].view(n, 32, h, w)
            off += n * 32 * hw
        return out

    def range_slots(self, n, h, w):
        """The 32 range slots of the last forward pass of an [n, cin, h, w] input, as uint32 (float32 bit patterns): [0] the largest
        |input|, [1 + i] the largest |output| of convolution i (UNET_LAYERS order).  Written only while some layer runs on two
        float16 pieces (conv_math 'auto' / 'fp16x2'); the last convolution's slot has no reader, and the 4- / 5-channel conv3 kernel
        does not write it."""
        off = n * h * w * (32 + 16 + 8 + 4 + 2 + 32 + 32 + 64) * 4
        torch.cuda.synchronize(self.device)
        return self._ws[off:off + 128].cpu().numpy().view(np.uint32).copy()

    def walk_layers(self, x, inputs_from=None):
        """The UNet layer by layer through v2e_conv2d_lrelu (model.py:198-226: avg_pool2d and the bilinear x2 fused into the consuming
        convolution's loader, the skip concatenation as its second input): [(name, (x0, x1, pre), y)] for the 23 convolutions.
        inputs_from = the list another network's walk returned: every layer then runs on THAT walk's inputs (an isolated layer-by-layer
        comparison of two conv maths; v2e_amd.check_ckpt).  A two-float16-piece layer called this way stages its activations
        unscaled (include/v2e_amd.h): the isolated figure is an upper bound for what the same layer does inside v2e_unet_forward."""
        from .synth import unet_layer_shapes
        names = [q[0] for q in unet_layer_shapes(self.cin, self.cout)]
        stream = stream_ptr(self.device)
        out = []

        def conv(i, x0, x1, pre, h, w):
            if inputs_from is not None:
                x0, x1, pre = inputs_from[i][1]
            d = self.descs[i]
            y = torch.empty((x0.shape[0], d.cout, h, w), dtype=torch.float32, device=self.device)
            check(self.lib.v2e_conv2d_lrelu(ptr(x0), int(x0.shape[1]), ptr(x1), 0 if x1 is None else int(x1.shape[1]), pre, C.byref(d),
                                            ptr(y), int(x0.shape[0]), h, w, stream), "v2e_conv2d_lrelu")
            out.append((names[i], (x0, x1, pre), y))
            return y

        n, c, h, w = x.shape
        cur = conv(1, conv(0, x, None, 0, h, w), None, 0, h, w)
        skips = [cur]
        for d in range(5):
            h, w = h // 2, w // 2
            cur = conv(3 + 2 * d, conv(2 + 2 * d, cur, None, 1, h, w), None, 0, h, w)
            skips.append(cur)
        for u in range(5):
            h, w = h * 2, w * 2
            cur = conv(13 + 2 * u, conv(12 + 2 * u, cur, None, 2, h, w), skips[4 - u], 0, h, w)
        conv(22, cur, None, 0, h, w)
        return out
