"""One SuperSloMo convolution layer inside guard bands, shared by the layer-by-layer GPU modules (test_slomo_fp16x2_gpu.py,
test_slomo_conv_tiles_gpu.py).  Not a test module and not a conftest; importing it does not touch the GPU."""
import ctypes as C

import numpy as np
import torch

from test_slomo_gpu import _rand

GUARD = 1 << 14           # floats of guard band on either side of every tensor a layer reads or writes
BAND_BITS = 0x7FC0BEEF    # what the output's bands hold (a NaN with a payload: any write shows, and so does a copy of it)


def source_hw(h, w, pre):
    """Height and width of x0 for an h x w output: pre 1 pools a 2h x 2w source, pre 2 upsamples an h/2 x w/2 one."""
    return (2 * h, 2 * w) if pre == 1 else ((h // 2, w // 2) if pre == 2 else (h, w))


def _case_tensors(case, pre=0):
    k, c0, c1, cout, n, h, w = case
    rng = np.random.Generator(np.random.PCG64(2077 + k * 1000 + c0 + 3 * c1 + cout + 7 * h + w))
    x0 = _rand(rng, (n, c0) + source_hw(h, w, pre))
    x1 = _rand(rng, (n, c1, h, w)) if c1 else None
    cin = c0 + c1
    wt = _rand(rng, (cout, cin, k, k), 1.5 / np.sqrt(cin * k * k))
    b = _rand(rng, (cout,), 0.1)
    return x0, x1, wt, b


class _Layer:
    """One convolution's weights packed for the three kernel families, run through v2e_conv2d_lrelu on tensors that live inside
    larger device buffers: NaN around the inputs, sentinel bands around the output (checked after every launch).  A layer whose
    cout is no multiple of 32 (the 4- / 5-channel head) has no split-operand weights and runs as "f32" only."""

    def __init__(self, wt, b):
        from v2e_amd import _capi
        from v2e_amd.slomo import weight_scale_log2
        self.lib, self.check = _capi.lib(), _capi.check
        self.dev = torch.device("cuda")
        self.co, self.ci, self.k, _ = wt.shape
        co, ci, k = self.co, self.ci, self.k
        s = self._stream()
        tw = torch.from_numpy(wt).to(self.dev)
        self.tb = torch.from_numpy(b).to(self.dev)
        self.wp = torch.empty((ci, k, k, co), dtype=torch.float32, device=self.dev)
        self.check(self.lib.v2e_pack_conv_weight(C.c_void_p(tw.data_ptr()), C.c_void_p(self.wp.data_ptr()), co, ci, k, s), "pack")
        self.w3 = self.w2 = None
        if co % 32 == 0:
            cpad = (ci + 15) // 16 * 16
            self.w3 = torch.empty(cpad * k * k * co * 6, dtype=torch.uint8, device=self.dev)
            self.check(self.lib.v2e_pack_conv_weight_s3(C.c_void_p(tw.data_ptr()), C.c_void_p(self.w3.data_ptr()), co, ci, k, s), "pack_s3")
            # the product's rule for the weights' power of two (HipUNet calls the same function on the same number)
            self.sl2 = weight_scale_log2(float(tw.abs().max()))
            self.w2 = torch.empty(cpad * k * k * co * 4, dtype=torch.uint8, device=self.dev)
            self.check(self.lib.v2e_pack_conv_weight_h2(C.c_void_p(tw.data_ptr()), C.c_void_p(self.w2.data_ptr()), co, ci, k, self.sl2, s),
                       "pack_h2")
        torch.cuda.synchronize()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _desc(self, math):
        from v2e_amd._capi import ConvDesc
        d = ConvDesc(self.wp.data_ptr(), self.tb.data_ptr(), self.ci, self.co, self.k)
        if math == "bf16x3":
            d.weight_s3, d.split_kind = self.w3.data_ptr(), 0
        elif math == "fp16x2":
            d.weight_s3, d.split_kind = self.w2.data_ptr(), 2 | (self.sl2 << 8)
        else:
            assert math == "f32"
        return d

    def _banded_input(self, x):
        buf = torch.full((GUARD + x.size + GUARD,), float("nan"), dtype=torch.float32, device=self.dev)
        view = buf[GUARD:GUARD + x.size].view(x.shape)
        view.copy_(torch.from_numpy(x))
        return buf, view

    def _presplit(self, t0):
        """v2e_split3_nchw of a device tensor into the middle of a byte buffer of 0xFF (every bf16 of the bands is a NaN)."""
        n, c, h, w = t0.shape
        nb, gb = t0.numel() * 6, GUARD * 4
        buf = torch.full((gb + nb + gb,), 0xFF, dtype=torch.uint8, device=self.dev)
        xs = buf[gb:gb + nb]
        self.check(self.lib.v2e_split3_nchw(C.c_void_p(t0.data_ptr()), C.c_void_p(xs.data_ptr()), n, c, h, w, self._stream()), "split3")
        torch.cuda.synchronize()
        assert bool((buf[:gb] == 0xFF).all()) and bool((buf[gb + nb:] == 0xFF).all()), "the split wrote outside its buffer"
        return buf, xs, xs.clone()

    def run(self, x0, x1, math, pre=0):
        """pre as v2e_conv2d_lrelu takes it: 1: x0 is [n, c0, 2h, 2w] (fused avg_pool2d), 2: [n, c0, h/2, w/2] (fused bilinear x2),
        3: x0 is [n, c0, h, w] and the layer is handed its three bf16 pieces, split here by v2e_split3_nchw."""
        n = x0.shape[0]
        h, w = x0.shape[2:]
        if pre == 1:
            h, w = h // 2, w // 2
        elif pre == 2:
            h, w = 2 * h, 2 * w
        b0, t0 = self._banded_input(x0)
        b1, t1 = self._banded_input(x1) if x1 is not None else (None, None)
        src = t0
        if pre == 3:
            sbuf, src, skeep = self._presplit(t0)
        ny = n * self.co * h * w
        ybuf = torch.full((GUARD + ny + GUARD,), BAND_BITS, dtype=torch.int32, device=self.dev).view(torch.float32)
        y = ybuf[GUARD:GUARD + ny].view(n, self.co, h, w)
        y.fill_(float("nan"))
        d = self._desc(math)
        self.check(self.lib.v2e_conv2d_lrelu(C.c_void_p(src.data_ptr()), x0.shape[1], C.c_void_p(t1.data_ptr()) if t1 is not None else None,
                                             0 if x1 is None else x1.shape[1], pre, C.byref(d), C.c_void_p(y.data_ptr()), n, h, w,
                                             self._stream()), "conv")
        torch.cuda.synchronize()
        bits = ybuf.view(torch.int32)
        assert bool((bits[:GUARD] == BAND_BITS).all()), "%s wrote in front of its output" % math
        assert bool((bits[GUARD + ny:] == BAND_BITS).all()), "%s wrote behind its output" % math
        for buf, x in ((b0, x0), (b1, x1)):   # and the inputs and their surroundings are as they were
            if buf is not None:
                assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + x.size:]).all())
                assert np.array_equal(buf[GUARD:GUARD + x.size].cpu().numpy(), x.ravel())
        if pre == 3:
            gb = GUARD * 4
            assert bool((sbuf[:gb] == 0xFF).all()) and bool((sbuf[gb + skeep.numel():] == 0xFF).all()) and bool((src == skeep).all())
        return y.cpu().numpy()
