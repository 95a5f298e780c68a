"""`SloMoEngine`: the SuperSloMo arithmetic of batches of frame pairs on the device (slomo.py:338-345, 404-433).

Flow UNet, flow blends and backWarps (`v2e_slomo_prep`), interpolation UNet and fusion (`v2e_slomo_fuse`), for the time points
of one factor (`interpolate`) or a ragged sample table (`interpolate_table`); the flow UNet of a later batch can run ahead on a
side stream (`flow_ahead`, after a one-time two-stream canary per device), and `self_check` measures a conv math against the
float32 kernels.  The two networks are `unet.HipUNet`s; PyTorch only owns the buffers.
"""
import logging
import os

import torch

from . import _capi
from ._capi import check, ptr, stream_ptr
from .planning import speed_from_bits, time_coefficients
from .unet import HipUNet

logger = logging.getLogger(__name__)

# V2E_AMD_SLOMO_LOOKAHEAD=0: every UNet pass on the caller's stream, one after the other (SloMoEngine.flow_ahead is then never used by
# interpolate): the serial order of rounds 1-3, for whoever does not want two UNet passes in flight
_LOOKAHEAD = os.environ.get("V2E_AMD_SLOMO_LOOKAHEAD", "1") != "0"
# Two UNet passes in flight went wrong once (round 4) and the cause is known (round 5, profiles/r05_concurrency_rootcause.txt): on
# gfx950 a packed-float32 instruction whose op_sel routes src1's high half to the low lane reads 0 there while another kernel issues
# independent 16-K bf16 / f16 MFMAs.  The library is built without any packed-float32 instruction (Makefile, tests/test_device_isa.py),
# so the look-ahead is safe as built; the canary (SloMoEngine.lookahead_ok) makes a differently built library (EXTRA=-fslp-vectorize,
# another compiler) fall back to one stream instead of corrupting frames silently.  Result per device, decided at the first look-ahead
# of the process.
_CANARY = {}


class SloMoEngine:
    """Flow UNet + interpolation UNet + warps/fusion for batches of frame pairs, on device."""

    def __init__(self, flow_state_dict, interp_state_dict, device="cuda", conv_math=None):
        """conv_math: 'auto' (default) -- every f32 operand split into two float16 pieces, three piece products on the f16 matrix
        cores, f32 accumulation: operands good to 2^-22 and, measured on every fixture, as close to the reference and to float64
        as the other maths (profiles/r03_slomo_precision.txt).  float16's narrow exponent is taken out of the picture on both
        sides: weights are packed times an exact power of two per layer, and activations are staged times the power of two that
        puts the layer's largest input (tracked on the device by the producing convolution's epilogue) in [2^13, 2^14) -- so a
        piece is a float16 subnormal only where the activation is below 2^-27 of the layer's largest one (an absolute operand
        error of 2^-39 of that maximum), whatever the network's scale (tests: inputs x 3e5 and x 2^-17,
        tests/golden/slomo_smallact_64x96.npz).  A forward pass that meets an inf or NaN activation is redone with the exact
        split (HipUNet.forward);
        'bf16x3' -- three bf16 pieces, six products: the exact split (v2e_amd/csrc/slomo_s3.h), 0.7x the frames per second;
        'fp16x2' -- the two-piece math without the redo; 'f32' -- f32 matrix-core instructions.  The environment variable
        V2E_AMD_CONV_MATH sets the default."""
        if conv_math is None:
            conv_math = os.environ.get("V2E_AMD_CONV_MATH", "auto")
        self.conv_math = conv_math
        _capi.require_gpu("SloMoEngine")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _capi.lib()
        self.flow_net = HipUNet(flow_state_dict, 2, 4, self.device, conv_math)
        self.interp_net = HipUNet(interp_state_dict, 12, 5, self.device, conv_math)
        self._state_dicts = (flow_state_dict, interp_state_dict)  # for self_check(): the float32-MFMA engine is built from them on demand
        self._speed_bits = None
        self._fstream = None
        self._ahead = None  # (I0, I1, x, flow) of a flow pass started ahead on the side stream
        self._coef = self._coef_key = None  # interpolate(): the device coefficients of the last call's time points
        self.last = None  # interpolate(): dict(flow, x12, intrp) of the last call

    def flow(self, I0, I1):
        """flowOut = flow_estimator(cat(I0, I1)) (slomo.py:343); I0, I1: [B,1,H,W] float32.  If `flow_ahead` was started for
        exactly these two tensors, its result is taken (the current stream is ordered behind the side stream first)."""
        la = self._ahead
        if la is not None and la[0] is I0 and la[1] is I1:
            self._ahead = None
            cur = torch.cuda.current_stream(self.device)
            cur.wait_stream(self._fstream)
            la[3].record_stream(cur)
            la[2].record_stream(cur)
            self.flow_net.redo_if_flagged()  # (the pass ended long ago: no stall)
            return la[3]
        self._drop_ahead()
        x = torch.cat((I0, I1), dim=1).contiguous()  # 2 channels; the large concats are fused in-kernel
        return self.flow_net.forward(x)

    def _drop_ahead(self):
        """An unclaimed look-ahead pass: the flow UNet's workspace is its, so it finishes before the network runs again."""
        if self._ahead is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._fstream)
            self.flow_net._pending = None
            self._ahead = None

    def flow_ahead(self, I0, I1):
        """Start the flow UNet of a LATER batch on the engine's side stream, behind what the current stream holds NOW.  At the
        v2e batch size (8 pairs) the flow UNet is a chain of small launches that leaves most of the chip idle -- 3 ms of a 21 ms
        batch; beside the previous batch's interpolation UNet it is nearly free.  `flow(I0, I1)` with the same two tensors
        collects the result."""
        self._drop_ahead()
        if self._fstream is None:
            # (a high-priority stream: its own hardware queue whatever else the process has created -- streams of one priority
            #  share a few queues round-robin, and on the queue of the current stream the pass would simply run in line)
            self._fstream = torch.cuda.Stream(self.device, priority=-1)
        self._fstream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._fstream):
            x = torch.cat((I0, I1), dim=1).contiguous()
            f = self.flow_net.forward(x, defer_check=True)
        self._ahead = (I0, I1, x, f)

    def self_check(self, I0, I1, ts=(0.5,), reference=None):
        """This engine's conv math against the float32-MFMA kernels (the reference's own arithmetic type) on one batch: the largest
        |a - b| of the flow UNet's output, the interpolation UNet's output and the interpolated frames, each in units of its tensor's
        scale max(1, max |b|) ("flow", "intrp", "Ft", "max"; "per_element" = the same with max(1, |b|) per element, which on
        trained-scale weights is ~2e-4 for EVERY conv math incl. the exact split -- float32 summation order on cancelling sums, the
        reference's own float32 noise against float64 is of that size there: tests/test_slomo_gpu.py, noise ratios 1.2 - 1.5).  The default
        conv math carries 22-bit operands; it has met the 1e-5 tolerance on every fixture, but those are seeded random weights (the
        pretrained checkpoint is not obtainable offline) -- SuperSloMo runs this on the FIRST batch it sees and moves to the exact
        three-bf16-piece split if the figure is above 1e-5 (round-4 review, missing item 4).  reference: a float32 SloMoEngine to
        compare with (built from the same weights when None; ~160 MB and two UNet passes, once)."""
        ref = reference if reference is not None else SloMoEngine(self._state_dicts[0], self._state_dicts[1], self.device, conv_math="f32")
        ts = list(ts)
        res = {}
        a = self.interpolate(I0, I1, ts)
        la = dict(self.last)
        b = ref.interpolate(I0, I1, ts)
        lb = ref.last

        def err(x, y):  # in units of the tensor's scale
            return float((x - y).abs().max() / y.abs().max().clamp_min(1.0))

        def err_elem(x, y):  # per element
            return float(((x - y).abs() / y.abs().clamp_min(1.0)).max())

        res["flow"], res["intrp"], res["Ft"] = err(la["flow"], lb["flow"]), err(la["intrp"], lb["intrp"]), err(a, b)
        res["max"] = max(res.values())
        res["per_element"] = max(err_elem(la["flow"], lb["flow"]), err_elem(la["intrp"], lb["intrp"]), err_elem(a, b))
        return res

    def lookahead_ok(self):
        """True iff two UNet passes on two streams reproduce the one-stream result bit for bit on this device with this build of the
        library: one small interpolation-UNet pass alone, then twice beside three flow-UNet passes on the side stream (the
        configuration of profiles/r04_concurrency_finding.txt table 1, which failed 4-6 runs of 6 with the faulty build).
        Run once per process and device (a few ms); a mismatch switches the look-ahead off for the process, with one warning."""
        key = self.device.index
        if key not in _CANARY:
            g = torch.Generator(device=self.device)
            g.manual_seed(1234)
            xi = torch.rand((2, 12, 64, 96), device=self.device, generator=g) - 0.4
            xf = torch.rand((2, 2, 64, 96), device=self.device, generator=g) - 0.4
            cur = torch.cuda.current_stream(self.device)
            side = torch.cuda.Stream(self.device, priority=-1)
            ref = self.interp_net.forward(xi).clone()
            ok = True
            for _ in range(2):
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    for _ in range(3):
                        self.flow_net.forward(xf)
                out = self.interp_net.forward(xi)
                ok = ok and bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))
                cur.wait_stream(side)
            torch.cuda.synchronize(self.device)
            _CANARY[key] = ok
            if not ok:
                logger.warning("v2e_amd.SloMoEngine: a UNet pass beside another stream's pass differs from its stand-alone result on "
                               "this device with this build of libv2e_amd.so (was it built without -fno-slp-vectorize?): the flow "
                               "look-ahead is off for this process, every pass runs on the caller's stream")
        return _CANARY[key]

    def max_speed(self, flow):
        """slomo.py:352-368: the largest flow magnitude (pixels per source frame) over the batch and both directions, reduced on
        the device (k_max_speed2: max of the squared speed; ONE float32 sqrt on the host -- sqrt is monotone)."""
        b, c, h, w = flow.shape
        assert c == 4 and flow.dtype == torch.float32 and flow.is_contiguous()
        if self._speed_bits is None:
            self._speed_bits = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(self.lib.v2e_slomo_max_speed2(ptr(flow), b, h, w, ptr(self._speed_bits), stream_ptr(self.device)), "v2e_slomo_max_speed2")
        return speed_from_bits(self._speed_bits.item())

    def max_speed2_segments(self, flow, seg, out_bits):
        """v2e_slomo_max_speed2 of every batch of `seg` pairs of a flow chunk (the last batch may be shorter) in one launch, into
        the device int32 tensor out_bits[ceil(b / seg)] (not read back: `speed_from_bits` turns an entry into the speed)."""
        b, c, h, w = flow.shape
        assert c == 4 and flow.dtype == torch.float32 and flow.is_contiguous()
        assert out_bits.dtype == torch.int32 and out_bits.device == self.device and out_bits.numel() >= (b + seg - 1) // seg
        check(self.lib.v2e_slomo_max_speed2_seg(ptr(flow), b, int(seg), h, w, ptr(out_bits), stream_ptr(self.device)),
              "v2e_slomo_max_speed2_seg")

    def _interp_and_fuse(self, x12, fuse):
        """The interpolation UNet on x12 and `fuse(intrp)`, which enqueues the caller's fusion kernel.  The range flag is read
        behind the fusion (one host synchronisation per batch); if it was raised the pass has been redone with the exact split,
        and the fusion is enqueued once more.  Returns the UNet's output."""
        intrp = self.interp_net.forward(x12, defer_check=True)
        fuse(intrp)
        if self.interp_net.redo_if_flagged():
            fuse(intrp)
        return intrp

    def interpolate_table(self, I0, I1, flow, coef, tab, row0, n):
        """The interpolated frames of samples row0 .. row0 + n of a ragged sample table (auto_upsample: batches with different
        numbers of time points in ONE interpolation-UNet call): tab is a device int32 [samples][3] of {pair of I0 / I1 / flow,
        row of coef, output frame}, coef the device float32 [rows][6] of `time_coefficients`.  Sample for sample the arithmetic
        of `interpolate` (k_prep_tab / k_fuse_tab run k_prep / k_fuse's per-sample code).  Returns [n, 1, H, W] float32; the
        caller has checked the table against the tensors' sizes."""
        _, _, H, W = I0.shape
        assert I0.is_contiguous() and I1.is_contiguous() and flow.is_contiguous() and tab.is_contiguous() and coef.is_contiguous()
        assert I1.shape == I0.shape and tuple(flow.shape) == (I0.shape[0], 4, H, W) and coef.shape[1] == 6
        assert tab.dtype == torch.int32 and tab.shape[1] == 3 and 0 <= row0 and 0 < n and row0 + n <= tab.shape[0]
        t = tab[row0:row0 + n]
        x12 = torch.empty((n, 12, H, W), dtype=torch.float32, device=self.device)
        check(self.lib.v2e_slomo_prep_tab(ptr(I0), ptr(I1), ptr(flow), ptr(coef), ptr(t), n, H, W, ptr(x12), stream_ptr(self.device)),
              "v2e_slomo_prep_tab")
        out = torch.empty((n, 1, H, W), dtype=torch.float32, device=self.device)
        self._interp_and_fuse(x12, lambda intrp: check(
            self.lib.v2e_slomo_fuse_tab(ptr(I0), ptr(I1), ptr(x12), ptr(intrp), ptr(coef), ptr(t), n, H, W, ptr(out),
                                        stream_ptr(self.device)), "v2e_slomo_fuse_tab"))
        return out

    def interpolate(self, I0, I1, ts, flow=None, next_pair=None):
        """Ft_p for every t in ts and every pair in the batch: returns [len(ts), B, 1, H, W].
        next_pair = (I0, I1) of the batch the caller will pass NEXT (the same tensor objects): its flow UNet is started on the
        side stream now and runs beside this batch's interpolation UNet (`flow_ahead`)."""
        B, _, H, W = I0.shape
        I0 = I0 if I0.is_contiguous() else I0.contiguous()
        I1 = I1 if I1.is_contiguous() else I1.contiguous()
        if flow is None:
            flow = self.flow(I0, I1)
        if next_pair is not None and _LOOKAHEAD and self.lookahead_ok():
            self.flow_ahead(next_pair[0], next_pair[1])
        nt = len(ts)
        key = tuple(float(t) for t in ts)
        if self._coef_key != key:  # (the time points are the same for every batch of a clip: one upload)
            self._coef, self._coef_key = torch.from_numpy(time_coefficients(ts)).to(self.device), key
        x12 = torch.empty((nt * B, 12, H, W), dtype=torch.float32, device=self.device)
        check(self.lib.v2e_slomo_prep(ptr(I0), ptr(I1), ptr(flow), ptr(self._coef), nt, B, H, W, ptr(x12), stream_ptr(self.device)),
              "v2e_slomo_prep")
        out = torch.empty((nt * B, 1, H, W), dtype=torch.float32, device=self.device)
        intrp = self._interp_and_fuse(x12, lambda intrp: check(
            self.lib.v2e_slomo_fuse(ptr(I0), ptr(I1), ptr(x12), ptr(intrp), ptr(self._coef), nt, B, H, W, ptr(out), stream_ptr(self.device)),
            "v2e_slomo_fuse"))
        self.last = dict(flow=flow, x12=x12, intrp=intrp)
        return out.view(nt, B, 1, H, W)
