"""Device-resident video -> events pipeline (BASELINE configs[2]).

The reference's v2e.py runs its three stages through the filesystem: source frames as .npy,
`SuperSloMo.interpolate` writes 8-bit PNGs (slomo.py:436-444), v2e.py reads them back
(v2e.py:832) and calls `EventEmulator.generate_events` per frame.  `VideoToEvents` keeps every
frame in HBM and produces the same uint8 frames for the emulator:

  source uint8 [N,H,W] --Pillow-exact LANCZOS--> [N,h,w] --/255 - mean--> SloMo (HIP, all U time
  points per batch) --(+mean)*255, byte truncation--> uint8 --Pillow-exact BILINEAR--> [P*U,H,W]
  --> emulator (HIP, Philox, one device-resident run)

One clip over several GPUs: `VideoToEvents.run(..., group=)` shards the SuperSloMo stage by source pairs over the ranks of a process
group and funnels the uint8 frames, in order, to the rank that owns the emulator state.

Frame order and times follow slomo.py:391-400, 441 and v2e.py:786-797: output frame b*U + k of a batch has
interpTime pair + k/U (in source frame intervals), and v2e.py stretches the interpTimes so that they SPAN the processed
duration of the source clip: t = interpTime * (N_src - 1) * interval / (max(interpTimes) - min(interpTimes)).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from ._capi import check
from .emulator import default_event_capacity
from .resample import coeffs_8bpc
from .slomo import speed_from_bits, time_coefficients


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class DeviceResampler:
    """Pillow-exact uint8 resize [n,ih,iw] -> [n,oh,ow] on device (tables cached on device)."""

    def __init__(self, in_hw, out_hw, filt, device):
        self.ih, self.iw = in_hw
        self.oh, self.ow = out_hw
        self.device = torch.device(device)
        self.lib = _capi.lib()
        self.hb = self.hk = self.vb = self.vk = None
        self.hks = self.vks = 0
        if self.ow != self.iw:
            b, k = coeffs_8bpc(self.iw, self.ow, filt)
            self.hb, self.hk, self.hks = torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device), k.shape[1]
        if self.oh != self.ih:
            b, k = coeffs_8bpc(self.ih, self.oh, filt)
            self.vb, self.vk, self.vks = torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device), k.shape[1]

    def __call__(self, x):
        assert x.dtype == torch.uint8 and x.is_contiguous() and tuple(x.shape[-2:]) == (self.ih, self.iw)
        n = x.numel() // (self.ih * self.iw)
        out = torch.empty((n, self.oh, self.ow), dtype=torch.uint8, device=self.device)
        tmp = torch.empty((n, self.ih, self.ow), dtype=torch.uint8, device=self.device) if (self.ow != self.iw and self.oh != self.ih) else None
        s = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        check(self.lib.v2e_resample_u8(_ptr(x), _ptr(tmp), _ptr(out), n, self.ih, self.iw, self.oh, self.ow, _ptr(self.hb),
                                       _ptr(self.hk), self.hks, _ptr(self.vb), _ptr(self.vk), self.vks, s), "v2e_resample_u8")
        return out


def interp_times(n_src, U, batch_size=None, factors=None):
    """The un-normalised interpTimes of slomo.interpolate (slomo.py:388-400): per batch of `batch_size` pairs (None: one batch)
    inputFrameCounter + k * (1 / U_b), k < U_b * pairs in the batch.  factors: U_b per batch (auto_upsample); None: U for all."""
    npairs = n_src - 1
    bs = npairs if not batch_size else int(batch_size)
    starts = range(0, npairs, bs)
    factors = [U] * len(starts) if factors is None else [int(u) for u in factors]
    if len(factors) != len(starts):
        raise ValueError("%d upsampling factors for %d batches" % (len(factors), len(starts)))
    return np.concatenate([_batch_interp_times(b0, u, min(bs, npairs - b0)) for b0, u in zip(starts, factors)])


def _batch_interp_times(b0, u, nb):
    """The interpTimes of one batch of nb pairs starting at pair b0 with factor u (slomo.py:393-398)."""
    return b0 + np.array(range(u * nb)) * (1 / u)


def interp_frame_times(n_src, U, src_frame_interval_s, batch_size=None, factors=None):
    """Times of the interpolated frames as v2e.py computes them, operation for operation: interpTimes are built per batch of
    `batch_size` pairs as inputFrameCounter + k * (1 / U) (`interp_times`; factors: one U per batch, auto_upsample), then
    normalised to the processed duration of the source clip (v2e.py:786-797: f = srcVideoRealProcessedDuration / (max(interpTimes) -
    min(interpTimes)); interpTimes = f * interpTimes)."""
    interp = interp_times(n_src, U, batch_size, factors)
    duration = (n_src - 1) * float(src_frame_interval_s)
    f = duration / (np.max(interp) - np.min(interp))
    return f * interp


def auto_upsampling_factor(speed_bits, minimum=None):
    """slomo.py:352-379: a batch's upsampling factor from the float32 bits of its largest squared flow speed
    (v2e_slomo_max_speed2): ceil of the float32 sqrt, at least `minimum` (None: no minimum) and at least 2.  A NaN flow raises
    ValueError, as int(np.ceil(nan)) does in the reference."""
    speed = speed_from_bits(speed_bits)
    if speed != speed:
        raise ValueError("auto_upsample: the flow of a batch is NaN, so its upsampling factor is undefined")
    u = int(np.ceil(speed))
    if minimum is not None and minimum > u:
        u = minimum
    if u < 2:
        u = 2
    return u


def auto_sample_table(factors, n_pairs, batch_size):
    """The samples of a flow chunk of n_pairs pairs whose batches of batch_size pairs have the upsampling factors `factors`, in v2e
    frame order (slomo.py:441: batch offset + U_b * pair in batch + k): (ts, tab, cuts) with ts the time points (k + 0.5) / U
    (slomo.py:405) of every distinct U, tab one (pair, row of ts, output frame) per sample, cuts the batches' first samples and the
    end.  Every entry is checked against the sizes: the kernels index with them."""
    if (len(factors) - 1) * batch_size >= n_pairs or len(factors) * batch_size < n_pairs:
        raise ValueError("%d factors for %d pairs in batches of %d" % (len(factors), n_pairs, batch_size))
    ts, row0 = [], {}
    for u in sorted(set(factors)):
        row0[u] = len(ts)
        ts += [(k + 0.5) / u for k in range(u)]
    tab, cuts = [], [0]
    for j, u in enumerate(factors):
        b0, b1 = j * batch_size, min((j + 1) * batch_size, n_pairs)
        for i in range(b0, b1):
            for k in range(u):
                tab.append((i, row0[u] + k, cuts[-1] + u * (i - b0) + k))
        cuts.append(len(tab))
    n = len(tab)
    assert all(0 <= p < n_pairs and 0 <= r < len(ts) and 0 <= f < n for p, r, f in tab)
    return ts, tab, cuts


# Samples per interpolation-UNet call of the auto_upsample path: consecutive batches (each with its own U_b) are packed into calls
# of at most this many samples.  0: one call per batch (no packing; A/B runs).  DESIGN.md section 5 has the measurement.
AUTO_SAMPLES_PER_CALL = 128


def flow_chunk_pairs(batch_size):
    """Pairs per flow-UNet call of `upsample` and `_upsample_auto`: whole interpolation batches, as many as fit in 64 pairs (one at least)."""
    return int(batch_size) * max(1, 64 // int(batch_size))


def stream_chunks(n_pairs, batch_size, chunk_pairs=None):
    """The chunks [(p0, p1)] of source pairs that `VideoToEvents.run_stream` takes in turn.  chunk_pairs must be a positive multiple
    of the flow chunk (`flow_chunk_pairs`; default four of them): every flow-UNet call, interpolation call and auto_upsample sample
    packing of a chunk is then the very call the unchunked `upsample` makes, which keeps the frames bit-identical under the conv maths
    that scale activations per call.  A clip shorter than one chunk is one chunk."""
    fc = flow_chunk_pairs(batch_size)
    if chunk_pairs is None:
        chunk_pairs = 4 * fc
    if isinstance(chunk_pairs, bool) or int(chunk_pairs) != chunk_pairs or chunk_pairs <= 0 or int(chunk_pairs) % fc:
        raise ValueError("chunk_pairs must be a positive multiple of the flow chunk of %d pairs (batch_size %d), got %r"
                         % (fc, int(batch_size), chunk_pairs))
    chunk_pairs, n_pairs = int(chunk_pairs), int(n_pairs)
    return [(p0, min(p0 + chunk_pairs, n_pairs)) for p0 in range(0, n_pairs, chunk_pairs)]


def last_flow_chunk(n_pairs, batch_size):
    """The pairs (f0, n_pairs) of the clip's last flow-UNet call in `upsample` / `_upsample_auto`."""
    fc = flow_chunk_pairs(batch_size)
    return (int(n_pairs) - 1) // fc * fc, int(n_pairs)


def stream_time_scale(n_src, src_frame_interval_s, batch_size, last_factor):
    """The factor f of `interp_frame_times` (v2e.py:786-797: processed duration / (max(interpTimes) - min(interpTimes))) from the
    factor of the clip's LAST batch alone: interpTimes rise batch after batch, so the maximum is the last batch's last time, the
    minimum the first batch's first, 0."""
    npairs = int(n_src) - 1
    bs = int(batch_size)
    b0 = (npairs - 1) // bs * bs
    last = _batch_interp_times(b0, int(last_factor), npairs - b0)
    duration = npairs * float(src_frame_interval_s)
    return duration / (np.max(last) - 0.0)


def chunk_frame_times(p0, p1, batch_size, factors, scale):
    """Times of the interpolated frames of source pairs [p0, p1) (p0 a multiple of batch_size), `factors` the U of each of their
    batches: the slice of `interp_frame_times` for the whole clip that belongs to them, bit for bit (`scale`: stream_time_scale)."""
    bs = int(batch_size)
    starts = range(p0, p1, bs)
    if p0 % bs or len(factors) != len(starts):
        raise ValueError("%d factors for pairs [%d, %d) in batches of %d" % (len(factors), p0, p1, bs))
    parts = [_batch_interp_times(b0, int(u), min(bs, p1 - b0)) for b0, u in zip(starts, factors)]
    return scale * np.concatenate(parts)


def stream_source_shape(frames_u8):
    """(N, H, W) of the source clip of `run_stream`: a uint8 [N,H,W] torch tensor (device or host) or numpy array, N >= 2."""
    if torch.is_tensor(frames_u8):
        ok = frames_u8.dtype == torch.uint8
    elif isinstance(frames_u8, np.ndarray):
        ok = frames_u8.dtype == np.uint8
    else:
        raise TypeError("frames_u8 must be a torch tensor or a numpy array, got %s" % type(frames_u8).__name__)
    if not ok:
        raise ValueError("frames_u8 must be uint8, got %s" % frames_u8.dtype)
    if frames_u8.ndim != 3:
        raise ValueError("frames_u8 must be [N,H,W], got shape %s" % (tuple(frames_u8.shape),))
    N, H, W = (int(v) for v in frames_u8.shape)
    if N < 2 or H < 1 or W < 1:
        raise ValueError("frames_u8 needs at least two frames of at least one pixel, got shape %s" % ((N, H, W),))
    return N, H, W


class VideoToEvents:
    """SuperSloMo upsampling + DVS emulation of one clip without leaving HBM."""
    auto_upsample = False  # (also for subclasses that set their own attributes instead of calling __init__)

    def __init__(self, slomo_engine, emulator, upsampling_factor, batch_size=8, mean=0.428, auto_upsample=False):
        """auto_upsample=True (v2e's default mode, slomo.py:352-379): every batch of `batch_size` source pairs gets its own factor
        U_b = max(ceil(largest flow speed of the batch), upsampling_factor or 0, 2); upsampling_factor is then the minimum and may
        be None.  After a run: `upsampling_factors` (per batch), `interpTimes` (un-normalised, what slomo.interpolate returns) and
        `avg_upsampling_factor`."""
        self.eng = slomo_engine
        self.emu = emulator
        self.auto_upsample = bool(auto_upsample)
        if self.auto_upsample:
            self.U = None if upsampling_factor is None else int(upsampling_factor)
        else:
            self.U = int(upsampling_factor)
        self.batch_size = int(batch_size)
        self.mean = float(mean)
        self.lib = _capi.lib()
        self._rs_in = self._rs_out = None
        self.samples_per_call = int(os.environ.get("V2E_AMD_AUTO_SAMPLES_PER_CALL", AUTO_SAMPLES_PER_CALL))
        self.upsampling_factors = self.interpTimes = self.avg_upsampling_factor = None
        self.host_syncs = 0  # auto_upsample: factor read-backs of the last upsample() (one per flow chunk)
        self.dvs_frames = self.dvs_frame_times = None  # run / run_stream with renderer=: the DVS video of the last clip

    def upsample(self, frames_u8):
        """frames_u8: device uint8 [N,H,W] -> device uint8 [(N-1)*U, H, W], the frames the reference's
        interpolate() would have written as PNGs (in order).  auto_upsample: sum over batches of U_b * pairs frames."""
        if self.auto_upsample:
            return self._upsample_auto(frames_u8)
        x, h, w = self._normalised_input(frames_u8)
        return self._upsample_fixed(x, h, w, tuple(frames_u8.shape[1:]))

    def _upsample_fixed(self, x, h, w, out_hw):
        """Fixed U from the normalised input x [N,1,h,w] (`_normalised_input`): uint8 [(N-1)*U, H, W]."""
        dev = self.eng.device
        N = int(x.shape[0])
        H, W = out_hw
        s = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        U = self.U
        ts = [(k + 0.5) / U for k in range(U)]
        out = torch.empty(((N - 1) * U, H, W), dtype=torch.uint8, device=dev)
        # the flow UNet sees up to 64 pairs at a time (its small levels fill the GPU only with many samples; a pair's
        # flow does not depend on what else is in the batch), the interpolation UNet U x batch_size samples
        fc = flow_chunk_pairs(self.batch_size)  # pairs per flow-UNet call: whole interpolation batches
        flow, f0, f1 = None, 0, 0
        for b0 in range(0, N - 1, self.batch_size):
            b1 = min(b0 + self.batch_size, N - 1)
            B = b1 - b0
            if b0 >= f1:
                f0, f1 = b0, min(b0 + fc, N - 1)
                flow = self.eng.flow(x[f0:f1], x[f0 + 1:f1 + 1])
            Ft = self.eng.interpolate(x[b0:b1], x[b0 + 1:b1 + 1], ts, flow=flow[b0 - f0:b1 - f0].contiguous())  # [U,B,1,h,w]
            q = torch.empty((B * U, h, w), dtype=torch.uint8, device=dev)
            check(self.lib.v2e_f32_to_u8_trunc(_ptr(Ft), _ptr(q), U, B, h * w, self.mean, 1, s()), "v2e_f32_to_u8_trunc")
            out[b0 * U:b1 * U] = self._rs_out(q)
        return out

    def _normalised_input(self, frames_u8):
        """LANCZOS to the network size (dataloader.py:122-123, 142) and ToTensor + Normalize: ([N,1,h,w] float32, h, w)."""
        dev = self.eng.device
        N, H, W = frames_u8.shape
        dim = (int(W / 32) * 32, int(H / 32) * 32)  # (w, h), dataloader.py:122-123
        w, h = dim
        if self._rs_in is None or (self._rs_in.ih, self._rs_in.iw) != (H, W):
            self._rs_in = DeviceResampler((H, W), (h, w), "lanczos", dev)
            self._rs_out = DeviceResampler((h, w), (H, W), "bilinear", dev)
        small = self._rs_in(frames_u8.contiguous())
        x = torch.empty((N, 1, h, w), dtype=torch.float32, device=dev)
        check(self.lib.v2e_u8_to_f32_norm(_ptr(small), _ptr(x), small.numel(), self.mean,
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "v2e_u8_to_f32_norm")
        return x, h, w

    def _upsample_auto(self, frames_u8):
        """auto_upsample: the flow UNet runs on chunks of up to 64 pairs (whole batches); one launch gives every batch's largest
        squared speed, read back ONCE per chunk -- behind the next chunk's flow UNet, which is enqueued first.  The chunk's samples
        (v2e frame order: batch offset + U_b * pair + k) go through the interpolation UNet in calls of up to `samples_per_call`
        samples that may span batches with different U_b (k_prep_tab / k_fuse_tab), and each sample is truncated straight into its
        frame slot, so the chunk's frames are one contiguous range for the BILINEAR resize."""
        dev = self.eng.device
        N = int(frames_u8.shape[0])
        P, bs = N - 1, self.batch_size
        if P < 1:
            raise ValueError("auto_upsample needs at least two source frames, got %d" % N)
        x, h, w = self._normalised_input(frames_u8)
        self.host_syncs = 0
        out, factors = self._upsample_auto_x(x, h, w)
        self.upsampling_factors = factors
        self.interpTimes = interp_times(N, None, bs, factors)
        self.avg_upsampling_factor = sum(factors) / len(factors)
        return out

    def _upsample_auto_x(self, x, h, w):
        """auto_upsample from the normalised input x [N,1,h,w]: (uint8 frames, the factor of every batch).  Adds its factor
        read-backs to host_syncs."""
        dev = self.eng.device
        P, bs = int(x.shape[0]) - 1, self.batch_size
        cur = torch.cuda.current_stream(dev)
        s = C.c_void_p(cur.cuda_stream)
        fc = flow_chunk_pairs(bs)  # pairs per flow-UNet call: whole interpolation batches
        chunks = [(f0, min(f0 + fc, P)) for f0 in range(0, P, fc)]
        bits_dev = torch.empty((fc + bs - 1) // bs, dtype=torch.int32, device=dev)
        bits_host = torch.empty(bits_dev.shape, dtype=torch.int32, pin_memory=True)
        factors, outs = [], []
        flow = self.eng.flow(x[0:chunks[0][1]], x[1:chunks[0][1] + 1])
        for ci, (f0, f1) in enumerate(chunks):
            nb = (f1 - f0 + bs - 1) // bs
            self.eng.max_speed2_segments(flow, bs, bits_dev)
            bits_host[:nb].copy_(bits_dev[:nb], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(cur)
            nxt = None
            if ci + 1 < len(chunks):  # the next chunk's flow UNet is queued before the host waits for this chunk's factors
                g0, g1 = chunks[ci + 1]
                nxt = self.eng.flow_net.forward(torch.cat((x[g0:g1], x[g0 + 1:g1 + 1]), dim=1).contiguous(), defer_check=True)
            ready.synchronize()
            self.host_syncs += 1
            us = [auto_upsampling_factor(b, self.U) for b in bits_host[:nb].tolist()]
            factors += us
            outs.append(self._interpolate_chunk(x[f0:f1], x[f0 + 1:f1 + 1], flow, us, h, w, s))
            if nxt is not None:
                self.eng.flow_net.redo_if_flagged()
                flow = nxt
        return (outs[0] if len(outs) == 1 else torch.cat(outs)), factors

    def _interpolate_chunk(self, I0, I1, flow, us, h, w, s):
        """uint8 [sum U_b * pairs_b, H, W] of one flow chunk whose batches have the factors `us`."""
        dev = self.eng.device
        npairs = int(I0.shape[0])
        ts, tab, cuts = auto_sample_table(us, npairs, self.batch_size)
        n = len(tab)
        coef = torch.from_numpy(time_coefficients(ts)).pin_memory().to(dev, non_blocking=True)
        tab_dev = torch.tensor(tab, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        cap = self.samples_per_call
        calls = [(a, min(a + cap, n)) for a in range(0, n, cap)] if cap > 0 else list(zip(cuts[:-1], cuts[1:]))
        q = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        I0, I1 = I0.contiguous(), I1.contiguous()
        for a, b in calls:
            out = self.eng.interpolate_table(I0, I1, flow, coef, tab_dev, a, b - a)
            check(self.lib.v2e_f32_to_u8_trunc_tab(_ptr(out), _ptr(q), _ptr(tab_dev[a:b]), b - a, h * w, self.mean, s),
                  "v2e_f32_to_u8_trunc_tab")
        return self._rs_out(q)

    def upsample_sharded(self, frames_u8, group=None, owner=None):
        """SuperSloMo of ONE clip over the ranks of `group` (BASELINE north_star: "frame batches shard across the
        GPUs"): the P = N - 1 source pairs are independent (slomo.py:330-466: every batch is computed from its own frames), so rank r
        interpolates pairs [r P / G, (r + 1) P / G) -- it needs source frames r P / G .. (r + 1) P / G only -- and the uint8 output
        frames are gathered IN ORDER: to rank `owner` point to point with exact sizes (90 KB per frame at 346x260, 27 MB for a second
        of video at 10x), or, owner = None, to every rank by one all-gather of padded blocks (gather_frames_in_order).
        Returns uint8 [(N - 1) U, H, W] on the assembling rank(s), None elsewhere.  Every rank must hold the same frames_u8 (or at
        least its own slice of it: only frames lo .. hi are read)."""
        import torch.distributed as dist
        if self.auto_upsample:
            raise NotImplementedError("auto_upsample: upsample_sharded needs the ranks' frame counts, which no longer follow from "
                                      "(pairs, world size) alone")
        if group is None and not dist.is_initialized():
            return self.upsample(frames_u8)
        G, r = dist.get_world_size(group), dist.get_rank(group)
        N = int(frames_u8.shape[0])
        lo, hi = pair_shard(N - 1, G, r)
        mine = self.upsample(frames_u8[lo:hi + 1]) if hi > lo else frames_u8.new_empty((0,) + tuple(frames_u8.shape[1:]))
        return gather_frames_in_order(mine, N - 1, self.U, group, owner)

    def _render_hw(self, H, W):
        """Size of the DVS video frames: the emulator's output size where it has one (v2e.py's output_height / output_width)."""
        return int(getattr(self.emu, "output_height", None) or H), int(getattr(self.emu, "output_width", None) or W)

    def _render_clip(self, renderer, ev, counts, hw, as_u8):
        """The DVS video of a whole clip from its device rows: render_run + flush_run; leaves dvs_frames / dvs_frame_times."""
        parts = [renderer.render_run(ev, counts, hw[0], hw[1], frame0=0, batch_size=self.batch_size, as_u8=as_u8),
                 renderer.flush_run(hw[0], hw[1], as_u8=as_u8)]
        parts = [p for p in parts if p[0] is not None]
        self.dvs_frames = torch.cat([p[0] for p in parts]) if parts else None
        self.dvs_frame_times = torch.cat([p[1] for p in parts]) if parts else None

    def run(self, frames_u8, src_frame_interval_s, return_device=False, group=None, owner=0, chunk_pairs=None, renderer=None,
            dvs_u8=False):
        """Full pipeline; returns (events, counts_per_interpolated_frame, n_interpolated_frames).
        renderer: a v2e_amd.EventRenderer -- the clip's DVS video (v2e.py:829-850: a packet per `batch_size` emulator frames,
        the leftover events at the end) is rendered from the device rows in one pass (EventRenderer.render_run / flush_run) and
        left in `dvs_frames` (device float64 [m,h,w] in 0..1, or uint8 with dvs_u8; None if no frame was completed) and
        `dvs_frame_times` (device float64 [m]; `renderer.frame_times_text` formats the reference's listing); events and counts
        are what they are without it.  Not with group=.
        group: a torch.distributed process group -- the SuperSloMo stage is sharded over its ranks by source pairs
        (`upsample_sharded`), the frames are funnelled in order to rank `owner` (rank within the group), which holds the emulator
        state and runs the DVS model; the other ranks return (None, None, n).
        chunk_pairs (with a group): the clip goes through in CHUNKS of that many source pairs -- every chunk sharded over the ranks
        and sent to the owner (point to point, exact sizes), the owner's DVS stage taking chunk c (enqueued, not waited for) while
        the ranks, the owner included, interpolate chunk c + 1: for a long clip the owner no longer idles through the whole
        interpolation and holds one chunk of frames, not the clip.  Same frames, order, times and events as one rank."""
        if renderer is not None and group is not None:
            raise NotImplementedError("renderer= with group=: multi-rank rendering is not implemented")
        if self.auto_upsample:
            if group is not None or chunk_pairs:
                raise NotImplementedError("auto_upsample with group= / chunk_pairs=: the ranks' frame counts would no longer follow "
                                          "from (pairs, world size) alone, so the ranks would have to exchange block sizes")
            up = self.upsample(frames_u8)
            times = interp_frame_times(int(frames_u8.shape[0]), None, float(src_frame_interval_s), self.batch_size,
                                       factors=self.upsampling_factors)
            return self._emulate(up, times, return_device, renderer, dvs_u8) + (int(up.shape[0]),)
        if group is not None and chunk_pairs:
            return self._run_chunked(frames_u8, src_frame_interval_s, return_device, group, owner, int(chunk_pairs))
        if group is not None:
            import torch.distributed as dist
            up = self.upsample_sharded(frames_u8, group, owner)
            n = (int(frames_u8.shape[0]) - 1) * self.U
            if dist.get_rank(group) != owner:
                return None, None, n
        else:
            up = self.upsample(frames_u8)
            n = up.shape[0]
        times = interp_frame_times(int(frames_u8.shape[0]), self.U, float(src_frame_interval_s), self.batch_size)
        return self._emulate(up, times, return_device, renderer, dvs_u8) + (n,)

    def _emulate(self, up, times, return_device, renderer, dvs_u8):
        """(events, counts) of the clip's interpolated frames; with a renderer the rows stay on the device until the DVS video
        is enqueued, and go to the host (if asked for there) as generate_events_batch would have sent them."""
        if renderer is None:
            return self.emu.generate_events_batch(up, times, return_device=return_device)
        ev, counts = self.emu.generate_events_batch(up, times, return_device=True)
        self._render_clip(renderer, ev, counts, self._render_hw(int(up.shape[1]), int(up.shape[2])), dvs_u8)
        if not return_device:
            ev = ev.cpu().numpy() if ev is not None and ev.shape[0] else None
        return ev, counts

    def run_stream(self, frames_u8, src_frame_interval_s, chunk_pairs=None, on_events=None, return_device=False, cap=None,
                   renderer=None, on_dvs_frames=None, dvs_u8=False):
        """The clip through the whole pipeline in chunks of `chunk_pairs` source pairs on one GPU, with device memory bounded by the
        chunk, not the clip; returns (events, counts_per_interpolated_frame, n_interpolated_frames) as `run` does, with the same
        events, counts, frame order, frame times, event files and (auto_upsample) `upsampling_factors`, `interpTimes` and
        `avg_upsampling_factor` as `run` on the same clip with the same fresh emulator.

        frames_u8: uint8 [N,H,W] on the device, or on the host (torch CPU tensor or numpy array: uploaded chunk by chunk through
        two pinned staging buffers on a copy stream).  chunk_pairs: a positive multiple of the flow chunk
        `flow_chunk_pairs(batch_size)` (default four of them; anything else raises ValueError) -- see `stream_chunks`.
        cap: the event-row capacity of every emulator run (None: the emulator's own sizing, `default_event_capacity`, for the
        largest chunk so far).

        The SloMo stage of chunk c + 1 (resize, normalisation, flow and interpolation UNets, truncation, resize back) runs on a side
        stream while the emulator's run of chunk c executes; the emulator is called from the caller's current stream and waits for
        each chunk's frames with an event.  auto_upsample: the time of every frame depends on the factor of the clip's last batch
        (v2e.py:786-797), so the flow UNet runs on the clip's last flow chunk before the first emulator run; `host_syncs` counts
        every factor read-back, that one included.

        on_events(events, counts, frame0): called once per chunk, in frame order, with the chunk's rows (None for a chunk without
        events on the host), its per-frame counts and the index of its first interpolated frame; nothing is accumulated and the
        call returns (None, counts of the whole clip, n).  With return_device=True the rows are a view of one of the emulator's
        two alternating event buffers: valid for the duration of the callback only (work the callback enqueues on the current
        stream is ordered before the buffer is reused).  Without on_events the rows are gathered (device rows copied out of the
        emulator's buffers) and returned as `run` returns them.

        renderer: a v2e_amd.EventRenderer -- every chunk's DVS frames (EventRenderer.render_run with the chunk's first frame
        index, so the packets are the clip's, whatever the chunking) are rendered behind that chunk's result() on a stream of
        their own, which the emulator's runs do not wait for until they reuse the chunk's row buffer; the leftover events are
        flushed at the end.  on_dvs_frames(frames, frame_times, first_frame_index): called in order for every chunk (and the
        flush) that completed frames, device tensors as `render_run` returns them (uint8 frames with dvs_u8), with the render
        stream current; without it the frames are gathered on the device and left in `dvs_frames` / `dvs_frame_times` as
        `run` leaves them.  The renderer's read-backs (one per chunk in DURATION and AREA_COUNT mode) are added to
        `host_syncs`.  Events, counts and event files are what they are without a renderer.

        An emulator built with record_single_pixel_states records its pixel across the chunks as it does across `run`'s one run (the
        sample index runs on over the chunk boundaries; `emu.cleanup()` writes the file): every chunk is then a probed run, on the
        per-frame kernels and not pipelined (EventEmulator.generate_events_batch_async)."""
        N, H, W = stream_source_shape(frames_u8)
        P, bs = N - 1, self.batch_size
        chunks = stream_chunks(P, bs, chunk_pairs)
        dt = float(src_frame_interval_s)
        dev = self.eng.device
        main = torch.cuda.current_stream(dev)
        side = self.__dict__.get("_stream_side")
        if side is None:  # created once: the UNets' workspaces and the resamplers' tables are used on it chunk after chunk
            side = self._stream_side = torch.cuda.Stream(dev, priority=-1)
        side.wait_stream(main)  # the source frames and whatever used the engine before
        for net in (self.eng.flow_net, self.eng.interp_net):
            if getattr(net, "_ws", None) is not None:  # (a workspace allocated on another stream, replaced on this one)
                net._ws.record_stream(side)
        feed = _HostFrameFeed(frames_u8, chunks, dev, side) if not (torch.is_tensor(frames_u8) and frames_u8.is_cuda) else None
        self.host_syncs = 0
        scale = None
        if not self.auto_upsample:
            scale = stream_time_scale(N, dt, bs, self.U)
        elif len(chunks) > 1:
            f0, f1 = last_flow_chunk(P, bs)
            with torch.cuda.stream(side):
                src = frames_u8[f0:f1 + 1] if feed is None else feed.upload_range(f0, f1 + 1)
                scale = stream_time_scale(N, dt, bs, self._last_flow_chunk_factors(src)[-1])
        factors, counts, evs, runs = [], [], [], []
        run_cap = nfr = 0
        d2h = None if return_device else self.__dict__.get("_stream_d2h")
        if not return_device and d2h is None:
            d2h = self._stream_d2h = torch.cuda.Stream(dev)

        rend = self.__dict__.get("_stream_render") if renderer is not None else None
        if renderer is not None and rend is None:
            rend = self._stream_render = torch.cuda.Stream(dev)
        hw = self._render_hw(H, W)
        dvs, dvs_t, syncs0 = [], [], (renderer.host_syncs if renderer is not None else 0)
        self.dvs_frames = self.dvs_frame_times = None

        def deliver(fr, t):
            if fr is None:
                return
            if on_dvs_frames is not None:
                on_dvs_frames(fr, t, renderer.numFramesWritten - int(t.shape[0]))
            else:
                dvs.append(fr)
                dvs_t.append(t)

        def render(ev, cnt, frame0):
            # the run's rows are final (result() has waited for them); they are read on the render stream, and the caller's
            # stream -- which carries the runs that will reuse this row buffer -- is ordered behind that read.  This relies on
            # what on_events' contract relies on: the emulator's own (pipelined) streams order every write to a row buffer behind
            # the caller's stream at the time the run is enqueued, so work put into the caller's stream before that enqueue
            # precedes the reuse.  COUNT and SOURCE make no read-back, so this wait is the only order there is.
            with torch.cuda.stream(rend):
                deliver(*renderer.render_run(ev, cnt, hw[0], hw[1], frame0=frame0, batch_size=bs, as_u8=dvs_u8))
                read = torch.cuda.Event()
                read.record(rend)
            main.wait_event(read)

        def collect():
            pend, _, frame0 = runs.pop(0)  # (the chunk's frames go with the entry: the host has waited for the run's rows)
            ev, cnt = pend.result()
            if renderer is not None:
                render(ev, cnt, frame0)
            if not return_device:  # on a stream of its own: the caller's stream holds the next run's chain
                with torch.cuda.stream(d2h):
                    ev = ev.cpu().numpy() if ev is not None and ev.shape[0] else None
            counts.append(np.asarray(cnt))
            if on_events is not None:
                on_events(ev, cnt, frame0)
            else:
                evs.append(ev.clone() if return_device else ev)

        try:
            if feed is not None:
                feed.start(0)
            for ci, (p0, p1) in enumerate(chunks):
                if len(runs) == 2:  # at most two runs in flight: the emulator's two buffer sets
                    collect()
                if feed is not None and ci + 1 < len(chunks):
                    feed.start(ci + 1)
                with torch.cuda.stream(side):
                    src = frames_u8[p0:p1 + 1] if feed is None else feed.frames(ci)
                    x, h, w = self._normalised_input(src)
                    if feed is not None:
                        feed.consumed(ci)
                    if self.auto_upsample:
                        up, us = self._upsample_auto_x(x, h, w)
                        factors += us
                    else:
                        up, us = self._upsample_fixed(x, h, w, (H, W)), [self.U] * len(range(p0, p1, bs))
                    del x
                    ready = torch.cuda.Event()
                    ready.record(side)
                if scale is None:  # auto_upsample, one chunk: its factors are the clip's
                    scale = stream_time_scale(N, dt, bs, us[-1])
                times = chunk_frame_times(p0, p1, bs, us, scale)
                if cap is None:  # the emulator's own sizing, for the largest chunk so far: its first run has one frame fewer (the
                    #              first frame is the initial state) and a set sized for that would be regrown by the third run
                    run_cap = max(run_cap, default_event_capacity(int(up.shape[0]), H, W))
                main.wait_event(ready)
                # (pipelined runs overlap run after run on streams of the emulator's, which it assigns by a probe on its first such
                #  run; a clip of one chunk has nothing to overlap and runs as run()'s does, plain launches on the caller's stream)
                pend = self.emu.generate_events_batch_async(up, times, return_device=True, use_graph=0,
                                                            cap=run_cap if cap is None else cap, pipelined=len(chunks) > 1)
                runs.append((pend, up, nfr))  # (`up` is read by the emulator's own streams: kept until the run's result)
                nfr += int(up.shape[0])
                del up
            while runs:
                collect()
            if renderer is not None:
                with torch.cuda.stream(rend):
                    deliver(*renderer.flush_run(hw[0], hw[1], as_u8=dvs_u8))
                    if dvs:
                        self.dvs_frames, self.dvs_frame_times = torch.cat(dvs), torch.cat(dvs_t)
                        self.dvs_frames.record_stream(main)
                        self.dvs_frame_times.record_stream(main)
                self.host_syncs += renderer.host_syncs - syncs0
        finally:
            main.wait_stream(side)
            if rend is not None:
                main.wait_stream(rend)
        if self.auto_upsample:
            self.upsampling_factors = factors
            self.interpTimes = interp_times(N, None, bs, factors)
            self.avg_upsampling_factor = sum(factors) / len(factors)
        counts = np.concatenate(counts)
        if on_events is not None:
            return None, counts, nfr
        if return_device:
            return torch.cat(evs), counts, nfr
        evs = [e for e in evs if e is not None]
        return (np.concatenate(evs) if evs else None), counts, nfr

    def _last_flow_chunk_factors(self, frames_u8):
        """auto_upsample: the factors of the batches of the clip's last flow chunk, from its source frames (f0 .. P): the flow UNet
        call and the reduction `_upsample_auto_x` makes for that chunk, read back once."""
        dev = self.eng.device
        bs = self.batch_size
        x = self._normalised_input(frames_u8)[0]
        n = int(x.shape[0]) - 1
        flow = self.eng.flow(x[0:n], x[1:n + 1])
        nb = (n + bs - 1) // bs
        bits_dev = torch.empty(nb, dtype=torch.int32, device=dev)
        self.eng.max_speed2_segments(flow, bs, bits_dev)
        bits = bits_dev.cpu().tolist()
        self.host_syncs += 1
        return [auto_upsampling_factor(b, self.U) for b in bits]

    def _run_chunked(self, frames_u8, src_frame_interval_s, return_device, group, owner, chunk_pairs):
        import torch.distributed as dist
        G, r = dist.get_world_size(group), dist.get_rank(group)
        N = int(frames_u8.shape[0])
        P, U = N - 1, self.U
        times = interp_frame_times(N, U, float(src_frame_interval_s), self.batch_size)
        shape = tuple(frames_u8.shape[1:])
        evs, counts, pending = [], [], None   # pending: (receive requests, the chunk's frames, its times) -- the chunk the owner takes next
        asynchronous = hasattr(self.emu, "generate_events_batch_async")
        runs = []

        def dvs(chunk, t):
            if asynchronous:  # enqueue; the result is read at the end (the emulator alternates two buffer sets: at most two in flight)
                runs.append(self.emu.generate_events_batch_async(chunk, t, return_device=return_device))
                while len(runs) > 1:
                    e, c = runs.pop(0).result()
                    # (device rows are a view of one of the emulator's two alternating buffers: the chunk after next overwrites it)
                    evs.append(e.clone() if return_device and e is not None else e)
                    counts.append(c)
            else:
                e, c = self.emu.generate_events_batch(chunk, t, return_device=return_device)
                evs.append(e)
                counts.append(c)

        for p0 in range(0, P, chunk_pairs):
            p1 = min(p0 + chunk_pairs, P)
            lo, hi = pair_shard(p1 - p0, G, r)
            # (the owner posts its receives BEFORE its own share of the interpolation: the other ranks' sends then complete as they finish)
            reqs, chunk = send_frames_to_owner_begin(p1 - p0, U, shape, frames_u8, group, owner)
            mine = self.upsample(frames_u8[p0 + lo:p0 + hi + 1]) if hi > lo else frames_u8.new_empty((0,) + shape)
            if r == owner and pending is not None:  # the DVS stage of the chunk BEFORE, while this chunk's frames arrive
                for q in pending[0]:
                    q.wait()
                dvs(pending[1], pending[2])
            reqs = send_frames_to_owner_finish(reqs, chunk, mine, p1 - p0, U, group, owner)
            if r == owner:
                pending = (reqs, chunk, times[p0 * U:p1 * U])
            else:
                for q in reqs:
                    q.wait()
        n = P * U
        if r != owner:
            return None, None, n
        for q in pending[0]:
            q.wait()
        dvs(pending[1], pending[2])
        for run in runs:
            e, c = run.result()
            evs.append(e)
            counts.append(c)
        import numpy as np
        evs = [e for e in evs if e is not None and len(e)]
        if not evs:
            ev = None
        elif torch.is_tensor(evs[0]):
            ev = torch.cat(evs)
        else:
            ev = np.concatenate(evs)
        return ev, np.concatenate([np.asarray(c) for c in counts]), n


class _HostFrameFeed:
    """Source frames on the host for `VideoToEvents.run_stream`: chunk c's frames p0 .. p1 go to the device through one of two
    pinned staging buffers on a copy stream while the chunk before is processed; the device buffer of a chunk is overwritten only
    after the side stream has consumed it."""

    def __init__(self, frames, chunks, device, side):
        self.src = frames.numpy() if torch.is_tensor(frames) else frames
        self.chunks, self.side = chunks, side
        n = max(p1 - p0 + 1 for p0, p1 in chunks)
        shape = (n,) + tuple(self.src.shape[1:])
        self.copy = torch.cuda.Stream(device)
        self.pinned = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        with torch.cuda.stream(side):  # (owned by the stream that reads them: freed behind its last use)
            self.dev = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(2)]
        self.copied, self.used = [None, None], [None, None]

    def start(self, ci):
        """Enqueue the upload of chunk ci's frames."""
        p0, p1 = self.chunks[ci]
        k, n = ci % 2, p1 - p0 + 1
        if self.copied[k] is not None:
            self.copied[k].synchronize()  # the pinned buffer's last upload has left it
        np.copyto(self.pinned[k][:n].numpy(), self.src[p0:p1 + 1])
        if self.used[k] is not None:
            self.copy.wait_event(self.used[k])
        with torch.cuda.stream(self.copy):
            self.dev[k][:n].copy_(self.pinned[k][:n], non_blocking=True)
        self.copied[k] = torch.cuda.Event()
        self.copied[k].record(self.copy)

    def frames(self, ci):
        """Chunk ci's frames on the device, the current (side) stream ordered behind their upload."""
        p0, p1 = self.chunks[ci]
        k = ci % 2
        torch.cuda.current_stream(self.dev[k].device).wait_event(self.copied[k])
        return self.dev[k][:p1 - p0 + 1]

    def consumed(self, ci):
        """The current stream has enqueued the last read of chunk ci's device frames."""
        k = ci % 2
        self.used[k] = torch.cuda.Event()
        self.used[k].record(torch.cuda.current_stream(self.dev[k].device))

    def upload_range(self, a, b):
        """Frames a .. b - 1 on the device (one-off, on the current stream)."""
        return torch.from_numpy(np.ascontiguousarray(self.src[a:b])).to(self.dev[0].device)


def pair_shard(n_pairs, world, rank):
    """Source pairs [lo, hi) of rank `rank`: contiguous blocks r P / G .. (r + 1) P / G; empty when P < G leaves none."""
    return rank * n_pairs // world, (rank + 1) * n_pairs // world


def gather_frames_in_order(mine, n_pairs, U, group=None, owner=None):
    """The ranks' interpolated-frame blocks (uint8 [pairs_r U, H, W], pairs_r from pair_shard) in the clip's frame order.
    owner = a rank of the group: POINT TO POINT to that rank, exact sizes, received straight into the clip's tensor (round 6; an
    all-gather hands every rank the whole clip -- G - 1 times the receive volume anybody needs -- and wants the blocks padded to the
    largest); the other ranks return None.  owner = None: every rank assembles the clip (one all-gather of padded blocks).  Block
    sizes follow from (n_pairs, world) alone, so no size exchange is needed."""
    import torch.distributed as dist
    G, r = dist.get_world_size(group), dist.get_rank(group)
    cnt = [(pair_shard(n_pairs, G, q)[1] - pair_shard(n_pairs, G, q)[0]) * U for q in range(G)]
    assert int(mine.shape[0]) == cnt[r], "this rank interpolated %d frames, its shard has %d" % (int(mine.shape[0]), cnt[r])
    if owner is not None:
        reqs, clip = send_frames_to_owner_begin(n_pairs, U, tuple(mine.shape[1:]), mine, group, owner)
        for q in send_frames_to_owner_finish(reqs, clip, mine, n_pairs, U, group, owner):
            q.wait()
        return clip if r == owner else None
    m = max(cnt)
    pad = mine if cnt[r] == m else torch.cat((mine, mine.new_zeros((m - cnt[r],) + tuple(mine.shape[1:]))))
    parts = [torch.empty_like(pad) for _ in range(G)]
    dist.all_gather(parts, pad.contiguous(), group=group)
    return torch.cat([parts[q][:cnt[q]] for q in range(G)])


def _global_rank(group, q):
    import torch.distributed as dist
    return q if group is None or group is dist.group.WORLD else dist.get_global_rank(group, q)


def send_frames_to_owner_begin(n_pairs, U, frame_shape, like, group, owner):
    """Owner: the tensor of the n_pairs * U frames and one posted receive per other rank's block, straight into its slice (posted
    before the owner's own interpolation, so that a sender never waits for the receiver).  Other ranks: ([], None)."""
    import torch.distributed as dist
    G, r = dist.get_world_size(group), dist.get_rank(group)
    if r != owner:
        return [], None
    clip = like.new_empty((n_pairs * U,) + tuple(frame_shape))
    reqs = []
    for q in range(G):
        lo, hi = pair_shard(n_pairs, G, q)
        if q != owner and hi > lo:
            reqs.append(dist.irecv(clip[lo * U:hi * U], src=_global_rank(group, q), group=group))
    return reqs, clip


def send_frames_to_owner_finish(reqs, clip, mine, n_pairs, U, group, owner):
    """Owner: its own block copied into place, the receive requests handed back.  Other ranks: their block sent (a request to wait for)."""
    import torch.distributed as dist
    G, r = dist.get_world_size(group), dist.get_rank(group)
    lo, hi = pair_shard(n_pairs, G, r)
    if r == owner:
        if hi > lo:
            clip[lo * U:hi * U] = mine
        return reqs
    return [dist.isend(mine.contiguous(), dst=_global_rank(group, owner), group=group)] if hi > lo else []
