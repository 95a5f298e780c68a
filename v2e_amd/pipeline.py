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
    parts = []
    for b0, u in zip(starts, factors):
        nb = min(bs, npairs - b0)
        parts.append(b0 + np.array(range(u * nb)) * (1 / u))
    return np.concatenate(parts)


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

    def upsample(self, frames_u8):
        """frames_u8: device uint8 [N,H,W] -> device uint8 [(N-1)*U, H, W], the frames the reference's
        interpolate() would have written as PNGs (in order).  auto_upsample: sum over batches of U_b * pairs frames."""
        if self.auto_upsample:
            return self._upsample_auto(frames_u8)
        dev = self.eng.device
        N, H, W = frames_u8.shape
        x, h, w = self._normalised_input(frames_u8)
        s = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        U = self.U
        ts = [(k + 0.5) / U for k in range(U)]
        out = torch.empty(((N - 1) * U, H, W), dtype=torch.uint8, device=dev)
        # the flow UNet sees up to 64 pairs at a time (its small levels fill the GPU only with many samples; a pair's
        # flow does not depend on what else is in the batch), the interpolation UNet U x batch_size samples
        fc = self.batch_size * max(1, 64 // self.batch_size)  # pairs per flow-UNet call: whole interpolation batches
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
        cur = torch.cuda.current_stream(dev)
        s = C.c_void_p(cur.cuda_stream)
        fc = bs * max(1, 64 // bs)  # pairs per flow-UNet call: whole interpolation batches
        chunks = [(f0, min(f0 + fc, P)) for f0 in range(0, P, fc)]
        bits_dev = torch.empty((fc + bs - 1) // bs, dtype=torch.int32, device=dev)
        bits_host = torch.empty(bits_dev.shape, dtype=torch.int32, pin_memory=True)
        factors, outs = [], []
        self.host_syncs = 0
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
        self.upsampling_factors = factors
        self.interpTimes = interp_times(N, None, bs, factors)
        self.avg_upsampling_factor = sum(factors) / len(factors)
        return outs[0] if len(outs) == 1 else torch.cat(outs)

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

    def run(self, frames_u8, src_frame_interval_s, return_device=False, group=None, owner=0, chunk_pairs=None):
        """Full pipeline; returns (events, counts_per_interpolated_frame, n_interpolated_frames).
        group: a torch.distributed process group -- the SuperSloMo stage is sharded over its ranks by source pairs
        (`upsample_sharded`), the frames are funnelled in order to rank `owner` (rank within the group), which holds the emulator
        state and runs the DVS model; the other ranks return (None, None, n).
        chunk_pairs (with a group): the clip goes through in CHUNKS of that many source pairs -- every chunk sharded over the ranks
        and sent to the owner (point to point, exact sizes), the owner's DVS stage taking chunk c (enqueued, not waited for) while
        the ranks, the owner included, interpolate chunk c + 1: for a long clip the owner no longer idles through the whole
        interpolation and holds one chunk of frames, not the clip.  Same frames, order, times and events as one rank."""
        if self.auto_upsample:
            if group is not None or chunk_pairs:
                raise NotImplementedError("auto_upsample with group= / chunk_pairs=: the ranks' frame counts would no longer follow "
                                          "from (pairs, world size) alone, so the ranks would have to exchange block sizes")
            up = self.upsample(frames_u8)
            times = interp_frame_times(int(frames_u8.shape[0]), None, float(src_frame_interval_s), self.batch_size,
                                       factors=self.upsampling_factors)
            ev, counts = self.emu.generate_events_batch(up, times, return_device=return_device)
            return ev, counts, int(up.shape[0])
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
        ev, counts = self.emu.generate_events_batch(up, times, return_device=return_device)
        return ev, counts, n

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
