"""Device-resident video -> events pipeline (BASELINE configs[2]).

The reference's v2e.py runs its three stages through the filesystem: source frames as .npy,
`SuperSloMo.interpolate` writes 8-bit PNGs (slomo.py:436-444), v2e.py reads them back
(v2e.py:832) and calls `EventEmulator.generate_events` per frame.  `VideoToEvents` keeps every
frame in HBM and produces the same uint8 frames for the emulator:

  source uint8 [N,H,W] --Pillow-exact LANCZOS--> [N,h,w] --/255 - mean--> SloMo (HIP, all U time
  points per batch) --(+mean)*255, byte truncation--> uint8 --Pillow-exact BILINEAR--> [P*U,H,W]
  --> emulator (HIP, Philox, one device-resident run)

Here: `DeviceResampler` and `VideoToEvents` (`upsample`, `run`, the render helpers).  The frame order, factor and chunk arithmetic
is `planning`'s, the chunk-by-chunk run on one GPU (`run_stream`) is `stream`'s, and one clip over several GPUs
(`run(..., group=)`, `upsample_sharded`) is `shard`'s; their names are re-exported here.
"""
import os

import torch
import torch.distributed as dist

from . import _capi
from ._capi import check, ptr, stream_ptr
from .planning import (auto_sample_table, auto_upsampling_factor, chunk_frame_times, flow_chunk_pairs,  # noqa: F401  (re-exported)
                       flow_chunks, interp_frame_times, interp_times, last_flow_chunk, speed_from_bits, stream_chunks,
                       stream_time_scale, time_coefficients, time_points)
from .resample import coeffs_8bpc
from .shard import (gather_frames_in_order, pair_shard, run_chunked, send_frames_to_owner_begin,  # noqa: F401  (re-exported)
                    send_frames_to_owner_finish)
from .stream import StreamRun, rows_to_host, stream_source_shape  # noqa: F401  (re-exported)


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
        check(self.lib.v2e_resample_u8(ptr(x), ptr(tmp), ptr(out), n, self.ih, self.iw, self.oh, self.ow, ptr(self.hb),
                                       ptr(self.hk), self.hks, ptr(self.vb), ptr(self.vk), self.vks, stream_ptr(self.device)),
              "v2e_resample_u8")
        return out


# Samples per interpolation-UNet call of the auto_upsample path: consecutive batches (each with its own U_b) are packed into calls
# of at most this many samples.  0: one call per batch (no packing; A/B runs).  DESIGN.md section 5 has the measurement.
AUTO_SAMPLES_PER_CALL = 128


class VideoToEvents:
    """SuperSloMo upsampling + DVS emulation of one clip without leaving HBM."""
    # (class-level defaults: also for subclasses that set their own attributes instead of calling __init__)
    auto_upsample = False
    _streams = None  # run_stream's streams by name, created on first need (`_stream`)

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
        """Fixed U from the normalised input x [N,1,h,w] (`_normalised_input`): uint8 [(N-1)*U, H, W].  The flow UNet sees a flow
        chunk of pairs at a time (`flow_chunk_pairs`), the interpolation UNet U x batch_size samples."""
        dev = self.eng.device
        N = int(x.shape[0])
        H, W = out_hw
        U, bs = self.U, self.batch_size
        ts = time_points(U)
        out = torch.empty(((N - 1) * U, H, W), dtype=torch.uint8, device=dev)
        for f0, f1 in flow_chunks(N - 1, bs):
            flow = self.eng.flow(x[f0:f1], x[f0 + 1:f1 + 1])
            for b0 in range(f0, f1, bs):
                b1 = min(b0 + bs, f1)
                B = b1 - b0
                Ft = self.eng.interpolate(x[b0:b1], x[b0 + 1:b1 + 1], ts, flow=flow[b0 - f0:b1 - f0].contiguous())  # [U,B,1,h,w]
                q = torch.empty((B * U, h, w), dtype=torch.uint8, device=dev)
                check(self.lib.v2e_f32_to_u8_trunc(ptr(Ft), ptr(q), U, B, h * w, self.mean, 1, stream_ptr(dev)), "v2e_f32_to_u8_trunc")
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
        check(self.lib.v2e_u8_to_f32_norm(ptr(small), ptr(x), small.numel(), self.mean, stream_ptr(dev)), "v2e_u8_to_f32_norm")
        return x, h, w

    def _upsample_auto(self, frames_u8):
        """auto_upsample: the flow UNet runs on chunks of up to 64 pairs (whole batches); one launch gives every batch's largest
        squared speed, read back ONCE per chunk -- behind the next chunk's flow UNet, which is enqueued first.  The chunk's samples
        (v2e frame order: batch offset + U_b * pair + k) go through the interpolation UNet in calls of up to `samples_per_call`
        samples that may span batches with different U_b (k_prep_tab / k_fuse_tab), and each sample is truncated straight into its
        frame slot, so the chunk's frames are one contiguous range for the BILINEAR resize."""
        N = int(frames_u8.shape[0])
        if N < 2:
            raise ValueError("auto_upsample needs at least two source frames, got %d" % N)
        x, h, w = self._normalised_input(frames_u8)
        self.host_syncs = 0
        out, factors = self._upsample_auto_x(x, h, w)
        self._set_auto_result(N, factors)
        return out

    def _set_auto_result(self, n_src, factors):
        """auto_upsample: what a run leaves about its factors (one per batch)."""
        self.upsampling_factors = factors
        self.interpTimes = interp_times(n_src, None, self.batch_size, factors)
        self.avg_upsampling_factor = sum(factors) / len(factors)

    def _read_factors(self, flow, x=None, nxt=None):
        """auto_upsample: the factor of every batch of a flow chunk from its flow -- one launch reduces every batch's largest
        squared speed, one copy brings them to the host (counted in host_syncs).  nxt = (f0, f1): the flow UNet on those pairs of
        x is enqueued, its range check left to the caller (`HipUNet.redo_if_flagged`), before the host waits for the copy.
        Returns (factors, that flow or None)."""
        dev, bs = self.eng.device, self.batch_size
        nb = (int(flow.shape[0]) + bs - 1) // bs
        bits_dev = torch.empty(nb, dtype=torch.int32, device=dev)
        bits_host = torch.empty(nb, dtype=torch.int32, pin_memory=True)
        self.eng.max_speed2_segments(flow, bs, bits_dev)
        bits_host.copy_(bits_dev, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        flow_nxt = None
        if nxt is not None:
            f0, f1 = nxt
            flow_nxt = self.eng.flow_net.forward(torch.cat((x[f0:f1], x[f0 + 1:f1 + 1]), dim=1).contiguous(), defer_check=True)
        ready.synchronize()
        self.host_syncs += 1
        return [auto_upsampling_factor(b, self.U) for b in bits_host.tolist()], flow_nxt

    def _upsample_auto_x(self, x, h, w):
        """auto_upsample from the normalised input x [N,1,h,w]: (uint8 frames, the factor of every batch).  Adds its factor
        read-backs to host_syncs."""
        chunks = flow_chunks(int(x.shape[0]) - 1, self.batch_size)
        factors, outs = [], []
        flow = self.eng.flow(x[0:chunks[0][1]], x[1:chunks[0][1] + 1])
        for (f0, f1), nxt in zip(chunks, chunks[1:] + [None]):
            # the next chunk's flow UNet is queued before the host waits for this chunk's factors
            us, flow_nxt = self._read_factors(flow, x, nxt)
            factors += us
            outs.append(self._interpolate_chunk(x[f0:f1], x[f0 + 1:f1 + 1], flow, us, h, w))
            if nxt is not None:
                self.eng.flow_net.redo_if_flagged()
                flow = flow_nxt
        return (outs[0] if len(outs) == 1 else torch.cat(outs)), factors

    def _last_flow_chunk_factors(self, frames_u8):
        """auto_upsample: the factors of the batches of the clip's last flow chunk, from its source frames (f0 .. P): the flow UNet
        call and the reduction `_upsample_auto_x` makes for that chunk, read back once."""
        x = self._normalised_input(frames_u8)[0]
        n = int(x.shape[0]) - 1
        return self._read_factors(self.eng.flow(x[0:n], x[1:n + 1]))[0]

    def _interpolate_chunk(self, I0, I1, flow, us, h, w):
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
            check(self.lib.v2e_f32_to_u8_trunc_tab(ptr(out), ptr(q), ptr(tab_dev[a:b]), b - a, h * w, self.mean, stream_ptr(dev)),
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
        if self.auto_upsample:
            raise NotImplementedError("auto_upsample: upsample_sharded needs the ranks' frame counts, which no longer follow from "
                                      "(pairs, world size) alone")
        if group is None and not dist.is_initialized():
            return self.upsample(frames_u8)
        N = int(frames_u8.shape[0])
        lo, hi = pair_shard(N - 1, dist.get_world_size(group), dist.get_rank(group))
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
            return run_chunked(self, frames_u8, src_frame_interval_s, return_device, group, owner, int(chunk_pairs))
        N = int(frames_u8.shape[0])
        if group is not None:
            up = self.upsample_sharded(frames_u8, group, owner)
            if dist.get_rank(group) != owner:
                return None, None, (N - 1) * self.U
        else:
            up = self.upsample(frames_u8)
        times = interp_frame_times(N, self.U, float(src_frame_interval_s), self.batch_size)
        return self._emulate(up, times, return_device, renderer, dvs_u8) + (int(up.shape[0]),)

    def _emulate(self, up, times, return_device, renderer, dvs_u8):
        """(events, counts) of the clip's interpolated frames; with a renderer the rows stay on the device until the DVS video
        is enqueued, and go to the host (if asked for there) as generate_events_batch would have sent them."""
        if renderer is None:
            return self.emu.generate_events_batch(up, times, return_device=return_device)
        ev, counts = self.emu.generate_events_batch(up, times, return_device=True)
        self._render_clip(renderer, ev, counts, self._render_hw(int(up.shape[1]), int(up.shape[2])), dvs_u8)
        return (ev if return_device else rows_to_host(ev)), counts

    def _stream(self, name, **kw):
        """The pipeline's stream `name` of run_stream ('side', 'd2h', 'render'), created on first need and kept: whatever is
        allocated or cached on one (UNet workspaces, resampler tables) is used on it clip after clip."""
        if self._streams is None:
            self._streams = {}
        if name not in self._streams:
            self._streams[name] = torch.cuda.Stream(self.eng.device, **kw)
        return self._streams[name]

    def run_stream(self, frames_u8, src_frame_interval_s, chunk_pairs=None, on_events=None, return_device=False, cap=None,
                   renderer=None, on_dvs_frames=None, dvs_u8=False, on_frames=None):
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

        on_frames(frames, times, frame0): called once per chunk, in frame order, on the caller's stream (which has been ordered
        behind the chunk's SloMo stage) before the chunk's emulator run is enqueued, with the very uint8 tensor [F,H,W] the emulator
        is about to read, the F frame times and the index of the chunk's first interpolated frame -- ThresholdSweep.add_run takes
        it as it is.  The tensor is valid for the duration of the callback only: work the callback enqueues on the current stream
        reads it before its memory is reused, anything else has to copy it.  Without on_frames nothing changes.

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
        return StreamRun(self, frames_u8, src_frame_interval_s, chunk_pairs, on_events, return_device, cap, renderer, on_dvs_frames,
                         dvs_u8, on_frames).run()
