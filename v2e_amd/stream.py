"""The streaming run of `pipeline.VideoToEvents.run_stream`: a clip through SuperSloMo and the emulator chunk by chunk, with
device memory bounded by the chunk.

`StreamRun` is one call's state (the streams, the emulator runs in flight, what has been gathered) and its steps; `_HostFrameFeed`
uploads source frames that live on the host, a chunk ahead.  The contract is in `VideoToEvents.run_stream`'s docstring.  What
chunked runs share is here too: `rows_to_host` and `join_chunks`.
"""
import numpy as np
import torch

from .emulator import default_event_capacity
from .planning import chunk_frame_times, last_flow_chunk, stream_chunks, stream_time_scale


def rows_to_host(ev):
    """Device event rows as a numpy array on the host, None for no rows: what generate_events_batch returns without return_device."""
    return ev.cpu().numpy() if ev is not None and ev.shape[0] else None


def join_chunks(rows, counts, keep_empty=False):
    """(event rows, per-frame counts) of a clip from those of its chunks, torch or numpy rows alike.  Chunks without rows (None or
    of length 0) are left out, and a clip without rows gives None; keep_empty: every chunk's rows are concatenated as they are."""
    counts = np.concatenate([np.asarray(c) for c in counts])
    if not keep_empty:
        rows = [e for e in rows if e is not None and len(e)]
    if not rows:
        return None, counts
    return (torch.cat(rows) if torch.is_tensor(rows[0]) else np.concatenate(rows)), counts


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


class StreamRun:
    """One `VideoToEvents.run_stream` call: `run()` takes the clip through and returns what run_stream returns.

    Streams: `main`, the caller's, carries the emulator's runs; `side` the SloMo stage of the next chunk; `d2h` the copies of
    rows to the host; `rend` the DVS frames.  The last three are the pipeline's, created on first need and kept.  `runs` holds
    the at most two emulator runs in flight as (handle, the chunk's frames, index of its first frame)."""

    def __init__(self, pipe, frames_u8, src_frame_interval_s, chunk_pairs, on_events, return_device, cap, renderer, on_dvs_frames,
                 dvs_u8, on_frames=None):
        """Checks the clip and the chunking, then readies the streams, the host frame feed and -- where it is known before the
        first chunk -- the time scale, and resets the pipeline's per-clip results."""
        N, self.H, self.W = stream_source_shape(frames_u8)
        chunks = self.chunks = stream_chunks(N - 1, pipe.batch_size, chunk_pairs)
        self.pipe, self.frames, self.N, self.dt = pipe, frames_u8, N, float(src_frame_interval_s)
        self.on_events, self.return_device, self.cap, self.on_frames = on_events, return_device, cap, on_frames
        self.renderer, self.on_dvs_frames, self.dvs_u8 = renderer, on_dvs_frames, dvs_u8
        self.runs, self.rows, self.counts, self.factors, self.dvs = [], [], [], [], []
        self.run_cap = self.nfr = 0
        dev, bs = pipe.eng.device, pipe.batch_size
        self.main = torch.cuda.current_stream(dev)
        # (created once: the UNets' workspaces and the resamplers' tables are used on it chunk after chunk)
        side = self.side = pipe._stream("side", priority=-1)
        side.wait_stream(self.main)  # the source frames and whatever used the engine before
        for net in (pipe.eng.flow_net, pipe.eng.interp_net):
            if net._ws is not None:  # (a workspace allocated on another stream, replaced on this one)
                net._ws.record_stream(side)
        on_device = torch.is_tensor(frames_u8) and frames_u8.is_cuda
        self.feed = None if on_device else _HostFrameFeed(frames_u8, chunks, dev, side)
        pipe.host_syncs = 0
        self.scale = None  # auto_upsample, one chunk: known with that chunk's factors
        if not pipe.auto_upsample:
            self.scale = stream_time_scale(N, self.dt, bs, pipe.U)
        elif len(chunks) > 1:
            f0, f1 = last_flow_chunk(N - 1, bs)
            with torch.cuda.stream(side):
                src = frames_u8[f0:f1 + 1] if on_device else self.feed.upload_range(f0, f1 + 1)
                self.scale = stream_time_scale(N, self.dt, bs, pipe._last_flow_chunk_factors(src)[-1])
        self.d2h = None if return_device else pipe._stream("d2h")
        self.rend = None if renderer is None else pipe._stream("render")
        self.syncs0 = 0 if renderer is None else renderer.host_syncs
        self.hw = pipe._render_hw(self.H, self.W)
        pipe.dvs_frames = pipe.dvs_frame_times = None

    def run(self):
        try:
            if self.feed is not None:
                self.feed.start(0)
            for ci in range(len(self.chunks)):
                if len(self.runs) == 2:  # at most two runs in flight: the emulator's two buffer sets
                    self.collect()
                self.enqueue(ci)
            while self.runs:
                self.collect()
            if self.renderer is not None:
                self.flush_render()
        finally:
            self.main.wait_stream(self.side)
            if self.rend is not None:
                self.main.wait_stream(self.rend)
        if self.pipe.auto_upsample:
            self.pipe._set_auto_result(self.N, self.factors)
        rows, counts = join_chunks(self.rows, self.counts, keep_empty=self.return_device)
        return (None if self.on_events is not None else rows), counts, self.nfr

    def enqueue(self, ci):
        """Chunk ci: its SloMo stage on the side stream, its emulator run on the caller's behind it."""
        pipe, chunks, feed, side = self.pipe, self.chunks, self.feed, self.side
        p0, p1 = chunks[ci]
        bs = pipe.batch_size
        if feed is not None and ci + 1 < len(chunks):
            feed.start(ci + 1)
        with torch.cuda.stream(side):
            src = self.frames[p0:p1 + 1] if feed is None else feed.frames(ci)
            x, h, w = pipe._normalised_input(src)
            if feed is not None:
                feed.consumed(ci)
            if pipe.auto_upsample:
                up, us = pipe._upsample_auto_x(x, h, w)
                self.factors += us
            else:
                up, us = pipe._upsample_fixed(x, h, w, (self.H, self.W)), [pipe.U] * len(range(p0, p1, bs))
            del x
            ready = torch.cuda.Event()
            ready.record(side)
        if self.scale is None:  # auto_upsample, one chunk: its factors are the clip's
            self.scale = stream_time_scale(self.N, self.dt, bs, us[-1])
        times = chunk_frame_times(p0, p1, bs, us, self.scale)
        if self.cap is None:  # the emulator's own sizing, for the largest chunk so far: its first run has one frame fewer (the
            #                   first frame is the initial state) and a set sized for that would be regrown by the third run
            self.run_cap = max(self.run_cap, default_event_capacity(int(up.shape[0]), self.H, self.W))
        self.main.wait_event(ready)
        if self.on_frames is not None:
            # The chunk's frames before its run is enqueued: what the callback enqueues on the caller's stream reads them ahead of
            # the run's chain.  `up` belongs to the side stream's allocator and must not return to it before that work has read
            # it; it is kept with the run's entry until collect() has the run's result, and the host has then waited for rows
            # that the chain wrote behind the callback's work on the same stream.
            self.on_frames(up, times, self.nfr)
        # (pipelined runs overlap run after run on streams of the emulator's, which it assigns by a probe on its first such
        #  run; a clip of one chunk has nothing to overlap and runs as run()'s does, plain launches on the caller's stream)
        pend = pipe.emu.generate_events_batch_async(up, times, return_device=True, use_graph=0,
                                                    cap=self.run_cap if self.cap is None else self.cap,
                                                    pipelined=len(chunks) > 1)
        self.runs.append((pend, up, self.nfr))  # (`up` is read by the emulator's own streams: kept until the run's result)
        self.nfr += int(up.shape[0])

    def collect(self):
        """The oldest run in flight: its rows rendered, brought to the host, handed to on_events or gathered."""
        pend, _, frame0 = self.runs.pop(0)  # (the chunk's frames go with the entry: the host has waited for the run's rows)
        ev, cnt = pend.result()
        if self.renderer is not None:
            self.render(ev, cnt, frame0)
        if not self.return_device:  # on a stream of its own: the caller's stream holds the next run's chain
            with torch.cuda.stream(self.d2h):
                ev = rows_to_host(ev)
        self.counts.append(cnt)
        if self.on_events is not None:
            self.on_events(ev, cnt, frame0)
        else:
            self.rows.append(ev.clone() if self.return_device else ev)

    def render(self, ev, cnt, frame0):
        """The DVS frames of one run's rows, on the render stream."""
        # the run's rows are final (result() has waited for them); they are read on the render stream, and the caller's
        # stream -- which carries the runs that will reuse this row buffer -- is ordered behind that read.  This relies on
        # what on_events' contract relies on: the emulator's own (pipelined) streams order every write to a row buffer behind
        # the caller's stream at the time the run is enqueued, so work put into the caller's stream before that enqueue
        # precedes the reuse.  COUNT and SOURCE make no read-back, so this wait is the only order there is.
        with torch.cuda.stream(self.rend):
            self.deliver(*self.renderer.render_run(ev, cnt, self.hw[0], self.hw[1], frame0=frame0, batch_size=self.pipe.batch_size,
                                                   as_u8=self.dvs_u8))
            read = torch.cuda.Event()
            read.record(self.rend)
        self.main.wait_event(read)

    def deliver(self, fr, t):
        """Completed DVS frames and their times: to on_dvs_frames, or gathered."""
        if fr is None:
            return
        if self.on_dvs_frames is not None:
            self.on_dvs_frames(fr, t, self.renderer.numFramesWritten - int(t.shape[0]))
        else:
            self.dvs.append((fr, t))

    def flush_render(self):
        """The leftover events' DVS frame; the gathered frames become the pipeline's dvs_frames / dvs_frame_times."""
        with torch.cuda.stream(self.rend):
            self.deliver(*self.renderer.flush_run(self.hw[0], self.hw[1], as_u8=self.dvs_u8))
            if self.dvs:
                self.pipe.dvs_frames, self.pipe.dvs_frame_times = (torch.cat(part) for part in zip(*self.dvs))
                self.pipe.dvs_frames.record_stream(self.main)
                self.pipe.dvs_frame_times.record_stream(self.main)
        self.pipe.host_syncs += self.renderer.host_syncs - self.syncs0


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
