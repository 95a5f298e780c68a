"""Drop-in `EventRenderer`: DVS frames from events, rendered on the GPU a packet at a time.

Mirrors the surface of v2ecore/renderer.py: `ExposureMode`, the constructor signature (:37-99),
`render_events_to_frames(event_arr, height, width, return_frames) -> frames or None` (:161-366) with the frame the packet
ends in left behind in `currentFrame`, and `accumulate_event_frame` (:368-400).

How a packet is rendered here (v2e_amd/csrc/render.hip): the reference walks the packet window by window; this class
never walks it.  The host only works out the packet's window boundaries -- DURATION: the frame start times, the same
scalar additions the reference makes, until they pass the packet's second-to-last time stamp (the only two values read
back from the device); COUNT: plain index arithmetic; AREA_COUNT: the segment ends found by one single-wave scan kernel
(per-cell counters in LDS, the trigger event re-counted in the next window as renderer.py:253-266 does) -- and ONE
launch then drops every event into the frame(s) its window rule assigns it to (binary search over the boundaries; an
event exactly on a DURATION boundary belongs to both neighbours, as the reference's searchsorted left / right pair gives
it), one more clips and normalises all frames of the packet.  The reference's edge behaviour is part of the contract and
kept: the running frame is reset at every packet (:273), the last event of a packet is never accumulated (:303-306), the
frame a packet ends in is not emitted (except SOURCE).  Pinned by frames of the reference's own class in every mode
(tests/golden/make_golden_renderer.py).  AVI output and the preview window (cv2) are outside the hot path: `dvs_vid` /
`preview` raise NotImplementedError.

Whole runs (`render_run` / `flush_run`): the rows and per-frame counts of a device-resident run (`generate_events_batch`,
`VideoToEvents.run` / `run_stream`) are cut into the packets v2e.py:837-850 would hand the per-packet call (`run_packets`) and
all of them are rendered in one pass: the packets' windows are found on the device (DURATION: one lane makes the reference's
scalar additions packet after packet, the start time carried in a device scalar; AREA_COUNT: one single-wave walk over all
packets; COUNT / SOURCE: index arithmetic on the host), one launch histograms every event into the plane of its global frame,
one clips and normalises, and every frame's time (renderer.py:343-350) is computed on the device; `frame_times_text` formats
them as the reference's `-frame_times.txt`.  Frames and times stay on the device; the only read-back is the frame count
(DURATION, AREA_COUNT), which also brings `currentFrameStartTime` back, so the per-packet call can follow a run (not while
rows are pending).
"""
import ctypes as C
import logging
from enum import Enum

import numpy as np
import torch

from . import _capi
from ._capi import check
from .sinks import EventFrameAccumulator

logger = logging.getLogger(__name__)

MAX_RUN_FRAMES = 1 << 22  # DURATION: frames one run may complete before render_run refuses (a time stamp far from the others)


def run_packets(counts, frame0=0, batch_size=8, pending_rows=0):
    """The packets v2e.py:829-850 hands `render_events_to_frames` for emulator frames frame0 .. frame0 + len(counts) - 1 that
    produced counts[k] events each: a frame's events are appended only when it has events (:837-841), and the packet is flushed
    after a frame that has events and whose index i in the clip satisfies i % batch_size == 0 (:842-846).  pending_rows: rows
    appended before frame0 and not yet flushed; they sit in front of this run's rows.  Returns (packets, pending_frames):
    packets int64 [P,2], the row range [first, end) of every flushed packet in (pending rows + this run's rows) -- the first
    starts at row 0, each starts where the one before ends -- and the number of this run's trailing frames whose rows (from the
    last packet's end on) are still pending: v2e.py renders them after the loop ("process leftover events", :848-850).  Host
    arithmetic only."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if (counts < 0).any() or pending_rows < 0 or int(batch_size) < 1:
        raise ValueError("run_packets: negative count / pending_rows or batch_size < 1")
    end = int(pending_rows) + np.cumsum(counts)
    idx = int(frame0) + np.arange(len(counts))
    cut = np.nonzero((counts > 0) & (idx % int(batch_size) == 0))[0]
    ends = end[cut]
    packets = np.stack((np.concatenate(([0], ends[:-1])), ends), axis=1).astype(np.int64) if len(cut) else np.zeros((0, 2), np.int64)
    pending_frames = len(counts) - (int(cut[-1]) + 1 if len(cut) else 0)
    return packets, pending_frames


def frame_times_text(video_name, frame_times, first_frame=0, header=True):
    """The text of the reference's `<dvs_vid>-frame_times.txt` (renderer.py:157-159, 352-353) for frames first_frame,
    first_frame + 1, ... with the times `frame_times` (device tensor or array, seconds): the two header lines (if header) and
    one '{}\t{:10.6f}\n' line per frame."""
    if torch.is_tensor(frame_times):
        frame_times = frame_times.cpu().numpy()
    t = [] if frame_times is None else np.asarray(frame_times, dtype=np.float64).reshape(-1)
    s = '# frame times for {}\n# frame# time(s)\n'.format(video_name) if header else ''
    return s + ''.join('{}\t{:10.6f}\n'.format(int(first_frame) + k, float(v)) for k, v in enumerate(t))


def write_frame_times(path, video_name, frame_times):
    """Write `frame_times_text` of a whole clip to `path`."""
    with open(path, 'w') as f:
        f.write(frame_times_text(video_name, frame_times))


class ExposureMode(Enum):  # renderer.py:19-23
    DURATION = 1
    COUNT = 2
    AREA_COUNT = 3
    SOURCE = 4


class EventRenderer(object):
    """Class for DVS rendering from events (MI355X implementation of v2ecore.renderer.EventRenderer)."""

    def __init__(self, full_scale_count=3, output_path=None, dvs_vid=None, preview=False,
                 exposure_mode=ExposureMode.DURATION, exposure_value=1 / 300.0, area_dimension=None,
                 frame_times_suffix='-frame_times.txt', avi_frame_rate=30, device="cuda"):
        if dvs_vid is not None or preview:
            raise NotImplementedError("v2e_amd.EventRenderer: AVI output / preview (cv2) are outside the hot path; "
                                      "use return_frames=True")
        self.exposure_mode = exposure_mode
        self.exposure_value = exposure_value
        self.output_path = output_path
        self.width = None
        self.height = None
        self.full_scale_count = full_scale_count
        self.accum_mode = 'duration'
        self.dvs_frame_times_suffix = frame_times_suffix
        self.frame_rate_hz = None
        self.event_count = None
        self.frameIntevalS = None
        self.avi_frame_rate = avi_frame_rate
        self.area_counts = None
        self.area_count = None
        self.area_dimension = area_dimension
        if self.exposure_mode == ExposureMode.DURATION:
            self.frame_rate_hz = 1 / self.exposure_value
            self.frameIntevalS = 1 / self.frame_rate_hz
        elif self.exposure_mode == ExposureMode.COUNT:
            self.event_count = int(self.exposure_value)
        elif self.exposure_mode == ExposureMode.AREA_COUNT:
            self.area_count = int(self.exposure_value)
        elif self.exposure_mode == ExposureMode.SOURCE:
            pass
        else:
            raise ValueError(f'exposure mode {self.exposure_mode} is unknown; must be duration, count, or area-count')
        self.video_output_file_name = None
        self.video_output_file = None
        self.frame_times_output_file = None
        self.emulator = None
        self.preview = False
        self.numFramesWritten = 0
        self.currentFrameStartTime = None
        self.currentFrame = None  # device float64 [h,w] while a frame is being filled, else None
        self.printed_empty_packet_warning = False
        _capi.require_gpu("EventRenderer")
        self.device = torch.device(device)
        self._acc = None
        # whole runs (render_run): rows appended and not yet flushed, the DURATION start time on the device, read-backs made
        self._pend_rows = None
        self._time_state = None
        self.host_syncs = 0

    def cleanup(self):
        pass

    # renderer.py:368-400
    def accumulate_event_frame(self, events_dev, histrange):
        """ON/OFF histograms of `events_dev` (device float32 [n,4]) added to the running frame, clipped to +-full scale."""
        if self._acc is None or (self._acc.height, self._acc.width) != (self.height, self.width):
            self._acc = EventFrameAccumulator(self.height, self.width, self.full_scale_count, device=self.device)
        acc = self._acc
        acc.histrange = [(float(histrange[0][0]), float(histrange[0][1])), (float(histrange[1][0]), float(histrange[1][1]))]
        if self.currentFrame is None:
            acc.currentFrame.zero_()
        acc.accumulate(events_dev)
        self.currentFrame = acc.currentFrame

    def _duration_bounds(self, ts_first, ts_second_last, n):
        """Start times T_0 .. T_m of the frames this packet touches (frame k = [T_k, T_k+1], k < m complete; T_m opens the
        frame the packet ends in), advancing `currentFrameStartTime` as the reference does (renderer.py:209-213, 315-318):
        a frame is complete while events beyond its end remain besides the packet's last one, i.e. while the
        second-to-last time stamp lies past the next frame's start."""
        if self.currentFrameStartTime is None:
            self.currentFrameStartTime = ts_first
        bounds = [self.currentFrameStartTime]
        if n >= 2:
            while ts_second_last > self.currentFrameStartTime + self.frameIntevalS:
                nxt = self.currentFrameStartTime + self.frameIntevalS
                if not nxt > self.currentFrameStartTime:
                    raise ValueError("exposure duration %g s does not advance the frame time %r (float32 time stamps)"
                                     % (self.frameIntevalS, self.currentFrameStartTime))
                self.currentFrameStartTime += self.frameIntevalS
                bounds.append(self.currentFrameStartTime)
        return bounds

    def render_events_to_frames(self, event_arr, height: int, width: int, return_frames=False):
        """Render the frames this packet completes (renderer.py:161-366).  `event_arr`: [n,4] events (ts, x, y, pol) as a
        host array or a device tensor.  Returns the completed frames as a float64 [m,h,w] numpy array in 0..1 (only if
        return_frames), or None; the frame the packet ends in stays in `currentFrame` (device float64 [h,w])."""
        if self._pend_rows is not None:
            raise RuntimeError("rows of render_run are still pending on the device: call flush_run before per-packet calls")
        self._time_state = None  # (a later render_run takes the start time from currentFrameStartTime again)
        self.width = width
        self.height = height
        if event_arr is None or event_arr.shape[0] == 0:
            if not self.printed_empty_packet_warning:
                logger.info('event_arr is None or there are no events, doing nothing, supressing further warnings')
                self.printed_empty_packet_warning = True
            return None
        dev = self.device
        if torch.is_tensor(event_arr):
            ev = event_arr.to(dev, torch.float32).contiguous()
            n = int(ev.shape[0])
            edge = ev[[0, max(n - 2, 0)], 0].cpu().numpy() if self.exposure_mode == ExposureMode.DURATION else None
        else:
            host = np.ascontiguousarray(event_arr, dtype=np.float32)
            n = int(host.shape[0])
            ev = torch.from_numpy(host).to(dev)
            edge = host[[0, max(n - 2, 0)], 0] if self.exposure_mode == ExposureMode.DURATION else None
        lib = _capi.lib()
        stream = _capi.stream_ptr(dev)
        mode = self.exposure_mode
        bounds_dev = seg_dev = None
        n_bounds = n_seg = 0
        count_per_frame = 1
        has_open = 1
        if mode == ExposureMode.DURATION:
            bounds = self._duration_bounds(edge[0], edge[1], n)
            n_complete = len(bounds) - 1
            bounds_dev = torch.tensor([float(b) for b in bounds], dtype=torch.float64).to(dev)
            n_bounds = len(bounds)
        elif mode == ExposureMode.COUNT:
            count_per_frame = int(self.event_count)
            n_complete = (n - 2) // count_per_frame if n >= 2 else 0  # frames [k c, (k + 1) c) with (k + 1) c < n - 1
        elif mode == ExposureMode.AREA_COUNT:
            nw = 1 + self.width // self.area_dimension
            nh = 1 + self.height // self.area_dimension
            if self.area_counts is None or tuple(self.area_counts.shape) != (nw, nh):
                self.area_counts = torch.zeros((nw, nh), dtype=torch.int32, device=dev)
            seg_dev = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
            out2 = torch.zeros((2,), dtype=torch.int32, device=dev)
            check(lib.v2e_render_area_segments(C.c_void_p(ev.data_ptr()), n, C.c_void_p(self.area_counts.data_ptr()), nw, nh,
                                               float(self.area_dimension), int(self.area_count), C.c_void_p(seg_dev.data_ptr()),
                                               int(seg_dev.numel()), C.c_void_p(out2.data_ptr()), stream), "v2e_render_area_segments")
            n_seg = n_complete = int(out2[0].item())
        else:  # SOURCE: the whole packet is one frame, and it is emitted
            n_complete, has_open = 1, 0
        npx = height * width
        diff = torch.empty((n_complete + has_open, npx), dtype=torch.int32, device=dev)
        frames = torch.empty((n_complete, height, width), dtype=torch.float64, device=dev)
        cur = torch.empty((height, width), dtype=torch.float64, device=dev) if has_open else None
        check(lib.v2e_render_packet(C.c_void_p(ev.data_ptr()), n - 1, mode.value,
                                    C.c_void_p(bounds_dev.data_ptr()) if bounds_dev is not None else None, n_bounds,
                                    count_per_frame, C.c_void_p(seg_dev.data_ptr()) if seg_dev is not None else None, n_seg,
                                    n_complete, has_open, C.c_void_p(diff.data_ptr()),
                                    C.c_void_p(frames.data_ptr()) if n_complete else None,
                                    C.c_void_p(cur.data_ptr()) if cur is not None else None, height, width,
                                    0.0, float(self.height), 0.0, float(self.width), float(self.full_scale_count), stream),
              "v2e_render_packet")
        self.currentFrame = cur
        if n_complete == 0 or not return_frames:
            return None
        return frames.cpu().numpy()

    # ------------------------------------------------------------------------------------------------------ whole runs
    def render_run(self, rows, counts, height: int, width: int, frame0=0, batch_size=8, return_frames=True, as_u8=False):
        """Render every DVS frame the packets of a device-resident run complete, in one pass.  rows: device float32 [N,4]
        (ts, x, y, pol), the run's events in order (None or empty for a run without events); counts: events per emulator
        frame, sum N (what `generate_events_batch` returns); frame0: the clip index of the run's first emulator frame, so
        that `run_packets` cuts the same packets however the clip is split into runs.  Rows left pending at the end of the
        run are copied aside on the device and go in front of the next run's; `flush_run` renders them at the end of the clip.

        Returns (frames, frame_times), device tensors: frames float64 [m,h,w] in 0..1, the values the reference returns (or
        uint8 with as_u8, `(img * 255).astype(uint8)`, the bytes it hands its AVI writer, renderer.py:339; None if not
        return_frames), frame_times float64 [m] in seconds (renderer.py:343-350).  (None, None) where no frame was
        completed.  `numFramesWritten` advances by m; the frame the last packet ends in stays in `currentFrame` (device
        float64 [h,w]; None in SOURCE mode), the frames the other packets end in are discarded as the reference discards
        them.  One host read-back (`host_syncs`) in DURATION and AREA_COUNT mode, for the frame count (DURATION: with
        it `currentFrameStartTime`, the host's copy of the start time carried on the device); none otherwise."""
        self.width = width
        self.height = height
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        n_new = int(counts.sum())
        n_rows = 0 if rows is None else int(rows.shape[0])
        if n_rows != n_new:
            raise ValueError("render_run: %d rows for counts that sum to %d" % (n_rows, n_new))
        n_pend = 0 if self._pend_rows is None else int(self._pend_rows.shape[0])
        packets, _ = run_packets(counts, frame0, batch_size, pending_rows=n_pend)
        if n_new == 0:
            return None, None  # nothing appended, nothing flushed
        if not torch.is_tensor(rows) or not rows.is_cuda:
            raise TypeError("render_run takes the run's rows as a device tensor")
        rows = rows.to(torch.float32)
        ev = rows if n_pend == 0 else torch.cat((self._pend_rows, rows))
        used = int(packets[-1, 1]) if len(packets) else 0
        pend = ev[used:].clone() if used < n_pend + n_new else None
        out = (None, None)
        if len(packets):  # (a refused run leaves the pending rows as they were)
            out = self._render_packets(ev.contiguous(), [0] + [int(e) for e in packets[:, 1]], return_frames, as_u8)
        self._pend_rows = pend
        return out

    def flush_run(self, height=None, width=None, return_frames=True, as_u8=False):
        """v2e.py:848-850, "process leftover events": the rows still pending after the clip's last run, rendered as the final
        packet.  Returns what `render_run` returns; (None, None) without pending rows (currentFrame is then left alone)."""
        if height is not None:
            self.height = height
        if width is not None:
            self.width = width
        ev = self._pend_rows
        if ev is None or ev.shape[0] == 0:
            self._pend_rows = None
            return None, None
        out = self._render_packets(ev.contiguous(), [0, int(ev.shape[0])], return_frames, as_u8)
        self._pend_rows = None
        return out

    def _render_packets(self, ev, off, return_frames, as_u8):
        """The packets rows [off[p], off[p + 1]) of `ev` (device float32 [N,4], every packet non-empty) in one pass."""
        if self.height is None or self.width is None:
            raise ValueError("height and width not set for the output frames")
        dev, lib, mode = self.device, _capi.lib(), self.exposure_mode
        stream = _capi.stream_ptr(dev)
        P, n_rows = len(off) - 1, off[-1]
        assert P >= 1 and off[0] == 0 and all(b > a for a, b in zip(off, off[1:])) and n_rows <= int(ev.shape[0])
        height, width = int(self.height), int(self.width)
        p_ev = C.c_void_p(ev.data_ptr())
        has_open, count_per_frame = 1, 1
        bounds = seg = None
        if mode in (ExposureMode.COUNT, ExposureMode.SOURCE):  # frames per packet are index arithmetic: no read-back
            if mode == ExposureMode.COUNT:
                count_per_frame = int(self.event_count)
                per = [(b - a - 2) // count_per_frame if b - a >= 2 else 0 for a, b in zip(off, off[1:])]
            else:
                per, has_open = [1] * P, 0
            f0 = np.concatenate(([0], np.cumsum(per)))
            total = int(f0[-1])
            table = torch.from_numpy(np.concatenate((np.asarray(off, np.int64), f0.astype(np.int64)))).to(dev)
            off_dev, f0_dev = table[:P + 1], table[P + 1:].to(torch.int32)
        else:
            off_dev = torch.tensor(off, dtype=torch.int64).to(dev)
            f0_dev = torch.empty((P + 1,), dtype=torch.int32, device=dev)
            out2 = torch.empty((2,), dtype=torch.int32, device=dev)
        p_off, p_f0 = C.c_void_p(off_dev.data_ptr()), C.c_void_p(f0_dev.data_ptr())
        times = None
        if mode == ExposureMode.DURATION:
            f32 = 1 if type(np.float32(0) + 0.5) is np.float32 else 0  # does `currentFrameStartTime += frameIntevalS` stay float32?
            if self._time_state is None:
                t0 = self.currentFrameStartTime
                self._time_state = torch.tensor([0.0, 0.0, 0.0] if t0 is None else [float(t0), 1.0, 0.0], dtype=torch.float64).to(dev)
            p_state = C.c_void_p(self._time_state.data_ptr())

            def windows(commit, bounds, times):
                check(lib.v2e_render_run_windows(p_ev, p_off, P, float(self.frameIntevalS), f32, p_state, commit, p_f0,
                                                 None if bounds is None else C.c_void_p(bounds.data_ptr()),
                                                 0 if bounds is None else int(bounds.numel()),
                                                 None if times is None else C.c_void_p(times.data_ptr()),
                                                 0 if times is None else int(times.numel()), MAX_RUN_FRAMES,
                                                 C.c_void_p(out2.data_ptr()), stream), "v2e_render_run_windows")

            windows(0, None, None)  # the counting pass: nothing is committed before the frame count is known to be sane
            total, err, t_end = torch.cat((out2.to(torch.float64), self._time_state[2:3])).tolist()  # ONE read-back
            total, err = int(total), int(err)
            self.host_syncs += 1
            if err == 1:
                raise ValueError("exposure duration %g s does not advance the frame time (float32 time stamps)" % self.frameIntevalS)
            if err:
                raise ValueError("exposure duration %g s: one run would complete more than %d frames" % (self.frameIntevalS, MAX_RUN_FRAMES))
            bounds = torch.empty((total + P,), dtype=torch.float64, device=dev)
            times = torch.empty((total,), dtype=torch.float64, device=dev)
            windows(1, bounds, times if total else None)
            self.currentFrameStartTime = np.float32(t_end) if f32 else np.float64(t_end)  # the host's copy of the device scalar
        elif mode == ExposureMode.AREA_COUNT:
            nw = 1 + self.width // self.area_dimension
            nh = 1 + self.height // self.area_dimension
            if self.area_counts is None or tuple(self.area_counts.shape) != (nw, nh):
                self.area_counts = torch.zeros((nw, nh), dtype=torch.int32, device=dev)
            seg = torch.empty((n_rows,), dtype=torch.int32, device=dev)
            check(lib.v2e_render_run_area_segments(p_ev, p_off, P, C.c_void_p(self.area_counts.data_ptr()), nw, nh,
                                                   float(self.area_dimension), int(self.area_count), C.c_void_p(seg.data_ptr()),
                                                   int(seg.numel()), p_f0, C.c_void_p(out2.data_ptr()), stream),
                  "v2e_render_run_area_segments")
            total = int(out2[0].item())
            self.host_syncs += 1
            if total > n_rows:
                raise _capi.V2EAmdError("AREA_COUNT: more windows than events")
        if mode != ExposureMode.DURATION and total:
            times = torch.empty((total,), dtype=torch.float64, device=dev)
            check(lib.v2e_render_run_frame_times(p_ev, p_off, P, mode.value, count_per_frame,
                                                 None if seg is None else C.c_void_p(seg.data_ptr()), p_f0, total,
                                                 C.c_void_p(times.data_ptr()), stream), "v2e_render_run_frame_times")
        want = 1 if return_frames and total else 0
        npx = height * width
        diff = torch.empty(((total if want else 0) + has_open, npx), dtype=torch.int32, device=dev)
        frames = None
        if want:
            frames = torch.empty((total, height, width), dtype=torch.uint8 if as_u8 else torch.float64, device=dev)
        cur = torch.empty((height, width), dtype=torch.float64, device=dev) if has_open else None
        if diff.numel():
            p_fr = None if frames is None else C.c_void_p(frames.data_ptr())
            check(lib.v2e_render_run(p_ev, n_rows, p_off, P, mode.value, None if bounds is None else C.c_void_p(bounds.data_ptr()),
                                     count_per_frame, None if seg is None else C.c_void_p(seg.data_ptr()), p_f0, total, has_open,
                                     want, C.c_void_p(diff.data_ptr()), None if as_u8 else p_fr, p_fr if as_u8 else None,
                                     None if cur is None else C.c_void_p(cur.data_ptr()), height, width,
                                     0.0, float(height), 0.0, float(width), float(self.full_scale_count), stream), "v2e_render_run")
        self.currentFrame = cur
        self.numFramesWritten += total
        if total == 0:
            return None, None
        return frames, times
