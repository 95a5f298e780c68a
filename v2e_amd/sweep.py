"""Threshold search on the device: `ThresholdSweep` counts the ON and OFF events of one clip for many thresholds in one pass.

The reference finds the thresholds that make the emulator match a recording by running the whole clip through one emulator per
threshold (dataset_scripts/ddd/ddd_find_thresholds.py: 95 thresholds, counts inside a region of interest, nearest count wins;
v2ecore/thres_estimator.py: all of v2e.py per threshold).  Only the thresholds, base_log_frame and the counts depend on the
threshold -- every Philox draw is keyed by (pixel, frame, stream, clip), lp_log_frame by the frames alone -- so one kernel
(v2e_amd/csrc/sweep.hip) reads each frame once and carries all columns' base_log_frame and counts in registers.

The contract, literally: `ThresholdSweep(...).run(frames, t)` returns, for every column j, the number of ON and OFF events with
x0 <= x <= x1 and y0 <= y <= y1 that

    EventEmulator(pos_thres=pos[j], neg_thres=neg[j], rng_mode="philox", seed=seed, sigma_thres=..., cutoff_hz=...,
                  leak_rate_hz=..., leak_jitter_fraction=..., noise_rate_cov_decades=..., refractory_period_s=...,
                  shot_noise_rate_hz=0)

emits when the F frames are given to it one by one from a fresh instance (the first frame initialises it and emits nothing).
Integers, no tolerance.  The refractory rule (emulator.py:830) couples the pixels of a frame; the kernel runs every column as if
it were off and flags the columns in which it would have switched on, and those are recomputed here with the emulator itself
(`SweepResult.rule_on` says which).  The sums over pixels are 64-bit; the one limit is a single pixel's own ON (or OFF) total of
a column over the whole clip, which the kernel keeps in 32 bits: beyond 2^32 - 1 events of one polarity on one pixel it wraps.

A clip of any length goes through chunk by chunk: `add_run(frames, t, frame0)` sweeps the clip's next frames and `result()` returns
the counts of all frames so far, the same integers `run` gives for them as one clip however the clip is cut.  The kernel
(v2e_thres_sweep_chunk) carries lp_log_frame and every column's base_log_frame from call to call in two sets of device planes that
alternate as its input and output -- it never writes what it reads -- adds to the counts and ORs into the flags, and keys Philox by
the clip's frame index.  With refractory_period_s == 0 no flag can rise and add_run never waits for the device.  Otherwise it reads
the T flags back after each call.  While the rule has never been on in a column, timestamp_mem is neither read nor written
(sweep.hip), so when a column's flag first rises in a chunk its state at the START of that chunk is still exact, and still there.
That column leaves the kernel: what the kernel added to it in this chunk is dropped, and from the chunk's first frame on it is
computed by the emulator itself, primed with the carried lp and base planes, an untouched timestamp_mem, the column's thresholds,
frame_counter = frame0 and the previous frame's time as t_previous, for the rest of the clip (`SweepResult.rule_on_from`).  One
emulator is shared by all such columns, their own state planes copied in and out around each block of frames
(`_advance_columns`).  `reset()` readies the instance for the next clip.  VideoToEvents.run_stream and SyntheticToEvents.run hand
each chunk's frames to `add_run` through their `on_frames` hook.

Out of scope: shot noise (it resets base_log_frame per column and adds rows), hdr, float frames, photoreceptor_noise, SCIDVS,
CSDVS, tape mode, per-frame or per-pixel count maps, reading recordings, multi-rank runs.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from ._capi import check

RECOMPUTE_BLOCK_FRAMES = 32  # frames per emulator run when a rule-on column is recomputed (bounds the event buffer)


class SweepResult(object):
    """on, off: numpy int64 [T]; rule_on: numpy bool [T], True where the column was computed by the emulator because the
    refractory rule switched on; rule_on_from: numpy int64 [T], the clip's index of the first frame the emulator computed in that
    column -- the `frame0` of the chunk in which it left the kernel (0 from `run`) -- and -1 where rule_on is False."""

    def __init__(self, on, off, rule_on, rule_on_from=None):
        self.on, self.off, self.rule_on = on, off, rule_on
        self.rule_on_from = np.where(rule_on, 0, -1).astype(np.int64) if rule_on_from is None else rule_on_from

    def __repr__(self):
        return "SweepResult(on=%r, off=%r, rule_on=%r, rule_on_from=%r)" % (self.on, self.off, self.rule_on, self.rule_on_from)


def check_continuation(frames_seen, t_last, t_frames, frame0=None):
    """The chunk with frame times t_frames continues a clip of which frames_seen frames have been swept, the last one at time
    t_last (ignored while frames_seen is 0): returns the clip's index of the chunk's first frame, which is frames_seen.  ValueError
    for an empty chunk, a frame0 that is given and is not frames_seen (a gap or an overlap), times that are not finite or do not
    increase inside the chunk, a first time that is negative, or one that is not after t_last."""
    t = np.asarray(t_frames, dtype=np.float64).reshape(-1)
    frames_seen = int(frames_seen)
    if len(t) < 1:
        raise ValueError("ThresholdSweep.add_run: a chunk has at least one frame")
    if frame0 is not None and int(frame0) != frames_seen:
        raise ValueError("ThresholdSweep.add_run: the chunk begins at frame %d of the clip but %d frames have been swept (%s)"
                         % (int(frame0), frames_seen, "a gap" if int(frame0) > frames_seen else "an overlap"))
    if not (np.all(np.isfinite(t)) and t[0] >= 0 and np.all(np.diff(t) > 0)):
        raise ValueError("ThresholdSweep.add_run: frame times must be finite, not negative and increasing")
    if frames_seen > 0 and not t[0] > float(t_last):
        raise ValueError("ThresholdSweep.add_run: the chunk's first frame time %r is not after the last frame swept, %r"
                         % (float(t[0]), float(t_last)))
    return frames_seen


class _EmuColumn(object):
    """A column of a streamed sweep that the emulator computes (the refractory rule switched on in it).  acc: device int64 [2], its
    ON / OFF counts so far; base0: its base_log_frame [H*W] at the start of the chunk in which it left the kernel (None: it left
    in the clip's first chunk and starts as a fresh emulator); planes: what the shared emulator's state planes held after this
    column's last block -- base_log_frame, timestamp_mem and the two threshold planes, padded as the engine holds them (None before
    its first block)."""

    def __init__(self, acc, base0):
        self.acc, self.base0, self.planes = acc, base0, None


def _thresholds(values, what):
    a = np.array(values, dtype=np.float64).reshape(-1)
    if len(a) < 1:
        raise ValueError("ThresholdSweep: %s is empty" % what)
    if not (np.all(np.isfinite(a)) and np.all(a > 0)):
        raise ValueError("ThresholdSweep: %s must be positive and finite, got %r" % (what, values))
    return a


class ThresholdSweep(object):
    """ON / OFF event counts of a clip for every (thresholds[j], neg_thresholds[j]) in one pass over the frames (module docstring).

    roi = ((x0, x1), (y0, y1)), inclusive as in v2e_utils.select_events_in_roi; None: the whole sensor.  neg_thresholds=None: the
    same values as thresholds.  cols_per_thread: columns a thread of the kernel carries (0: the library's default; 4, 8, 16).
    max_iters: of the emulators that recompute rule-on columns."""

    def __init__(self, height, width, thresholds, neg_thresholds=None, *, roi=None, sigma_thres=0.03, cutoff_hz=0.0,
                 leak_rate_hz=0.1, refractory_period_s=0.0, leak_jitter_fraction=0.1, noise_rate_cov_decades=0.1, seed=0,
                 device="cuda", cols_per_thread=0, max_iters=64):
        self.height, self.width = int(height), int(width)
        if self.height < 1 or self.width < 1:
            raise ValueError("ThresholdSweep: height and width must be positive")
        self.thresholds = _thresholds(thresholds, "thresholds")
        self.neg_thresholds = self.thresholds.copy() if neg_thresholds is None else _thresholds(neg_thresholds, "neg_thresholds")
        if len(self.neg_thresholds) != len(self.thresholds):
            raise ValueError("ThresholdSweep: %d thresholds but %d neg_thresholds" % (len(self.thresholds), len(self.neg_thresholds)))
        if roi is None:
            roi = ((0, self.width - 1), (0, self.height - 1))
        try:
            (x0, x1), (y0, y1) = roi
            x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
        except (TypeError, ValueError):
            raise ValueError("ThresholdSweep: roi must be ((x0, x1), (y0, y1)), got %r" % (roi,))
        if not (0 <= x0 <= x1 < self.width and 0 <= y0 <= y1 < self.height):
            raise ValueError("ThresholdSweep: roi %r is empty or outside the %dx%d sensor" % (roi, self.width, self.height))
        self.roi = ((x0, x1), (y0, y1))
        self.sigma_thres = float(sigma_thres)
        self.cutoff_hz = float(cutoff_hz)
        self.leak_rate_hz = float(leak_rate_hz)
        self.refractory_period_s = float(refractory_period_s)
        self.leak_jitter_fraction = float(leak_jitter_fraction)
        self.noise_rate_cov_decades = float(noise_rate_cov_decades)
        for name in ("sigma_thres", "cutoff_hz", "leak_rate_hz", "refractory_period_s"):
            v = getattr(self, name)
            if not (math.isfinite(v) and v >= 0):
                raise ValueError("ThresholdSweep: %s must be finite and not negative, got %r" % (name, v))
        self.seed = int(seed)
        if int(cols_per_thread) not in (0, 4, 8, 16):
            raise ValueError("ThresholdSweep: cols_per_thread must be 0, 4, 8 or 16")
        self.cols_per_thread = int(cols_per_thread)
        self.max_iters = int(max_iters)
        self.device = torch.device(device)
        self.recomputed_columns = 0  # columns of the last run that took the emulator path
        # the streamed sweep (add_run / result / reset): two sets of state planes (lp [npx], base [T][npx]) that alternate as the
        # kernel's input and output, the counts and flags it adds to, the emulator shared by the rule-on columns
        self._planes = self._counts = self._rule = self._emu = None
        self.reset()

    @classmethod
    def from_emulator(cls, emu, thresholds, neg_thresholds=None, *, roi=None, height=None, width=None, device=None, **kw):
        """A sweep with the model parameters of an EventEmulator (its own thresholds are not used).  height / width default to the
        emulator's output_height / output_width.  ValueError for what the sweep does not model."""
        if float(getattr(emu, "shot_noise_rate_hz", 0.0) or 0.0) > 0:
            raise ValueError("ThresholdSweep: shot_noise_rate_hz > 0 is out of scope (shot events reset base_log_frame per column)")
        for attr, what in (("log_input", "hdr"), ("photoreceptor_noise", "photoreceptor_noise"), ("scidvs", "scidvs"),
                           ("csdvs_enabled", "cs_lambda_pixels / cs_tau_p_ms (centre-surround)")):
            if getattr(emu, attr, False):
                raise ValueError("ThresholdSweep: %s is out of scope" % what)
        if getattr(emu, "cs_lambda_pixels", None) is not None or getattr(emu, "cs_tau_p_ms", None) is not None:
            raise ValueError("ThresholdSweep: cs_lambda_pixels / cs_tau_p_ms (centre-surround) is out of scope")
        height = emu.output_height if height is None else height
        width = emu.output_width if width is None else width
        if height is None or width is None:
            raise ValueError("ThresholdSweep.from_emulator: the emulator has no output_height / output_width; pass height and width")
        return cls(height, width, thresholds, neg_thresholds, roi=roi, sigma_thres=emu.sigma_thres, cutoff_hz=emu.cutoff_hz,
                   leak_rate_hz=emu.leak_rate_hz, refractory_period_s=emu.refractory_period_s,
                   leak_jitter_fraction=emu.leak_jitter_fraction, noise_rate_cov_decades=emu.noise_rate_cov_decades,
                   seed=emu.seed, device=emu.device if device is None else device, **kw)

    # ------------------------------------------------------------------------------------------------------------ run
    def _check_frames(self, frames, t_frames, what="run", min_frames=2):
        if not torch.is_tensor(frames):
            raise ValueError("ThresholdSweep.%s: frames must be a device tensor [F,H,W] of uint8 (host arrays are not swept: "
                             "upload them once)" % what)
        if not frames.is_cuda:
            raise ValueError("ThresholdSweep.%s: frames are on the host; the sweep reads them from device memory" % what)
        if frames.dtype != torch.uint8:
            raise ValueError("ThresholdSweep.%s: frames must be uint8, got %s" % (what, frames.dtype))
        if frames.dim() != 3 or tuple(frames.shape[1:]) != (self.height, self.width):
            raise ValueError("ThresholdSweep.%s: frames must be [F,%d,%d], got %r" % (what, self.height, self.width, tuple(frames.shape)))
        t = np.array([float(v) for v in t_frames], dtype=np.float64)
        if len(t) != frames.shape[0]:
            raise ValueError("ThresholdSweep.%s: need one timestamp per frame" % what)
        if len(t) < min_frames:
            raise ValueError("ThresholdSweep.run: at least two frames (the first one initialises the emulator)" if min_frames == 2 else
                             "ThresholdSweep.add_run: a chunk has at least one frame")
        if not (np.all(np.isfinite(t)) and t[0] >= 0 and np.all(np.diff(t) > 0)):
            raise ValueError("ThresholdSweep.%s: frame times must be finite, not negative and increasing" % what)
        return t

    def run(self, frames, t_frames):
        """frames: uint8 [F,H,W] on the device; t_frames[F].  Enqueued on the current stream behind whatever produced the frames;
        returns a SweepResult (the counts are read back, so the call waits for them)."""
        t = self._check_frames(frames, t_frames)
        _capi.require_gpu("ThresholdSweep")
        lib = _capi.lib()
        dev = frames.device
        frames = frames.contiguous()
        F, T = int(frames.shape[0]), len(self.thresholds)
        P = self._sweep_params()
        (x0, x1), (y0, y1) = self.roi
        with torch.cuda.device(dev):
            counts = torch.empty((T, 2), dtype=torch.int64, device=dev)
            rule = torch.empty((T,), dtype=torch.int32, device=dev)
            check(lib.v2e_thres_sweep(C.c_void_p(frames.data_ptr()), _capi.DT_U8, F, self.height, self.width,
                                      t.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P),
                                      self.thresholds.ctypes.data_as(C.POINTER(C.c_double)),
                                      self.neg_thresholds.ctypes.data_as(C.POINTER(C.c_double)), T,
                                      (C.c_int * 4)(x0, x1, y0, y1), C.c_void_p(counts.data_ptr()), C.c_void_p(rule.data_ptr()),
                                      _capi.stream_ptr(dev)), "v2e_thres_sweep")
            counts_h = counts.cpu().numpy()
            rule_on = rule.cpu().numpy() != 0
            on, off = counts_h[:, 0].copy(), counts_h[:, 1].copy()
            for j in np.nonzero(rule_on)[0]:
                on[j], off[j] = self._recompute_column(int(j), frames, t)
        self.recomputed_columns = int(rule_on.sum())
        return SweepResult(on, off, rule_on)

    def _sweep_params(self):
        P = _capi.SweepParams()
        P.sigma_thres, P.cutoff_hz, P.leak_rate_hz = self.sigma_thres, self.cutoff_hz, self.leak_rate_hz
        P.leak_jitter_fraction, P.noise_rate_cov_decades = self.leak_jitter_fraction, self.noise_rate_cov_decades
        P.refractory_period_s = self.refractory_period_s
        P.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        P.cols_per_thread = self.cols_per_thread
        return P

    def _new_emulator(self, j, device):
        """The emulator column j is: Philox mode, the sweep's model parameters, no shot noise."""
        from .emulator import EventEmulator
        return EventEmulator(pos_thres=float(self.thresholds[j]), neg_thres=float(self.neg_thresholds[j]), sigma_thres=self.sigma_thres,
                             cutoff_hz=self.cutoff_hz, leak_rate_hz=self.leak_rate_hz, refractory_period_s=self.refractory_period_s,
                             shot_noise_rate_hz=0.0, leak_jitter_fraction=self.leak_jitter_fraction,
                             noise_rate_cov_decades=self.noise_rate_cov_decades, seed=self.seed, device=str(device),
                             rng_mode="philox", max_iters=self.max_iters)

    def _recompute_column(self, j, frames, t):
        """The exact path of a column in which the refractory rule switched on: a fresh Philox-mode emulator over the same frames, in
        blocks (it carries its state from run to run), its rows counted in the ROI on the device."""
        emu = self._new_emulator(j, frames.device)
        try:
            acc = torch.zeros((2,), dtype=torch.int64, device=frames.device)
            for a in range(0, len(t), RECOMPUTE_BLOCK_FRAMES):
                b = min(a + RECOMPUTE_BLOCK_FRAMES, len(t))
                ev, _ = emu.generate_events_batch(frames[a:b], t[a:b], return_device=True)
                acc += count_rows_in_roi(ev, self.roi)  # (before the next run reuses the event buffer)
            on, off = (int(v) for v in acc.cpu().tolist())
        finally:
            emu.cleanup()
        return on, off

    # ------------------------------------------------------------------------------------------------------- streamed
    def reset(self):
        """Ready for the next clip: the carried state, the counts and the flags start over, and the emulator of the rule-on columns
        is released with the planes kept for them."""
        self.frames_seen = 0  # frames of the clip swept so far
        self.host_syncs = 0   # read-backs add_run and result have waited for (the runs of a rule-on column's emulator wait besides)
        self._t_last = None   # the time of the last frame swept
        self._cur = 0         # which set of state planes holds the state behind the last frame swept
        self._cols = {}       # column -> _EmuColumn, in the order the columns left the kernel
        self._rule_on_from = np.full(len(self.thresholds), -1, dtype=np.int64)
        if self._counts is not None:
            self._counts.zero_()
            self._rule.zero_()
        if self._emu is not None:
            self._emu.cleanup()
            self._emu = None

    def add_run(self, frames, t_frames, frame0=None):
        """The clip's next chunk: frames uint8 [F,H,W] on the device, F >= 1, with their F times.  The first call after
        construction or reset() brings the clip's first frames; every later one continues where the one before ended (frame0, when
        given, is the number of frames swept so far, and the times go on increasing: `check_continuation`).  The signature is that
        of the `on_frames` hook of VideoToEvents.run_stream and SyntheticToEvents.run.

        Enqueued on the current stream behind whatever produced the frames; every call of a clip is to be made on the same stream
        (or ordered behind the one before by the caller).  The frames have been read when the work enqueued here has run, so a
        producer that reuses their buffer orders that behind the current stream.  With refractory_period_s == 0 no flag can rise
        and the call does not wait for the device.  Otherwise it reads the T flags back (one small read-back, counted in
        host_syncs), and a column whose flag has risen is computed by the emulator from the start of this chunk on, for the rest
        of the clip (module docstring); those runs wait for their events."""
        t = self._check_frames(frames, t_frames, "add_run", 1)
        frame0 = check_continuation(self.frames_seen, self._t_last, t, frame0)
        _capi.require_gpu("ThresholdSweep")
        lib = _capi.lib()
        dev = frames.device
        frames = frames.contiguous()
        F, T, npx = int(frames.shape[0]), len(self.thresholds), self.height * self.width
        P = self._sweep_params()
        (x0, x1), (y0, y1) = self.roi
        refr = self.refractory_period_s > 0
        # the emulator's t_previous when it is given the chunk's first frame: the clip's first frame does not advance it
        t_prev = float(self._t_last) if frame0 > 1 else 0.0
        with torch.cuda.device(dev):
            if self._planes is not None and self._counts.device != dev:
                if self.frames_seen:
                    raise ValueError("ThresholdSweep.add_run: the clip's state is on %s, this chunk on %s" % (self._counts.device, dev))
                self._planes = None
            if self._planes is None:
                R = torch.float64 if self.cutoff_hz > 0 else torch.float32
                self._planes = [(torch.empty((npx,), dtype=R, device=dev), torch.empty((T, npx), dtype=R, device=dev)) for _ in range(2)]
                self._counts = torch.zeros((T, 2), dtype=torch.int64, device=dev)
                self._rule = torch.zeros((T,), dtype=torch.int32, device=dev)
            (lp_in, base_in), (lp_out, base_out) = self._planes[self._cur], self._planes[1 - self._cur]
            before = self._counts.clone() if refr else None  # what a column that leaves the kernel in this chunk keeps
            check(lib.v2e_thres_sweep_chunk(C.c_void_p(frames.data_ptr()), _capi.DT_U8, F, self.height, self.width,
                                            t.ctypes.data_as(C.POINTER(C.c_double)), frame0, t_prev, C.byref(P),
                                            self.thresholds.ctypes.data_as(C.POINTER(C.c_double)),
                                            self.neg_thresholds.ctypes.data_as(C.POINTER(C.c_double)), T,
                                            (C.c_int * 4)(x0, x1, y0, y1), C.c_void_p(lp_in.data_ptr()), C.c_void_p(base_in.data_ptr()),
                                            C.c_void_p(lp_out.data_ptr()), C.c_void_p(base_out.data_ptr()),
                                            C.c_void_p(self._counts.data_ptr()), C.c_void_p(self._rule.data_ptr()),
                                            _capi.stream_ptr(dev)), "v2e_thres_sweep_chunk")
            if refr:
                rule_on = self._rule.cpu().numpy() != 0
                self.host_syncs += 1
                for j in (int(j) for j in np.nonzero(rule_on)[0] if int(j) not in self._cols):
                    # the state the kernel read is still there (it writes the other set): exact, the rule never having been on
                    self._cols[j] = _EmuColumn(before[j].clone(), None if frame0 == 0 else base_in[j].clone())
                    self._rule_on_from[j] = frame0
                if self._cols:
                    self._advance_columns(frames, t, frame0, t_prev, None if frame0 == 0 else lp_in)
        self._cur ^= 1
        self.frames_seen += F
        self._t_last = float(t[-1])

    def result(self):
        """A SweepResult of all frames swept so far: what `run` returns for them as one clip.  The one read-back of the counts
        (counted in host_syncs); the sweep goes on with the next add_run."""
        T = len(self.thresholds)
        rule_on = np.zeros(T, dtype=bool)
        rule_on[list(self._cols)] = True
        if self._counts is None:
            return SweepResult(np.zeros(T, np.int64), np.zeros(T, np.int64), rule_on, self._rule_on_from.copy())
        with torch.cuda.device(self._counts.device):
            host = torch.cat([self._counts.reshape(-1)] + [col.acc for col in self._cols.values()]).cpu().numpy()
        self.host_syncs += 1
        on, off = host[0:2 * T:2].copy(), host[1:2 * T:2].copy()
        for k, j in enumerate(self._cols):  # the kernel's additions since the column left it are not the column's
            on[j], off[j] = host[2 * T + 2 * k], host[2 * T + 2 * k + 1]
        return SweepResult(on, off, rule_on, self._rule_on_from.copy())

    def _advance_columns(self, frames, t, frame0, t_prev, lp):
        """The rule-on columns through the chunk, by the emulator itself (Philox mode) in blocks of RECOMPUTE_BLOCK_FRAMES frames,
        their rows counted in the ROI.  One emulator serves them all: between two runs its handle keeps nothing of a column but
        the six state planes it was bound (v2e_emu_bind_state; the second set of planes a refractory chain alternates with is
        copied back before a run ends) -- of which lp_log_frame and the noise rate are the same in every column -- and the host
        object keeps the thresholds, the frame counter and t_previous.  So per block every column's four own planes are copied in
        and out around its run, and device memory grows by those planes per column, not by an emulator with its event buffers.
        lp: lp_log_frame [H*W] at the start of the chunk (the kernel's carried plane; None: the chunk begins the clip)."""
        if self._emu is None:
            self._emu = self._new_emulator(next(iter(self._cols)), frames.device)
        emu, npx = self._emu, self.height * self.width
        for a in range(0, len(t), RECOMPUTE_BLOCK_FRAMES):
            b = min(a + RECOMPUTE_BLOCK_FRAMES, len(t))
            lp_next = None
            for j, col in self._cols.items():
                self._load_column(emu, j, col, frame0 + a, t_prev, lp, frames[a])
                ev, _ = emu.generate_events_batch(frames[a:b], t[a:b], return_device=True)
                if ev is not None and ev.shape[0]:
                    col.acc += count_rows_in_roi(ev, self.roi)  # (before the next run reuses the event buffer)
                eng = emu._engine
                own = (eng.base, eng.ts_mem, eng.pos_thres, eng.neg_thres)
                if col.planes is None:
                    col.planes, col.base0 = [x.clone() for x in own], None
                else:
                    for dst, src in zip(col.planes, own):
                        dst.copy_(src)
                if lp_next is None:
                    lp_next = eng.lp[0, :npx].clone()
            lp = lp_next
            t_prev = float(t[b - 1]) if frame0 + b > 1 else 0.0

    def _load_column(self, emu, j, col, g0, t_prev, lp, frame):
        """The shared emulator becomes column j about to be given the clip's frame g0."""
        pj, nj = float(self.thresholds[j]), float(self.neg_thresholds[j])
        npx = self.height * self.width
        if col.planes is None:
            # the column's first block: a fresh emulator -- which is all there is to it when the column left the kernel in the
            # clip's first chunk.  Otherwise its first-frame step draws the column's threshold planes and the noise rate (k_init)
            # and leaves timestamp_mem zero, untouched as the kernel's invariant has it; lp and base are then the carried ones
            emu.reset()
            emu.pos_thres = emu.pos_thres_nominal = pj
            emu.neg_thres = emu.neg_thres_nominal = nj
            emu.t_previous = 0
            if g0 == 0:
                return
            emu._first_frame(frame, self.height, self.width, 0.0)
            emu._engine.base[0, :npx].copy_(col.base0)
        else:
            eng = emu._engine
            for dst, src in zip((eng.base, eng.ts_mem, eng.pos_thres, eng.neg_thres), col.planes):
                dst.copy_(src)
            emu.pos_thres_nominal, emu.neg_thres_nominal = pj, nj
            emu._thres_scalar = (pj, nj)
            if not self.sigma_thres > 0:
                emu.pos_thres, emu.neg_thres = pj, nj
        emu._engine.lp[0, :npx].copy_(lp)
        emu.frame_counter, emu.t_previous = g0, t_prev


def count_rows_in_roi(ev, roi):
    """[ON, OFF] (device int64 [2]) of the device rows ev [N,4] = (t, x, y, p) with x0 <= x <= x1 and y0 <= y <= y1."""
    (x0, x1), (y0, y1) = roi
    if ev is None or ev.shape[0] == 0:
        return torch.zeros((2,), dtype=torch.int64, device=None if ev is None else ev.device)
    x, y, p = ev[:, 1], ev[:, 2], ev[:, 3]
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    return torch.stack(((inside & (p > 0)).sum(), (inside & (p < 0)).sum()))


def estimate_thresholds(result, thresholds, dvs_on_count, dvs_off_count):
    """ddd_find_thresholds.py:147-155 in the order the thresholds were given: the threshold whose ON (OFF) count is nearest the
    recording's, absolute differences, strict `<`, so the first minimum wins.  Returns (pos_thres, neg_thres, on_diffs, off_diffs);
    the thresholds are None when `thresholds` is empty, as the reference's loop would leave them."""
    thresholds = [float(v) for v in thresholds]
    on, off = np.asarray(result.on), np.asarray(result.off)
    if len(on) != len(thresholds) or len(off) != len(thresholds):
        raise ValueError("estimate_thresholds: %d thresholds but %d / %d counts" % (len(thresholds), len(on), len(off)))
    min_pos_diff = min_neg_diff = math.inf
    pos_thres = neg_thres = None
    on_diffs, off_diffs = [], []
    for j, thres in enumerate(thresholds):
        abs_pos_diff = abs(int(on[j]) - int(dvs_on_count))
        abs_neg_diff = abs(int(off[j]) - int(dvs_off_count))
        on_diffs.append(abs_pos_diff)
        off_diffs.append(abs_neg_diff)
        if abs_pos_diff < min_pos_diff:
            min_pos_diff = abs_pos_diff
            pos_thres = thres
        if abs_neg_diff < min_neg_diff:
            min_neg_diff = abs_neg_diff
            neg_thres = thres
    return pos_thres, neg_thres, np.asarray(on_diffs, dtype=np.int64), np.asarray(off_diffs, dtype=np.int64)
