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

Out of scope: shot noise (it resets base_log_frame per column and adds rows), hdr, float frames, photoreceptor_noise, SCIDVS,
CSDVS, tape mode, a clip streamed across several `run` calls, per-frame or per-pixel count maps, reading recordings.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from ._capi import check

RECOMPUTE_BLOCK_FRAMES = 32  # frames per emulator run when a rule-on column is recomputed (bounds the event buffer)


class SweepResult(object):
    """on, off: numpy int64 [T]; rule_on: numpy bool [T], True where the column was recomputed by the emulator because the
    refractory rule switched on."""

    def __init__(self, on, off, rule_on):
        self.on, self.off, self.rule_on = on, off, rule_on

    def __repr__(self):
        return "SweepResult(on=%r, off=%r, rule_on=%r)" % (self.on, self.off, self.rule_on)


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
    def _check_frames(self, frames, t_frames):
        if not torch.is_tensor(frames):
            raise ValueError("ThresholdSweep.run: frames must be a device tensor [F,H,W] of uint8 (host arrays are not swept: "
                             "upload them once)")
        if not frames.is_cuda:
            raise ValueError("ThresholdSweep.run: frames are on the host; the sweep reads them from device memory")
        if frames.dtype != torch.uint8:
            raise ValueError("ThresholdSweep.run: frames must be uint8, got %s" % (frames.dtype,))
        if frames.dim() != 3 or tuple(frames.shape[1:]) != (self.height, self.width):
            raise ValueError("ThresholdSweep.run: frames must be [F,%d,%d], got %r" % (self.height, self.width, tuple(frames.shape)))
        t = np.array([float(v) for v in t_frames], dtype=np.float64)
        if len(t) != frames.shape[0]:
            raise ValueError("ThresholdSweep.run: need one timestamp per frame")
        if len(t) < 2:
            raise ValueError("ThresholdSweep.run: at least two frames (the first one initialises the emulator)")
        if not (np.all(np.isfinite(t)) and t[0] >= 0 and np.all(np.diff(t) > 0)):
            raise ValueError("ThresholdSweep.run: frame times must be finite, not negative and increasing")
        return t

    def run(self, frames, t_frames):
        """frames: uint8 [F,H,W] on the device; t_frames[F].  Enqueued on the current stream behind whatever produced the frames;
        returns a SweepResult (the counts are read back, so the call waits for them)."""
        t = self._check_frames(frames, t_frames)
        if not torch.cuda.is_available():
            raise _capi.V2EAmdError("v2e_amd.ThresholdSweep needs a ROCm GPU; there is no CPU fallback")
        lib = _capi.lib()
        dev = frames.device
        frames = frames.contiguous()
        F, T = int(frames.shape[0]), len(self.thresholds)
        P = _capi.SweepParams()
        P.sigma_thres, P.cutoff_hz, P.leak_rate_hz = self.sigma_thres, self.cutoff_hz, self.leak_rate_hz
        P.leak_jitter_fraction, P.noise_rate_cov_decades = self.leak_jitter_fraction, self.noise_rate_cov_decades
        P.refractory_period_s = self.refractory_period_s
        P.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        P.cols_per_thread = self.cols_per_thread
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

    def _recompute_column(self, j, frames, t):
        """The exact path of a column in which the refractory rule switched on: a fresh Philox-mode emulator over the same frames, in
        blocks (it carries its state from run to run), its rows counted in the ROI on the device."""
        from .emulator import EventEmulator
        emu = EventEmulator(pos_thres=float(self.thresholds[j]), neg_thres=float(self.neg_thresholds[j]), sigma_thres=self.sigma_thres,
                            cutoff_hz=self.cutoff_hz, leak_rate_hz=self.leak_rate_hz, refractory_period_s=self.refractory_period_s,
                            shot_noise_rate_hz=0.0, leak_jitter_fraction=self.leak_jitter_fraction,
                            noise_rate_cov_decades=self.noise_rate_cov_decades, seed=self.seed, device=str(frames.device),
                            rng_mode="philox", max_iters=self.max_iters)
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
