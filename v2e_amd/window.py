"""Window-filter ROC next to the rows: `WindowSweep` scores the fixed-window filter (FWF of the DND21 denoising benchmark) against
the emulator's signal / noise labels for every (L, sigma, k) in one pass over the rows of device-resident runs, and hands out the
keep-mask of one chosen (L, sigma, k).  The filter keeps no per-pixel map: it remembers the coordinates of the last L events and
passes a new one when at least k of them lie within a spatial distance sigma.  The double-window filter of the same paper feeds its
own verdicts back into its windows, which makes it serial per parameter setting: `DoubleWindowSweep` (v2e_amd/dwindow.py) scores it.

Rows are what every run hands out: device float32 [n,4] = (t, x = column, y = row, p), taken in row order; neither p nor the value
of t is used.  A row is bad under exactly DenoiseSweep's rule (t not finite, or x / y not an integer value inside [0,W) / [0,H)):
it is counted in n_bad, never enters the window, enters no histogram and gets keep = False.  The valid rows of all `add_run` calls
since construction or `reset()` form one stream v_0, v_1, ...; with Lmax = lengths[-1] the window of v_m at (x, y) is v_{m-1}
(depth 1), ..., v_{m-D}, D = min(m, Lmax).  For each sigma_s of `sigmas` and k = 1 .. MAX_SUPPORT (4), d[s][k] is the smallest j
with #{1 <= i <= j : |x - x_{m-i}| + |y - y_{m-i}| <= sigma_s} >= k (L1 distance; a row at the same pixel counts), Lmax + 1 if the
window holds no such j.  The row passes FWF(L, sigma_s, k) iff d[s][k] <= L, so with bin(d) = searchsorted(lengths, d, 'left') one
histogram, hist[k-1, s, label, bin(d[s][k])] += 1 (int64 [4,S,2,NL+1], label 1 = signal, 0 = noise, bin NL = passes no length of
the table), holds the true- and false-positive rates of all 4 * S * NL filters.  After its depths are read the row enters the
window, whatever any filter says about it.

The filter is serial only through "the last Lmax valid rows".  Each pass compacts the packed words x | y << 16 of its valid rows,
in order, behind the Lmax words carried from the pass before (0xffffffff: no row yet), a workgroup stages 256 consecutive words and
the Lmax before them in LDS, and every thread walks back from its own (v2e_amd/csrc/window.hip); every sum is an integer atomic, so
the result depends on the row order only: a clip cut into several calls, or a call cut into row blocks (`max_rows_per_pass`),
gives identical results.  `add_run` fits the `on_events` callbacks of `VideoToEvents.run_stream` and `SyntheticToEvents.run`; it
enqueues on the current stream and never waits for the device: the number of valid rows stays in device memory.

Scratch per row of a pass: 4 bytes of packed words and 4 of row indices, 4 more per 256 rows; 1 byte more per row of the call with
a keep mask or bool labels.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi, _rowpasses
from ._capi import check, ptr, stream_ptr
from ._roc import RocResult
from ._rowpasses import DEFAULT_ROWS_PER_PASS

MAX_LENGTHS = 64
MAX_LENGTH = 1024
MAX_SIGMAS = 8
MAX_SIGMA = 65535
MAX_SUPPORT = 4
MAX_SIDE = 65535
XY_NONE = 0xFFFFFFFF  # the packed word of "no row yet"


def int_table(who, name, table, most, lo, hi):
    """`table` as an ascending int64 table of 1 .. most integers in lo .. hi; ValueError in the words of class `who`."""
    try:
        t = np.array(table, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be a table of integers" % (who, name)) from None
    if not 1 <= len(t) <= most:
        raise ValueError("%s: 1 to %d %s, got %d" % (who, most, name, len(t)))
    if not np.all(np.isfinite(t)) or np.any(t != np.floor(t)) or np.any(t < lo) or np.any(t > hi) or np.any(np.diff(t) <= 0):
        raise ValueError("%s: %s must be integers in %d .. %d, strictly ascending" % (who, name, lo, hi))
    return t.astype(np.int64)


def check_keep(who, keep, lmax):
    """keep = (L, sigma, k) of `who`.add_run as three ints, L in 1 .. lmax; None stays None."""
    if keep is None:
        return None
    try:
        length, sigma, k = keep
        ints = (int(length), int(sigma), int(k))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s.add_run: keep must be (L, sigma, k), got %r" % (who, keep,)) from None
    if ints != (length, sigma, k):
        raise ValueError("%s.add_run: keep's L, sigma and k must be integers, got %r" % (who, keep,))
    if not 1 <= ints[0] <= lmax:
        raise ValueError("%s.add_run: keep's L must be in 1 .. %d (the longest length), got %r" % (who, lmax, length))
    if ints[1] < 0:
        raise ValueError("%s.add_run: keep's sigma must be >= 0, got %r" % (who, sigma,))
    if not 1 <= ints[2] <= MAX_SUPPORT:
        raise ValueError("%s.add_run: keep's k must be in 1 .. %d, got %r" % (who, MAX_SUPPORT, k))
    return ints


class WindowResult(RocResult):
    """The histogram of a `WindowSweep` on the host, and the ROC it holds.

    hist      int64 [4,S,2,NL+1]: hist[k-1, s, label, b] rows whose depth d[s][k] falls in bin b (label 1 = signal, 0 = noise)
    lengths   int64 [NL]
    sigmas    int64 [S]
    n_signal, n_noise, n_bad   valid signal rows, valid noise rows, bad rows
    passed    int64 [4,S,2,NL]: rows that pass FWF(lengths[b], sigmas[s], k) -- the cumulative sum of hist over its first NL bins
    tpr, fpr  float64 [4,S,NL]: passed signal rows / n_signal, passed noise rows / n_noise; NaN where the denominator is 0
    """

    def __init__(self, hist, lengths, sigmas, n_bad=0):
        self.lengths = np.array(lengths, dtype=np.int64).reshape(-1)
        self.sigmas = np.array(sigmas, dtype=np.int64).reshape(-1)
        NL, S = len(self.lengths), len(self.sigmas)
        self.hist = np.array(hist, dtype=np.int64)
        if self.hist.shape != (MAX_SUPPORT, S, 2, NL + 1):
            raise ValueError("WindowResult: hist must be [%d, %d, 2, %d], got %r" % (MAX_SUPPORT, S, NL + 1, self.hist.shape))
        self.n_noise = int(self.hist[0, 0, 0].sum())
        self.n_signal = int(self.hist[0, 0, 1].sum())
        self.n_bad = int(n_bad)

    @property
    def passed(self):
        return np.cumsum(self.hist[:, :, :, :-1], axis=3)

    def best(self):
        """(L, sigma, k, tpr, fpr) at the first maximum of tpr - fpr, taken in (k ascending, sigma ascending, L ascending) order.
        ValueError when there is no signal or no noise row (tpr - fpr is NaN everywhere)."""
        (k, s, b), tpr, fpr = self._best("WindowResult")
        return int(self.lengths[b]), int(self.sigmas[s]), int(k) + 1, tpr, fpr


class WindowSweep(object):
    """FWF true- and false-positive counts of a clip for k = 1 .. 4, every sigma and every window length of two tables, from the
    device rows of its runs (module docstring)."""

    def __init__(self, height, width, lengths, sigmas, max_rows_per_pass=DEFAULT_ROWS_PER_PASS, device="cuda:0"):
        self.height, self.width = int(height), int(width)
        if not (1 <= self.height <= MAX_SIDE and 1 <= self.width <= MAX_SIDE):  # (no per-pixel map: no limit on height * width)
            raise ValueError("WindowSweep: height and width must be in 1 .. %d" % MAX_SIDE)
        self.lengths = int_table("WindowSweep", "lengths", lengths, MAX_LENGTHS, 1, MAX_LENGTH)
        self.sigmas = int_table("WindowSweep", "sigmas", sigmas, MAX_SIGMAS, 0, MAX_SIGMA)
        self.max_length = int(self.lengths[-1])
        self.max_rows_per_pass = _rowpasses.check_rows_per_pass("WindowSweep", max_rows_per_pass)
        self.device = torch.device(device)
        self.passes = 0        # row blocks processed so far
        self._state = None     # the device buffers, allocated by the first call that needs them
        self._sigmas_c = (C.c_int32 * len(self.sigmas))(*[int(s) for s in self.sigmas])

    # ------------------------------------------------------------------------------------------------------------ device state
    def _dev(self):
        if self._state is None:
            _capi.require_gpu("WindowSweep")
            dev, NL, S = self.device, len(self.lengths), len(self.sigmas)
            self._state = {
                "tail": torch.full((self.max_length,), -1, dtype=torch.int32, device=dev),  # (uint32 words: -1 is XY_NONE)
                "hist": torch.zeros((MAX_SUPPORT, S, 2, NL + 1), dtype=torch.int64, device=dev),
                "seen": torch.zeros((2,), dtype=torch.int64, device=dev),                   # valid rows, bad rows so far
                "lengths": torch.from_numpy(self.lengths.astype(np.int32)).to(dev),
            }
        return self._state

    def reset(self):
        """The window back to "no row yet", the histogram and the row counters to zero (enqueued on the current stream)."""
        if self._state is not None:
            self._state["tail"].fill_(-1)
            self._state["hist"].zero_()
            self._state["seen"].zero_()

    @property
    def tail(self):
        """The carried window, int64 [Lmax] on the device: the words x | y << 16 of the last Lmax valid rows, the latest last, with
        0xffffffff (no row yet) in front while the stream is shorter: a copy."""
        return self._dev()["tail"].to(torch.int64) & XY_NONE

    # ------------------------------------------------------------------------------------------------------------ the run
    def add_run(self, rows, counts=None, frame0=0, n_signal=None, labels=None, keep=None):
        """Add one run's rows (device float32 [n,4]; None or empty: nothing happens) to the histogram and the window.

        The rows' labels: `labels`, a bool [n] tensor or array on the device or the host, True = signal; or `n_signal` with
        `counts` (per frame of the run: its first n_signal[f] of counts[f] rows are signal, what EventEmulator.last_n_signal and
        a run's counts are); with neither every row counts as signal.  frame0 is not needed and ignored: the signature is
        on_events'.  keep=(L, sigma, k): also return the mask d <= L, d the depth for that sigma and k; L any integer in
        1 .. lengths[-1], sigma any integer >= 0, k in 1 .. 4, none of them necessarily a table entry.
        Returns {"n": valid rows, "n_bad": bad rows, "mask": bool [n] or None}: n and n_bad are 0-dim int64 device tensors (reading
        one waits for the device; the call does not), mask a device tensor in the rows' order."""
        # every ValueError before the library or the device is touched
        keep = check_keep("WindowSweep", keep, self.max_length)
        n, labels, bounds = _rowpasses.check_run("WindowSweep", rows, counts, n_signal, labels, host_error=TypeError)
        st = self._dev()
        dev = self.device
        if n == 0:
            return _rowpasses.no_rows(dev, mask=True, keep=keep)
        rows = rows.to(dev).contiguous()
        lib = _capi.lib()
        stream = stream_ptr(dev)
        NL, S, lmax = len(self.lengths), len(self.sigmas), self.max_length
        lab, lb = _rowpasses.labels_to_device(labels, bounds, dev)
        mask = _rowpasses.new_mask(keep, n, dev)
        keep_l, keep_sigma, keep_k = keep if keep is not None else (1, 0, 1)
        keep_sigma = min(keep_sigma, 1 << 31)  # (beyond every distance of a sensor: the same filter)
        run = _rowpasses.WindowPasses(self, rows, st["tail"], st["seen"], keep=mask)
        for r0, m, xy, idx, n_valid in run:
            check(lib.v2e_window_depths(ptr(xy), ptr(idx), m, ptr(n_valid), ptr(st["lengths"]), NL, lmax, self._sigmas_c, S,
                                        *_rowpasses.label_args(lab, lb, r0), ptr(st["hist"]), run.keep_ptr(r0), keep_l, keep_sigma,
                                        keep_k, stream), "v2e_window_depths")
            check(lib.v2e_window_tail(ptr(xy), ptr(n_valid), m, lmax, ptr(st["tail"]), stream), "v2e_window_tail")
        return {"n": run.n, "n_bad": run.n_bad, "mask": None if mask is None else mask.view(torch.bool)}

    def result(self):
        """The histogram so far as a WindowResult: one small read-back (it waits for the runs enqueued so far)."""
        st = self._dev()
        flat = torch.cat([st["hist"].reshape(-1), st["seen"]]).cpu().numpy()
        return WindowResult(flat[:-2].reshape(MAX_SUPPORT, len(self.sigmas), 2, len(self.lengths) + 1), self.lengths, self.sigmas,
                            int(flat[-1]))
