"""Double-window-filter ROC next to the rows: `DoubleWindowSweep` scores the double-window filter (DWF of the DND21 denoising
benchmark, jAER's DoubleWindowFilter) against the emulator's signal / noise labels for every (L, sigma, k) of three tables, and hands
out the keep-mask of one of them.  It is the filter the paper recommends for memory-starved hardware: no per-pixel map, and, unlike
the fixed-window filter (`WindowSweep`), a burst of noise cannot flush the real events out of the filter's memory.

Rows are what every run hands out: device float32 [n,4] = (t, x = column, y = row, p), taken in row order; neither p nor the value
of t is used.  A row is bad under exactly WindowSweep's rule (row_pixel of v2e_amd/csrc/rowkeys.h: t not finite, or x / y not an
integer value inside [0,W) / [0,H)): it is counted in n_bad, enters no window and no count and gets keep = False.  The valid rows
of all `add_run` calls since construction or `reset()` form one stream.

A setting is (L, sigma, k).  It owns two windows, R ("real") and N ("noise"); each holds the (x, y) of at most L rows and both
start empty.  For a valid row at (x, y), c = #{w in R u N : |x - w.x| + |y - w.y| <= sigma} (L1 distance; a row at the same pixel
counts), and the row passes iff c >= k.  A passing row is appended to R, a failing row to N, and a window that now holds L + 1 rows
drops its oldest: every row enters exactly one window, and the first row of a stream always fails.  Each window has L entries, so
the filter remembers 2 L rows: the fair fixed-window comparison of DWF(L) is FWF(2 L).  For every setting of the three tables
passed[ki, s, li, label] += 1 for a passing valid row (label 1 = signal, 0 = noise); with the per-label totals of valid rows that
is the ROC of every setting.

The verdict feeds back into the windows, so one setting is a serial chain over the rows; the settings of a sweep are independent
chains, and one wavefront runs each (v2e_amd/csrc/dwindow.hip): it holds the setting's 2 L window words on chip, takes the pass's
compacted words 64 at a time and compares each row against 64 window words per step.  The windows and their positions are carried
in device memory, one wave owns a setting's counters and every sum is an integer, so the result depends on the row order only: a
clip cut into several calls, or a call cut into row blocks (`max_rows_per_pass`), gives identical results.  `add_run` fits the
`on_events` callbacks of `VideoToEvents.run_stream` and `SyntheticToEvents.run`; it enqueues on the current stream and never waits
for the device: the number of valid rows stays in device memory.

A pass is one kernel that is serial in its rows: 509 ns per row with windows of 512 on an MI355X, whatever the number of settings
(profiles/r28_double_window_sweep.txt), which is why the default `max_rows_per_pass`, 2^18 (0.13 s per pass at that rate), is
smaller than the other sweeps'.  Scratch per row of a pass: 4 bytes of packed words, 4 of row indices and 1
of labels, 4 more per 256 rows; 1 byte more per row of the call with a keep mask or bool labels.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi, _rowpasses
from ._capi import check, ptr, stream_ptr
from ._roc import RocResult
from .window import MAX_LENGTHS, MAX_SIDE, MAX_SIGMA, MAX_SIGMAS, MAX_SUPPORT, XY_NONE, check_keep, int_table

MAX_LENGTH = 512
DEFAULT_ROWS_PER_PASS = 1 << 18
WHO = "DoubleWindowSweep"


class DoubleWindowResult(RocResult):
    """The counts of a `DoubleWindowSweep` on the host, and the ROC they hold.

    passed    int64 [NK,S,NL,2]: passed[ki, s, li, label] valid rows that pass DWF(lengths[li], sigmas[s], supports[ki])
              (label 1 = signal, 0 = noise)
    lengths   int64 [NL]
    sigmas    int64 [S]
    supports  int64 [NK]
    n_signal, n_noise, n_bad   valid signal rows, valid noise rows, bad rows
    tpr, fpr  float64 [NK,S,NL]: passed signal rows / n_signal, passed noise rows / n_noise; NaN where the denominator is 0
    """

    LABEL_AXIS = -1

    def __init__(self, passed, lengths, sigmas, supports, n_signal, n_noise, n_bad=0):
        self.lengths = np.array(lengths, dtype=np.int64).reshape(-1)
        self.sigmas = np.array(sigmas, dtype=np.int64).reshape(-1)
        self.supports = np.array(supports, dtype=np.int64).reshape(-1)
        self.passed = np.array(passed, dtype=np.int64)
        shape = (len(self.supports), len(self.sigmas), len(self.lengths), 2)
        if self.passed.shape != shape:
            raise ValueError("DoubleWindowResult: passed must be [%d, %d, %d, 2], got %r" % (shape[:3] + (self.passed.shape,)))
        self.n_signal, self.n_noise, self.n_bad = int(n_signal), int(n_noise), int(n_bad)

    def best(self):
        """(L, sigma, k, tpr, fpr) at the first maximum of tpr - fpr, taken in (k ascending, sigma ascending, L ascending) order.
        ValueError when there is no signal or no noise row (tpr - fpr is NaN everywhere)."""
        (ki, s, li), tpr, fpr = self._best("DoubleWindowResult")
        return int(self.lengths[li]), int(self.sigmas[s]), int(self.supports[ki]), tpr, fpr


class DoubleWindowSweep(object):
    """DWF true- and false-positive counts of a clip for every support, sigma and window length of three tables, from the device
    rows of its runs (module docstring)."""

    def __init__(self, height, width, lengths, sigmas, supports=(1, 2, 3, 4), max_rows_per_pass=DEFAULT_ROWS_PER_PASS, device="cuda:0"):
        self.height, self.width = int(height), int(width)
        if not (1 <= self.height <= MAX_SIDE and 1 <= self.width <= MAX_SIDE):  # (no per-pixel map: no limit on height * width)
            raise ValueError("%s: height and width must be in 1 .. %d" % (WHO, MAX_SIDE))
        self.lengths = int_table(WHO, "lengths", lengths, MAX_LENGTHS, 1, MAX_LENGTH)
        self.sigmas = int_table(WHO, "sigmas", sigmas, MAX_SIGMAS, 0, MAX_SIGMA)
        self.supports = int_table(WHO, "supports", supports, MAX_SUPPORT, 1, MAX_SUPPORT)
        self.max_length = int(self.lengths[-1])
        self.max_rows_per_pass = _rowpasses.check_rows_per_pass(WHO, max_rows_per_pass)
        self.device = torch.device(device)
        self.passes = 0        # row blocks processed so far
        self._state = None     # the device buffers, allocated by the first call that needs them
        self._tables_c = tuple((C.c_int32 * len(t))(*[int(v) for v in t]) for t in (self.lengths, self.sigmas, self.supports))

    @property
    def n_settings(self):
        return len(self.supports) * len(self.sigmas) * len(self.lengths)

    # ------------------------------------------------------------------------------------------------------------ device state
    def _dev(self):
        if self._state is None:
            _capi.require_gpu(WHO)
            dev, F = self.device, self.n_settings
            self._state = {
                # (uint32 words: -1 is XY_NONE) the rings of R and N of every setting, and the slot each one's next row goes to
                "rings": torch.full((F, 2, self.max_length), -1, dtype=torch.int32, device=dev),
                "pos": torch.zeros((F, 2), dtype=torch.int32, device=dev),
                # passed [F][2], then valid noise rows, valid signal rows, then valid rows, bad rows
                "counts": torch.zeros((2 * F + 4,), dtype=torch.int64, device=dev),
                "tail": torch.full((1,), -1, dtype=torch.int32, device=dev),  # the one-word tail the compaction copies along
            }
        return self._state

    def reset(self):
        """All windows back to empty and all counts to zero (enqueued on the current stream)."""
        if self._state is not None:
            self._state["rings"].fill_(-1)
            self._state["pos"].zero_()
            self._state["counts"].zero_()

    @property
    def windows(self):
        """The carried windows, int64 [NK,S,NL,2,Lmax] on the device, index 0 = R and 1 = N: the words x | y << 16 of the rows each
        window holds, the latest last, with 0xffffffff in front where it holds fewer than Lmax rows (a setting with L < Lmax has at
        least Lmax - L such words): a copy."""
        st = self._dev()
        dev, lmax = self.device, self.max_length
        L = torch.from_numpy(self.lengths).to(dev).view(1, 1, -1, 1, 1)
        rings = st["rings"].view(len(self.supports), len(self.sigmas), len(self.lengths), 2, lmax).to(torch.int64) & XY_NONE
        pos = st["pos"].view(len(self.supports), len(self.sigmas), len(self.lengths), 2, 1).to(torch.int64)
        j = torch.arange(lmax, device=dev).view(1, 1, 1, 1, -1) - (lmax - L)  # the age rank inside the window: 0 = its oldest slot
        out = torch.gather(rings, 4, (pos + j.clamp(min=0)) % L)                # (a ring's oldest slot is the one at pos)
        return torch.where(j >= 0, out, torch.full_like(out, XY_NONE))

    # ------------------------------------------------------------------------------------------------------------ the run
    def _keep_indices(self, keep):
        """keep = (L, sigma, k) as its indices in the three tables: its windows have to be carried, so it must be a setting."""
        at = []
        for name, table, v in zip(("L", "sigma", "k"), (self.lengths, self.sigmas, self.supports), keep):
            hit = np.flatnonzero(table == v)
            if len(hit) == 0:
                raise ValueError("%s.add_run: keep's %s must be an entry of the sweep's table, got %r" % (WHO, name, v))
            at.append(int(hit[0]))
        return at

    def add_run(self, rows, counts=None, frame0=0, n_signal=None, labels=None, keep=None):
        """Add one run's rows (device float32 [n,4]; None or empty: nothing happens) to the counts and the windows.

        The rows' labels: `labels`, a bool [n] tensor or array on the device or the host, True = signal; or `n_signal` with
        `counts` (per frame of the run: its first n_signal[f] of counts[f] rows are signal, what EventEmulator.last_n_signal and
        a run's counts are); with neither every row counts as signal.  frame0 is not needed and ignored: the signature is
        on_events'.  keep=(L, sigma, k): also return that setting's verdicts; unlike WindowSweep's, it must be an entry of all
        three tables, because its windows are carried.
        Returns {"n": valid rows, "n_bad": bad rows, "mask": bool [n] or None}: n and n_bad are 0-dim int64 device tensors (reading
        one waits for the device; the call does not), mask a device tensor in the rows' order."""
        # every ValueError before the library or the device is touched
        keep = check_keep(WHO, keep, self.max_length)
        keep_at = None if keep is None else self._keep_indices(keep)
        n, labels, bounds = _rowpasses.check_run(WHO, rows, counts, n_signal, labels, host_error=TypeError)
        st = self._dev()
        dev = self.device
        if n == 0:
            return _rowpasses.no_rows(dev, mask=True, keep=keep)
        rows = rows.to(dev).contiguous()
        lib = _capi.lib()
        stream = stream_ptr(dev)
        F = self.n_settings
        lengths_c, sigmas_c, supports_c = self._tables_c
        lab, lb = _rowpasses.labels_to_device(labels, bounds, dev)
        mask = _rowpasses.new_mask(keep, n, dev)
        keep_li, keep_si, keep_ki = keep_at if keep_at is not None else (0, 0, 0)
        passed, totals, seen = st["counts"][:2 * F], st["counts"][2 * F:2 * F + 2], st["counts"][2 * F + 2:]
        run = _rowpasses.WindowPasses(self, rows, st["tail"], seen, keep=mask)
        for r0, m, xy, idx, n_valid in run:
            row_lab = torch.empty((m,), dtype=torch.uint8, device=dev)
            check(lib.v2e_dwindow_labels(ptr(idx), m, ptr(n_valid), *_rowpasses.label_args(lab, lb, r0), ptr(row_lab), ptr(totals),
                                         stream), "v2e_dwindow_labels")
            check(lib.v2e_dwindow_sweep(ptr(xy), ptr(idx), ptr(row_lab), m, ptr(n_valid), lengths_c, len(self.lengths), sigmas_c,
                                        len(self.sigmas), supports_c, len(self.supports), ptr(st["rings"]), ptr(st["pos"]), ptr(passed),
                                        run.keep_ptr(r0), keep_li, keep_si, keep_ki, stream), "v2e_dwindow_sweep")
        return {"n": run.n, "n_bad": run.n_bad, "mask": None if mask is None else mask.view(torch.bool)}

    def result(self):
        """The counts so far as a DoubleWindowResult: one small read-back (it waits for the runs enqueued so far)."""
        st = self._dev()
        flat = st["counts"].cpu().numpy()
        shape = (len(self.supports), len(self.sigmas), len(self.lengths), 2)
        return DoubleWindowResult(flat[:-4].reshape(shape), self.lengths, self.sigmas, self.supports, n_signal=int(flat[-3]),
                                  n_noise=int(flat[-4]), n_bad=int(flat[-1]))
