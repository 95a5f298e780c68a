"""Denoiser ROC next to the rows: `DenoiseSweep` scores the spatio-temporal correlation filter (STCF; with one supporting
neighbour jAER's BackgroundActivityFilter) against the emulator's signal / noise labels for every (k, tau) in one pass over the
rows of device-resident runs, and hands out the keep-mask of one chosen (k, tau).

Rows are what every run hands out: device float32 [n,4] = (t, x = column, y = row, p), processed in row order; p is not read.
A row is bad if t is not finite or x / y is not an integer value inside [0,W) / [0,H): it is counted in n_bad, neither reads nor
writes the map, enters no histogram and gets keep = False.  `last_t` is a float32 [H,W] map that starts at -inf and is carried
from call to call on the device.  For a valid row i at pixel (x, y), each of the 8 neighbours q inside the sensor (the centre is
excluded) gives age_q = float64(t_i) - float64(T_q), T_q the t of the latest row j < i at q in this call, else the carried
last_t[q]; a neighbour outside the sensor, or T_q = -inf, gives +inf; a neighbour whose latest time is later than t_i gives a
negative age, kept as it is.  a_1 <= ... <= a_8 are the eight ages sorted.  After its ages are read the row sets last_t[x,y] =
t_i, whether or not any filter would pass it (jAER's behaviour).  The row passes STCF(k, tau) iff a_k <= tau, so with
bin(a) = searchsorted(taus, a, 'left') one histogram, hist[k-1, label, bin(a_k)] += 1 (int64 [8,2,T+1], label 1 = signal, 0 =
noise, bin T = passes no tau of the table), holds the true- and false-positive rates of all 8 * T filters.

The filter is serial only through the map.  Each row gets the key pixel << 32 | row, the keys are sorted (torch.sort), and
"the latest earlier row at q" becomes a binary search in q's stretch of the sorted keys (v2e_amd/csrc/denoise.hip); every row
is then independent and every sum an integer atomic, so the result depends on the row order only: a clip cut into several calls,
or a call cut into row blocks (`max_rows_per_pass`), gives identical results.  `add_run` fits the `on_events` callbacks of
`VideoToEvents.run_stream` and `SyntheticToEvents.run`; it enqueues on the current stream and never waits for the device (the
sort allocates its scratch from torch's caching allocator).

Scratch per row of a pass: 8 bytes of keys, 16 of the sort's output (sorted keys and its int64 permutation, which is not used) and
24 of the sort's own buffers: 48 bytes at the peak (measured, profiles/r15_denoise_sweep.txt), 1.5 GiB at the default 2^25 rows per
pass; 1 byte more per row of the call with a keep mask or bool labels.
"""
import math

import numpy as np
import torch

from . import _capi, _rowpasses
from ._capi import check, ptr, stream_ptr
from ._roc import RocResult
from ._rowpasses import DEFAULT_ROWS_PER_PASS, label_bounds  # noqa: F401  (label_bounds: imported from here by users)

MAX_TAUS = 256
NEIGHBOURS = 8


def _check_taus(taus):
    t = np.array(taus, dtype=np.float64).reshape(-1)
    if not 1 <= len(t) <= MAX_TAUS:
        raise ValueError("DenoiseSweep: 1 to %d taus, got %d" % (MAX_TAUS, len(t)))
    if not np.all(np.isfinite(t)) or np.any(t < 0) or np.any(np.diff(t) <= 0):
        raise ValueError("DenoiseSweep: taus must be finite, >= 0 and strictly ascending")
    return t


def _check_keep(keep):
    if keep is None:
        return None
    try:
        k, tau = keep
        k_int, tau = int(k), float(tau)
    except (TypeError, ValueError):
        raise ValueError("DenoiseSweep.add_run: keep must be (k, tau), got %r" % (keep,)) from None
    if k_int != k or not 1 <= k_int <= NEIGHBOURS:
        raise ValueError("DenoiseSweep.add_run: keep's k must be an integer in 1 .. %d, got %r" % (NEIGHBOURS, k))
    if not (tau >= 0) or math.isnan(tau):
        raise ValueError("DenoiseSweep.add_run: keep's tau must be >= 0, got %r" % (tau,))
    return k_int, tau


class DenoiseResult(RocResult):
    """The histogram of a `DenoiseSweep` on the host, and the ROC it holds.

    hist      int64 [8,2,T+1]: hist[k-1, label, b] rows whose k-th smallest age falls in bin b (label 1 = signal, 0 = noise)
    taus      float64 [T]
    n_signal, n_noise, n_bad   valid signal rows, valid noise rows, bad rows
    passed    int64 [8,2,T]: rows that pass STCF(k, taus[b]) -- the cumulative sum of hist over its first T bins
    tpr, fpr  float64 [8,T]: passed signal rows / n_signal, passed noise rows / n_noise; NaN where the denominator is 0
    """

    def __init__(self, hist, taus, n_bad=0):
        self.taus = np.array(taus, dtype=np.float64).reshape(-1)
        T = len(self.taus)
        self.hist = np.array(hist, dtype=np.int64)
        if self.hist.shape != (NEIGHBOURS, 2, T + 1):
            raise ValueError("DenoiseResult: hist must be [%d, 2, %d], got %r" % (NEIGHBOURS, T + 1, self.hist.shape))
        self.n_noise = int(self.hist[0, 0].sum())
        self.n_signal = int(self.hist[0, 1].sum())
        self.n_bad = int(n_bad)

    @property
    def passed(self):
        return np.cumsum(self.hist[:, :, :-1], axis=2)

    def best(self):
        """(k, tau, tpr, fpr) at the first maximum of tpr - fpr, taken in (k ascending, tau ascending) order.  ValueError when there
        is no signal or no noise row (tpr - fpr is NaN everywhere)."""
        (k, b), tpr, fpr = self._best("DenoiseResult")
        return int(k) + 1, float(self.taus[b]), tpr, fpr


class DenoiseSweep(object):
    """STCF true- and false-positive counts of a clip for k = 1 .. 8 and every tau of a table, from the device rows of its runs
    (module docstring)."""

    def __init__(self, height, width, taus, max_rows_per_pass=DEFAULT_ROWS_PER_PASS, device="cuda:0"):
        self.height, self.width = _rowpasses.check_sensor("DenoiseSweep", height, width)
        self.taus = _check_taus(taus)
        self.max_rows_per_pass = _rowpasses.check_rows_per_pass("DenoiseSweep", max_rows_per_pass)
        self.device = torch.device(device)
        self.passes = 0        # row blocks processed so far
        self._state = None     # the device buffers, allocated by the first call that needs them

    # ------------------------------------------------------------------------------------------------------------ device state
    def _dev(self):
        if self._state is None:
            _capi.require_gpu("DenoiseSweep")
            dev, H, W, T = self.device, self.height, self.width, len(self.taus)
            self._state = {
                "last_t": torch.full((H, W), -math.inf, dtype=torch.float32, device=dev),
                "hist": torch.zeros((NEIGHBOURS, 2, T + 1), dtype=torch.int64, device=dev),
                "n_bad": torch.zeros((), dtype=torch.int64, device=dev),
                "taus": torch.from_numpy(self.taus).to(dev),
                "seg": _rowpasses.new_seg(H, W, dev),
            }
        return self._state

    def reset(self):
        """The map back to -inf, the histogram and n_bad to zero (enqueued on the current stream)."""
        if self._state is not None:
            self._state["last_t"].fill_(-math.inf)
            self._state["hist"].zero_()
            self._state["n_bad"].zero_()

    @property
    def last_t(self):
        """The carried map, float32 [H,W] on the device (-inf: no row yet): a copy."""
        return self._dev()["last_t"].clone()

    # ------------------------------------------------------------------------------------------------------------ the run
    def add_run(self, rows, counts=None, frame0=0, n_signal=None, labels=None, keep=None):
        """Add one run's rows (device float32 [n,4]; None or empty: nothing happens) to the histogram and the map.

        The rows' labels: `labels`, a bool [n] tensor or array on the device or the host, True = signal; or `n_signal` with
        `counts` (per frame of the run: its first n_signal[f] of counts[f] rows are signal, what EventEmulator.last_n_signal and
        a run's counts are); with neither every row counts as signal.  frame0 is not needed and ignored: the signature is
        on_events'.  keep=(k, tau): also return the mask a_k <= tau, tau any float64 >= 0.
        Returns {"n": valid rows, "n_bad": bad rows, "mask": bool [n] or None}: n and n_bad are 0-dim int64 device tensors (reading
        one waits for the device; the call does not), mask a device tensor in the rows' order."""
        # every ValueError before the library or the device is touched
        keep = _check_keep(keep)
        n, labels, bounds = _rowpasses.check_run("DenoiseSweep", rows, counts, n_signal, labels, host_error=TypeError)
        st = self._dev()
        dev = self.device
        if n == 0:
            return _rowpasses.no_rows(dev, mask=True, keep=keep)
        rows = rows.to(dev).contiguous()
        lib = _capi.lib()
        stream = stream_ptr(dev)
        H, W, T = self.height, self.width, len(self.taus)
        lab, lb = _rowpasses.labels_to_device(labels, bounds, dev)
        mask = _rowpasses.new_mask(keep, n, dev)
        k, tau = keep if keep is not None else (1, 0.0)
        run = _rowpasses.RowPasses(self, rows, st["seg"], keep=mask)
        for r0, m, ev, skeys in run:
            check(lib.v2e_denoise_ages(ptr(ev), m, H, W, ptr(skeys), ptr(st["seg"]), ptr(st["last_t"]), ptr(st["taus"]), T,
                                       *_rowpasses.label_args(lab, lb, r0), ptr(st["hist"]), run.keep_ptr(r0), k, tau, stream),
                  "v2e_denoise_ages")
            check(lib.v2e_denoise_map_update(ptr(ev), ptr(skeys), ptr(st["seg"]), H, W, ptr(st["last_t"]), stream),
                  "v2e_denoise_map_update")
        st["n_bad"] += run.n_bad
        return {"n": run.n, "n_bad": run.n_bad, "mask": None if mask is None else mask.view(torch.bool)}

    def result(self):
        """The histogram so far as a DenoiseResult: one small read-back (it waits for the runs enqueued so far)."""
        st = self._dev()
        flat = torch.cat([st["hist"].reshape(-1), st["n_bad"].reshape(1)]).cpu().numpy()
        return DenoiseResult(flat[:-1].reshape(NEIGHBOURS, 2, len(self.taus) + 1), self.taus, int(flat[-1]))


def denoise_rows(rows, counts, mask):
    """The rows a keep-mask keeps, in their order, and how many of each frame's: (rows[mask], counts_kept), counts_kept an int64
    array like `counts` (None for counts None).  Torch indexing and per-frame sums on the device; it waits for the device."""
    if not (torch.is_tensor(rows) and torch.is_tensor(mask)):
        raise TypeError("denoise_rows takes device tensors")
    if mask.dtype != torch.bool or mask.dim() != 1 or rows.dim() != 2 or int(mask.shape[0]) != int(rows.shape[0]):
        raise ValueError("denoise_rows: mask must be bool [n] for rows [n,4]")
    kept = rows[mask]
    if counts is None:
        return kept, None
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if np.any(c < 0) or int(c.sum()) != int(rows.shape[0]):
        raise ValueError("denoise_rows: counts sum to %d rows, there are %d" % (int(c.sum()), int(rows.shape[0])))
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(c)])).to(rows.device)
    run = torch.cat([torch.zeros((1,), dtype=torch.int64, device=rows.device), torch.cumsum(mask.to(torch.int64), 0)])
    return kept, (run[off[1:]] - run[off[:-1]]).cpu().numpy()
