"""A stream's own statistics next to the rows: `EventStats` counts, in one pass over the rows of device-resident runs, the events
per pixel, the same-pixel inter-event intervals and the events per time bin -- what the reference's ddd_plot_event_counts.py takes
from select_events_in_roi and histogram_events_in_time_bins (v2e_utils.py), and what shows leak periodicity, shot-noise rate,
refractory limits and hot pixels.  With the emulator's signal / noise labels every sum is kept for signal and noise separately;
`EventStatsResult.compare` puts an emulation beside a recording.

Rows.  Rows are device float32 [n,4] = (t, x = column, y = row, p), taken in row order.  A row is bad under exactly `DenoiseSweep`'s
rule (v2e_amd/csrc/rowkeys.h): t not finite, or x / y not an integer value inside [0,W) / [0,H).  It is counted in n_bad and touches
nothing.  A valid row is ON iff p > 0 (`EventPatches`' rule).

Labels.  `DenoiseSweep`'s: `n_signal=` with `counts=` (per frame of the run its first n_signal[f] of counts[f] rows are signal), or
`labels=` (bool [n], device or host, True = signal), or neither (all signal).  Label 1 is signal, 0 noise.

count.  int64 [2,2,H,W], indexed [label, pol, y, x], pol 0 = OFF, 1 = ON: every valid row, whatever `roi` and `time_bounds` are.

roi = ((x0, x1), (y0, y1)), inclusive (`ThresholdSweep`'s convention and checks; default: the whole sensor).  Everything below counts
the valid rows inside the ROI only.  The carried maps are stamped by every valid row.

Intervals.  The previous event of row i is the latest valid row j < i at the same pixel in this call, otherwise the carried `last_t`
(float32 [H,W], starts at -inf) / `last_p` (int8, +1 / -1, starts at 0): `EventPatches`' centre entry.  If there is none,
n_first[label, pol] += 1.  Otherwise d = float64(t_i) - float64(T_prev), kept when negative, tr = 2 * (previous ON) + (this ON) and
isi_hist[label, tr, searchsorted(isi_edges, d, 'right')] += 1, int64 [2,4,E+1].  d < 0 also counts in n_backwards[label].
min_isi[label, tr] is the smallest d >= 0 as float64, +inf where there is none.  isi_edges: 1 to 256 entries, finite, >= 0, strictly
ascending.

Time bins.  time_bounds is a strictly ascending finite float64 table of K + 1 entries, 1 <= K <= 2^20.
k = searchsorted(time_bounds, float64(t), 'right') - 1, and time_hist[label, pol, k] += 1 (int64 [2,2,K]) for 0 <= k < K; otherwise
the row counts in n_before (k < 0) or n_after.  With time_bounds=None there is no time histogram.

t_first / t_last.  The smallest and largest t of the valid rows (float32 values, ROI or not); None while there is none.

Cut independence.  Thread j of the kernel takes sorted key j of `DenoiseSweep`'s row index (pixel << 32 | row, torch.sort), so the
previous event is the key before it or the carried map; every sum is an integer atomic (v2e_amd/csrc/stats.hip).  The result
depends on the row order alone: a stream cut into several `add_run` calls, or a call cut into passes of `max_rows_per_pass` rows,
gives identical integers and identical final maps.  `add_run` fits the `on_events` callbacks of `run_stream` and
`SyntheticToEvents.run`, the chunks of `EventFileReader` and `generate_events_batch(return_device=True)`; it enqueues on the current
stream and never waits for the device.  `result()` is the one read-back.
"""
import math

import numpy as np
import torch

from . import _capi, _rowpasses
from ._capi import check, ptr, stream_ptr
from ._rowpasses import DEFAULT_ROWS_PER_PASS

MAX_EDGES = 256
MAX_TIME_BINS = 1 << 20
SUM_WORDS = 18   # stats.hip's sums[]: n_first [4], n_backwards [2], n_before, n_after, min_isi bits [8], keys of t_first, t_last
_INF_BITS = 0x7FF0000000000000
ISI_REPLICAS = 16             # copies of the interval histogram the kernel's workgroups spread their adds over (result() sums them)
MAX_TIME_CELLS = 1 << 16      # ... and as many copies of the time histogram, up to 64, as stay within this many cells


def _check_edges(edges):
    e = np.array(edges, dtype=np.float64).reshape(-1)
    if not 1 <= len(e) <= MAX_EDGES:
        raise ValueError("EventStats: 1 to %d isi_edges, got %d" % (MAX_EDGES, len(e)))
    if not np.all(np.isfinite(e)) or np.any(e < 0) or np.any(np.diff(e) <= 0):
        raise ValueError("EventStats: isi_edges must be finite, >= 0 and strictly ascending")
    return e


def _check_bounds(bounds):
    if bounds is None:
        return None
    b = np.array(bounds, dtype=np.float64).reshape(-1)
    if not 2 <= len(b) <= MAX_TIME_BINS + 1:
        raise ValueError("EventStats: time_bounds needs 2 to 2^20 + 1 entries, got %d" % len(b))
    if not np.all(np.isfinite(b)) or np.any(np.diff(b) <= 0):
        raise ValueError("EventStats: time_bounds must be finite and strictly ascending")
    return b


def _check_roi(name, roi, height, width):
    if roi is None:
        roi = ((0, width - 1), (0, height - 1))
    try:
        (x0, x1), (y0, y1) = roi
        x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
    except (TypeError, ValueError):
        raise ValueError("%s: roi must be ((x0, x1), (y0, y1)), got %r" % (name, roi)) from None
    if not (0 <= x0 <= x1 < width and 0 <= y0 <= y1 < height):
        raise ValueError("%s: roi %r is empty or outside the %dx%d sensor" % (name, roi, width, height))
    return (x0, x1), (y0, y1)


def _key_to_float(key):
    """The float32 whose stats.hip float_key is `key`."""
    bits = key & 0x7FFFFFFF if key & 0x80000000 else ~key & 0xFFFFFFFF
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def _pearson(a, b):
    """Pearson r of two equally long vectors in float64; NaN where a side is constant (or empty)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    if len(a) == 0:
        return math.nan
    da, db = a - a.mean(), b - b.mean()
    saa, sbb = float((da * da).sum()), float((db * db).sum())
    if saa == 0.0 or sbb == 0.0:
        return math.nan
    return float((da * db).sum() / math.sqrt(saa * sbb))


def _jsd(p, q):
    """Jensen-Shannon divergence in base 2 of two count vectors, each normalised to sum 1; NaN where one has no count."""
    p, q = np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(q, dtype=np.float64).reshape(-1)
    if p.sum() == 0 or q.sum() == 0:
        return math.nan
    p, q = p / p.sum(), q / q.sum()
    m = 0.5 * (p + q)

    def kl(a):
        nz = a > 0
        return float((a[nz] * np.log2(a[nz] / m[nz])).sum())
    return 0.5 * kl(p) + 0.5 * kl(q)


class EventStatsResult(object):
    """The sums of an `EventStats` on the host (numpy; the definitions: module docstring).

    height, width, roi, isi_edges float64 [E], time_bounds float64 [K+1] or None
    count int64 [2,2,H,W]      isi_hist int64 [2,4,E+1]    time_hist int64 [2,2,K] or None
    n_first int64 [2,2]        n_backwards int64 [2]       n_before, n_after, n, n_bad int
    min_isi float64 [2,4]      t_first, t_last float or None
    """

    def __init__(self, height, width, roi, isi_edges, time_bounds, count, isi_hist, time_hist, n_first, n_backwards, n_before,
                 n_after, min_isi, t_first, t_last, n_bad):
        self.height, self.width, self.roi = int(height), int(width), roi
        self.isi_edges = np.array(isi_edges, dtype=np.float64)
        self.time_bounds = None if time_bounds is None else np.array(time_bounds, dtype=np.float64)
        self.count = np.array(count, dtype=np.int64).reshape(2, 2, self.height, self.width)
        self.isi_hist = np.array(isi_hist, dtype=np.int64).reshape(2, 4, len(self.isi_edges) + 1)
        self.time_hist = None if self.time_bounds is None else np.array(time_hist, dtype=np.int64).reshape(2, 2, len(self.time_bounds) - 1)
        self.n_first = np.array(n_first, dtype=np.int64).reshape(2, 2)
        self.n_backwards = np.array(n_backwards, dtype=np.int64).reshape(2)
        self.n_before, self.n_after, self.n_bad = int(n_before), int(n_after), int(n_bad)
        self.min_isi = np.array(min_isi, dtype=np.float64).reshape(2, 4)
        self.t_first, self.t_last = t_first, t_last
        self.n = int(self.count.sum())

    @property
    def duration(self):
        """float64(t_last) - float64(t_first); None while there is no valid row."""
        return None if self.t_first is None else float(np.float64(self.t_last) - np.float64(self.t_first))

    def rate_hz(self, duration=None):
        """count / duration as float64 [2,2,H,W]; duration None: the stream's own.  ValueError unless the duration is > 0."""
        d = self.duration if duration is None else float(duration)
        if d is None or not d > 0 or not math.isfinite(d):
            raise ValueError("EventStatsResult.rate_hz: needs a finite duration > 0, got %r" % (d,))
        return self.count.astype(np.float64) / d

    def _labels(self, label):
        if label is None:
            return [0, 1]
        if label not in (0, 1, False, True):
            raise ValueError("EventStatsResult: label must be None, 0 (noise) or 1 (signal), got %r" % (label,))
        return [int(label)]

    def on_off_counts(self, roi=None, label=None):
        """(ON, OFF) events inside roi (None: the result's own ROI), of one label or, label None, of both: ints, from `count`."""
        (x0, x1), (y0, y1) = _check_roi("EventStatsResult.on_off_counts", self.roi if roi is None else roi, self.height, self.width)
        c = self.count[self._labels(label)][:, :, y0:y1 + 1, x0:x1 + 1]
        return int(c[:, 1].sum()), int(c[:, 0].sum())

    def time_series(self, pol, label=None):
        """float64 [K,2] of (bin centre, count), the layout v2e_utils.histogram_events_in_time_bins returns.  pol: 1 (or True) for
        ON, -1 or 0 for OFF, None for both."""
        if self.time_hist is None:
            raise ValueError("EventStatsResult.time_series: the statistics were taken without time_bounds")
        if pol not in (None, 1, 0, -1, True, False):
            raise ValueError("EventStatsResult.time_series: pol must be 1, -1 (or 0) or None, got %r" % (pol,))
        pols = [0, 1] if pol is None else [1 if pol > 0 else 0]
        h = self.time_hist[self._labels(label)][:, pols].sum(axis=(0, 1))
        return np.stack([(self.time_bounds[:-1] + self.time_bounds[1:]) / 2, h.astype(np.float64)], axis=1)

    def compare(self, other):
        """This stream beside another (an emulation beside a recording).  Both must share sensor, ROI, edges and bounds.  Returns
        {"time_corr": [OFF, ON], "map_corr": [OFF, ON], "isi_jsd"}: Pearson r of the time histograms (None without time_bounds) and of
        the per-pixel counts inside the ROI, labels summed, NaN where a side is constant; and the Jensen-Shannon divergence in base 2
        of the normalised interval histograms, labels and transitions summed (NaN where a side has no interval)."""
        if not isinstance(other, EventStatsResult):
            raise TypeError("EventStatsResult.compare takes another EventStatsResult")
        same_bounds = (self.time_bounds is None) == (other.time_bounds is None) and \
            (self.time_bounds is None or np.array_equal(self.time_bounds, other.time_bounds))
        if (self.height, self.width, self.roi) != (other.height, other.width, other.roi) or not same_bounds or \
                not np.array_equal(self.isi_edges, other.isi_edges):
            raise ValueError("EventStatsResult.compare: the two results must share sensor, roi, isi_edges and time_bounds")
        (x0, x1), (y0, y1) = self.roi
        maps = [r.count.sum(axis=0)[:, y0:y1 + 1, x0:x1 + 1] for r in (self, other)]
        out = {"map_corr": [_pearson(maps[0][pol], maps[1][pol]) for pol in (0, 1)],
               "time_corr": None,
               "isi_jsd": _jsd(self.isi_hist.sum(axis=(0, 1)), other.isi_hist.sum(axis=(0, 1)))}
        if self.time_hist is not None:
            out["time_corr"] = [_pearson(self.time_hist.sum(axis=0)[pol], other.time_hist.sum(axis=0)[pol]) for pol in (0, 1)]
        return out


class EventStats(object):
    """Counts, intervals and time-bin counts of a stream's rows, run by run, with the maps and every sum carried on the device
    (module docstring)."""

    def __init__(self, height, width, isi_edges=None, time_bounds=None, roi=None, max_rows_per_pass=DEFAULT_ROWS_PER_PASS,
                 device="cuda"):
        self.height, self.width = _rowpasses.check_sensor("EventStats", height, width)
        self.isi_edges = _check_edges(np.geomspace(1e-5, 10.0, 61) if isi_edges is None else isi_edges)
        self.time_bounds = _check_bounds(time_bounds)
        self.roi = _check_roi("EventStats", roi, self.height, self.width)
        self.max_rows_per_pass = _rowpasses.check_rows_per_pass("EventStats", max_rows_per_pass)
        self.device = torch.device(device)
        self.passes = 0           # row blocks processed so far
        self._state = None        # the device buffers, allocated by the first call that needs them

    @staticmethod
    def time_bins(start, stop, bin_s):
        """np.arange(start, stop, bin_s): the ticks of v2e_utils.histogram_events_in_time_bins (bin_s = time_bin_ms * 0.001), as a
        time_bounds table -- its bins are [tick[i], tick[i+1])."""
        ticks = np.arange(start, stop, bin_s, dtype=np.float64)
        if len(ticks) < 2:
            raise ValueError("EventStats.time_bins: need start + bin_s < stop, got %r, %r, %r" % (start, stop, bin_s))
        return ticks

    # ------------------------------------------------------------------------------------------------------------ device state
    def _time_replicas(self):
        K = 0 if self.time_bounds is None else len(self.time_bounds) - 1
        return max(1, min(64, MAX_TIME_CELLS // max(4 * K, 1)))

    def _sizes(self):
        E, K = len(self.isi_edges), 0 if self.time_bounds is None else len(self.time_bounds) - 1
        # sums and n_bad, the copies of isi_hist, the copies of time_hist, count
        return SUM_WORDS + 1, ISI_REPLICAS * 8 * (E + 1), self._time_replicas() * 4 * K, 4 * self.height * self.width

    def _dev(self):
        if self._state is None:
            _capi.require_gpu("EventStats")
            dev, H, W = self.device, self.height, self.width
            init = np.zeros(SUM_WORDS + 1, dtype=np.int64)
            init[8:16] = _INF_BITS
            init[16] = 0xFFFFFFFF
            acc = torch.zeros((sum(self._sizes()),), dtype=torch.int64, device=dev)   # one buffer: one read-back
            o = np.cumsum((0,) + self._sizes())
            self._state = {
                "last_t": torch.full((H, W), -math.inf, dtype=torch.float32, device=dev),
                "last_p": torch.zeros((H, W), dtype=torch.int8, device=dev),
                "seg": _rowpasses.new_seg(H, W, dev),
                "acc": acc, "sums": acc[o[0]:o[1]], "isi_hist": acc[o[1]:o[2]], "time_hist": acc[o[2]:o[3]], "count": acc[o[3]:o[4]],
                "init": torch.from_numpy(init).to(dev),
                "edges": torch.from_numpy(self.isi_edges).to(dev),
                "bounds": None if self.time_bounds is None else torch.from_numpy(self.time_bounds).to(dev),
            }
            self._state["sums"].copy_(self._state["init"])
        return self._state

    def reset(self):
        """The next stream: the maps back to -inf / 0, every sum to zero (enqueued on the current stream)."""
        if self._state is not None:
            st = self._state
            st["last_t"].fill_(-math.inf)
            st["last_p"].zero_()
            st["acc"].zero_()
            st["sums"].copy_(st["init"])

    @property
    def last_t(self):
        """The carried time map, float32 [H,W] on the device (-inf: no row yet): a copy."""
        return self._dev()["last_t"].clone()

    @property
    def last_p(self):
        """The carried polarity map, int8 [H,W] on the device (+1 / -1; 0: no row yet): a copy."""
        return self._dev()["last_p"].clone()

    # ------------------------------------------------------------------------------------------------------------ the run
    def add_run(self, rows, counts=None, frame0=None, n_signal=None, labels=None):
        """Add one run's rows (device float32 [n,4]; None or empty: nothing happens) to every sum and move the maps past them.

        The rows' labels: `labels` (bool [n], device or host, True = signal), or `n_signal` with `counts`, or neither (all signal);
        frame0 is not needed and ignored: the signature is on_events'.
        Returns {"n": valid rows, "n_bad": bad rows}: 0-dim int64 device tensors (reading one waits for the device; the call does
        not)."""
        # every ValueError before the library or the device is touched
        n, labels, bounds = _rowpasses.check_run("EventStats", rows, counts, n_signal, labels)
        st = self._dev()
        dev = self.device
        if n == 0:
            return _rowpasses.no_rows(dev)
        rows = rows.to(dev).contiguous()
        lib = _capi.lib()
        stream = stream_ptr(dev)
        H, W = self.height, self.width
        (x0, x1), (y0, y1) = self.roi
        lab, lb = _rowpasses.labels_to_device(labels, bounds, dev)
        K = 0 if st["bounds"] is None else int(st["bounds"].shape[0]) - 1
        run = _rowpasses.RowPasses(self, rows, st["seg"])
        for r0, m, ev, skeys in run:
            check(lib.v2e_stats_rows(ptr(ev), m, H, W, ptr(skeys), ptr(st["seg"]), ptr(st["last_t"]), ptr(st["last_p"]), x0, x1, y0, y1,
                                     ptr(st["edges"]), len(self.isi_edges), ptr(st["bounds"]), K,
                                     *_rowpasses.label_args(lab, lb, r0), ptr(st["count"]), ptr(st["isi_hist"]), ISI_REPLICAS,
                                     ptr(st["time_hist"]) if K else None, self._time_replicas(), ptr(st["sums"]), stream),
                  "v2e_stats_rows")
            check(lib.v2e_stats_map_update(ptr(ev), ptr(skeys), ptr(st["seg"]), H, W, ptr(st["last_t"]), ptr(st["last_p"]), stream),
                  "v2e_stats_map_update")
        st["sums"][SUM_WORDS] += run.n_bad
        return {"n": run.n, "n_bad": run.n_bad}

    def result(self):
        """The sums so far as an EventStatsResult: the one read-back (it waits for the runs enqueued so far)."""
        flat = self._dev()["acc"].cpu().numpy()
        o = np.cumsum((0,) + self._sizes())
        sums = flat[o[0]:o[1]]
        first_key, last_key = int(sums[16]), int(sums[17])
        some = last_key != 0
        isi_hist = flat[o[1]:o[2]].reshape(ISI_REPLICAS, -1).sum(axis=0)
        time_hist = flat[o[2]:o[3]].reshape(self._time_replicas(), -1).sum(axis=0)
        return EventStatsResult(self.height, self.width, self.roi, self.isi_edges, self.time_bounds, flat[o[3]:o[4]], isi_hist, time_hist,
                                sums[0:4], sums[4:6], sums[6], sums[7], sums[8:16].copy().view(np.float64),
                                _key_to_float(first_key) if some else None, _key_to_float(last_key) if some else None, sums[SUM_WORDS])
