"""Per-event time-surface patches next to the rows: `EventPatches` emits, for every row of device-resident runs, the
(2r+1) x (2r+1) patch of ages and polarities around it, as the maps were just before the row -- the input of a learned event
denoiser (the MLP filter, MLPF, of the DND21 work takes mode "linear"; HOTS- and HATS-style features are the same patches with
another decay).  `frame_labels` gives the training targets that go with them, `score_roc` puts a learned filter's scores on the ROC
axes `DenoiseSweep` draws.

Rows and validity.  Rows are device float32 [n,4] = (t, x = column, y = row, p), taken in row order.  A row is bad under exactly
`DenoiseSweep`'s rule: t not finite, or x / y not an integer value inside [0,W) / [0,H).  p is not examined for validity.  A bad row
reads and writes no map and gets valid = False.  Its features are the "none" values below.

Carried maps.  `last_t` is float32 [H,W] and starts at -inf.  `last_p` is int8 [H,W] and starts at 0.  Both are carried on the
device from call to call.

Per-row patch.  For a valid row i at (x, y) and every offset (dy, dx) in [-r, r]^2: the patch index is [dy + r, dx + r]; r is 1, 2
or 3; the centre is included.  Let q = (x + dx, y + dy).  If q is outside the sensor, the entry is none.  Otherwise T_q and P_q are
taken from the latest valid row j < i at q in this call: T_q is its t, P_q is the sign of its p (+1 if p > 0, else -1).  If no such
row exists in this call, the carried maps supply T_q and P_q.  A carried T_q of -inf means none.  age = float64(t_i) - float64(T_q).
A T_q later than t_i gives a negative age, which is kept.  The centre entry is the previous event at the same pixel.  The row is
never in its own patch.

After reading, the row stamps last_t[y,x] = t_i and last_p[y,x] = sign(p_i).

Output.  `features` is float32 [n, 2, P, P] with P = 2r+1.  mode="age": channel 0 is float32(age), rounded to nearest even; +inf
where none.  Channel 1 is P_q as +-1.0; 0 where none.  mode="linear" (MLPF's input; tau > 0 finite), channel 0: 0 where none or
age >= tau; 1 where age <= 0; otherwise float32(1 - age / tau), with the division and the subtraction each rounded in float64.
Channel 1: P_q where channel 0's entry is not of the first kind, that is, not none and age < tau; otherwise 0.

Invariance.  The result depends on the row order alone.  A clip cut into several `add_run` calls gives identical features and
identical final maps.  A call cut into blocks of `max_rows_per_pass` rows gives identical features and identical final maps.

The lookup is `DenoiseSweep`'s: each row gets the key pixel << 32 | row, the keys are sorted (torch.sort), and "the latest earlier
row at q" is a binary search in q's stretch of the sorted keys (v2e_amd/csrc/patches.hip).  Scratch per row of a pass is the sort's,
48 bytes at the peak; the features themselves take 2 * P * P * 4 bytes per row (392 at r = 3).
"""
import math

import torch

from . import _capi, _rowpasses
from ._capi import check, ptr, stream_ptr
from ._rowpasses import DEFAULT_ROWS_PER_PASS, label_bounds

MODES = {"age": 0, "linear": 1}
MAX_RADIUS = 3


class EventPatches(object):
    """The patches of a clip's rows, run by run, with the maps carried on the device (module docstring)."""

    def __init__(self, height, width, radius=3, mode="linear", tau=0.1, device="cuda", max_rows_per_pass=DEFAULT_ROWS_PER_PASS,
                 max_output_bytes=8 << 30):
        self.height, self.width = _rowpasses.check_sensor("EventPatches", height, width)
        if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
            raise ValueError("EventPatches: radius must be 1, 2 or %d, got %r" % (MAX_RADIUS, radius))
        self.radius = int(radius)
        self.size = 2 * self.radius + 1
        if mode not in MODES:
            raise ValueError("EventPatches: mode must be one of %s, got %r" % (sorted(MODES), mode))
        self.mode = mode
        try:
            self.tau = float(tau)
        except (TypeError, ValueError):
            raise ValueError("EventPatches: tau must be a number, got %r" % (tau,)) from None
        if mode == "linear" and not (math.isfinite(self.tau) and self.tau > 0):
            raise ValueError("EventPatches: mode 'linear' needs a finite tau > 0, got %r" % (tau,))
        self.max_rows_per_pass = _rowpasses.check_rows_per_pass("EventPatches", max_rows_per_pass)
        self.max_output_bytes = int(max_output_bytes)
        if self.max_output_bytes < 0:
            raise ValueError("EventPatches: max_output_bytes must be >= 0")
        self.device = torch.device(device)
        self.passes = 0        # row blocks processed so far
        self._state = None     # the device buffers, allocated by the first call that needs them

    # ------------------------------------------------------------------------------------------------------------ device state
    def _dev(self):
        if self._state is None:
            _capi.require_gpu("EventPatches")
            dev, H, W = self.device, self.height, self.width
            self._state = {
                "last_t": torch.full((H, W), -math.inf, dtype=torch.float32, device=dev),
                "last_p": torch.zeros((H, W), dtype=torch.int8, device=dev),
                "seg": _rowpasses.new_seg(H, W, dev),
            }
        return self._state

    def reset(self):
        """The maps back to -inf and 0 (enqueued on the current stream)."""
        if self._state is not None:
            self._state["last_t"].fill_(-math.inf)
            self._state["last_p"].zero_()

    @property
    def last_t(self):
        """The carried time map, float32 [H,W] on the device (-inf: no row yet): a copy."""
        return self._dev()["last_t"].clone()

    @property
    def last_p(self):
        """The carried polarity map, int8 [H,W] on the device (+1 / -1; 0: no row yet): a copy."""
        return self._dev()["last_p"].clone()

    # ------------------------------------------------------------------------------------------------------------ the run
    def add_run(self, rows, counts=None, frame0=0, out=None):
        """The patches of one run's rows (device float32 [n,4]; None or empty: empty results), and the maps moved past them.

        counts and frame0 are not needed and ignored: the signature is on_events'.  out: a float32 [>= n, 2, P, P] contiguous
        device tensor whose first n entries are written (every element of them), instead of a new tensor.
        Returns {"features": float32 [n,2,P,P], "valid": bool [n], "n": valid rows, "n_bad": bad rows}: device tensors, n and n_bad
        0-dim int64 (reading one waits for the device; the call does not)."""
        # every ValueError before the library or the device is touched
        P = self.size
        n = _rowpasses.check_run("EventPatches", rows)[0]
        if out is not None:
            if not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_cuda or out.dim() != 4 or \
                    tuple(out.shape[1:]) != (2, P, P) or int(out.shape[0]) < n or not out.is_contiguous():
                raise ValueError("EventPatches.add_run: out must be a contiguous device float32 [>= %d, 2, %d, %d] tensor" % (n, P, P))
            if rows is not None and out.device != rows.device:
                raise ValueError("EventPatches.add_run: out is on %s, the rows on %s" % (out.device, rows.device))
        elif n * 2 * P * P * 4 > self.max_output_bytes:
            raise ValueError("EventPatches.add_run: the features of %d rows take %d bytes, more than max_output_bytes = %d: split the "
                             "call or pass out=" % (n, n * 2 * P * P * 4, self.max_output_bytes))
        st = self._dev()
        dev = self.device
        if n == 0:
            feats = out[:0] if out is not None else torch.empty((0, 2, P, P), dtype=torch.float32, device=dev)
            return dict(_rowpasses.no_rows(dev), features=feats, valid=torch.zeros((0,), dtype=torch.bool, device=dev))
        rows = rows.to(dev).contiguous()
        lib = _capi.lib()
        stream = stream_ptr(dev)
        H, W = self.height, self.width
        feats = out[:n] if out is not None else torch.empty((n, 2, P, P), dtype=torch.float32, device=dev)
        valid = torch.empty((n,), dtype=torch.uint8, device=dev)
        run = _rowpasses.RowPasses(self, rows, st["seg"])
        for r0, m, ev, skeys in run:
            check(lib.v2e_patches_features(ptr(ev), m, H, W, ptr(skeys), ptr(st["seg"]), ptr(st["last_t"]), ptr(st["last_p"]),
                                           self.radius, MODES[self.mode], self.tau, ptr(feats[r0:r0 + m]), ptr(valid[r0:r0 + m]), stream),
                  "v2e_patches_features")
            check(lib.v2e_patches_map_update(ptr(ev), ptr(skeys), ptr(st["seg"]), H, W, ptr(st["last_t"]), ptr(st["last_p"]), stream),
                  "v2e_patches_map_update")
        return {"features": feats, "valid": valid.view(torch.bool), "n": run.n, "n_bad": run.n_bad}


def frame_labels(counts, n_signal, device=None):
    """bool [sum(counts)]: frame f's first n_signal[f] of its counts[f] rows are True (signal) -- a run's counts and
    EventEmulator.last_n_signal as one label per row, the training targets that go with the patches.  Torch ops on `device`."""
    bounds, total = label_bounds(counts, n_signal)
    device = torch.device("cpu" if device is None else device)
    start = torch.from_numpy(bounds[0::2].copy()).to(device)
    n_sig = torch.from_numpy((bounds[1::2] - bounds[0::2]).copy()).to(device)
    count = torch.diff(start, append=torch.tensor([total], dtype=torch.int64, device=start.device))
    frame = torch.repeat_interleave(torch.arange(len(bounds) // 2, device=start.device), count, output_size=total)
    return torch.arange(total, device=start.device) - start[frame] < n_sig[frame]


def score_roc(scores, labels, thresholds, valid=None):
    """A learned filter on DenoiseResult's ROC axes: scores float [n] (a row passes threshold b iff score >= thresholds[b], compared in
    float64; a NaN score passes none), labels bool [n] (True = signal), thresholds ascending and finite [T], valid bool [n] or None
    (rows to leave out altogether).  Returns {"passed": int64 [2,T] (noise row first, signal second), "tpr", "fpr": float64 [T]
    (passed / the valid rows of that label; NaN where there are none), "n_signal", "n_noise": 0-dim int64}, on the scores' device.
    Integer counting (torch.bucketize and scatter_add_, in roc_counts): exact."""
    if not (torch.is_tensor(scores) and torch.is_tensor(labels)):
        raise TypeError("score_roc takes tensors")
    if scores.dim() != 1 or not scores.dtype.is_floating_point:
        raise ValueError("score_roc: scores must be a float [n] tensor")
    n, dev = int(scores.shape[0]), scores.device
    if labels.dtype != torch.bool or tuple(labels.shape) != (n,):
        raise ValueError("score_roc: labels must be bool [%d]" % n)
    if valid is not None and (not torch.is_tensor(valid) or valid.dtype != torch.bool or tuple(valid.shape) != (n,)):
        raise ValueError("score_roc: valid must be bool [%d]" % n)
    thr = torch.as_tensor(thresholds, dtype=torch.float64).reshape(-1)
    T = int(thr.shape[0])
    if T < 1 or not bool(torch.isfinite(thr).all()) or bool((torch.diff(thr) <= 0).any()):
        raise ValueError("score_roc: thresholds must be finite and strictly ascending, at least one")
    passed, total = roc_counts(scores, labels.to(dev), thr.to(dev), None if valid is None else valid.to(dev))
    rate = passed.to(torch.float64) / total.to(torch.float64)[:, None]       # (0 / 0: NaN)
    return {"passed": passed, "tpr": rate[1], "fpr": rate[0], "n_signal": total[1], "n_noise": total[0]}


def roc_counts(scores, labels, thr, valid=None):
    """score_roc's counting on tensors of one device, arguments already checked (thr: float64 [T]): (passed int64 [2,T], the valid
    rows of each label int64 [2]).  Integer scatter-adds into a histogram of fixed size: exact, and nothing waits for the device."""
    T = int(thr.shape[0])
    s = scores.to(torch.float64)
    b = torch.bucketize(s, thr, right=True)                    # the number of thresholds <= score: the row passes thresholds[:b]
    b = torch.where(torch.isnan(s), torch.zeros_like(b), b)
    cell = b + (T + 1) * labels.to(torch.int64)
    if valid is not None:
        cell = torch.where(valid, cell, torch.full_like(cell, 2 * (T + 1)))  # (a cell of their own, dropped below)
    hist = torch.zeros((2 * (T + 1) + 1,), dtype=torch.int64, device=s.device)
    hist.scatter_add_(0, cell, torch.ones_like(cell))
    hist = hist[:-1].reshape(2, T + 1)
    passed = torch.flip(torch.cumsum(torch.flip(hist[:, 1:], [1]), 1), [1])   # passed[:, b] = rows whose count is above b
    return passed, hist.sum(1)
