"""A learned denoiser next to the rows: `MLPFilter` scores every row of device-resident runs with a one-hidden-layer MLP on its
time-surface patch -- the MLP filter, MLPF, of the DND21 work -- in one fused pass: patches gathered, network evaluated and score
written by one kernel (v2e_amd/csrc/mlpf.hip).  No feature ever exists in device memory, the scores are defined to the bit, and
`add_run(rows, counts, frame0)` has the shape of the other row consumers (`DenoiseSweep`, `EventPatches`, `EventStats`).

Rows, validity, carried maps, per-row patch.  Exactly `EventPatches`' with mode="linear" and the same tau (finite, > 0; module
docstring of v2e_amd/patches.py), including the stamping of last_t / last_p by every valid row, whether or not the filter keeps it.
The input vector of row i is its `EventPatches` features flattened as torch flattens [2, P, P]: x[c*P*P + (dy+r)*P + (dx+r)],
K = 2*P*P entries (18, 50 or 98 for r = 1, 2, 3).  In linear mode they are all finite.

Network.  One hidden layer with ReLU and one output.  w1 is float32 [hidden, K], b1 float32 [hidden], w2 float32 [1, hidden] or
[hidden], b2 float32 [1] or a scalar: nn.Linear's layouts.  1 <= hidden <= 64; all values finite.  Tensors and arrays are accepted;
anything not float32 is refused, nothing is rounded silently (a Python number for b2 must be a float32 value).

Arithmetic, chosen so that a numpy loop reproduces it bit for bit (tests/mlp_filter_ref.py):
    a_j = float64(b1[j]);  for k = 0 .. K-1 ascending:  a_j = a_j + float64(w1[j,k]) * float64(x[k])
    h_j = float32(a_j), rounded to nearest even;  h_j = h_j if h_j > 0 else 0      (a NaN becomes 0)
    s = float64(b2);  for j ascending:  s = s + float64(w2[j]) * float64(h_j);  score = float32(s)
The product of two float32 values is exact in float64, so each step is one float64 rounding, the same with or without an fma.
There is no sigmoid and no transcendental on the device: the score is the logit, and a probability threshold p is the logit
threshold log(p / (1 - p)), `MLPFilter.logit(p)`.  A bad row gets the float32 quiet NaN with bits 0x7fc00000, valid = False and
mask False.

Invariance.  Results depend on the row order alone.  Cutting a clip into calls, or a call into passes of `max_rows_per_pass`,
changes no score and no map.

Scratch per row beside the sort's 48 bytes of a pass: 4 bytes of score, 1 of valid, 1 of mask -- 6 bytes per row of the call (and 1
more while ROC labels are on the device), against the 2 * P * P * 4 = 392 bytes of features at r = 3 that `EventPatches` writes.
"""
import math

import numpy as np
import torch

from . import _capi, _rowpasses
from ._capi import check, ptr, stream_ptr
from ._rowpasses import DEFAULT_ROWS_PER_PASS
from .patches import MAX_RADIUS, frame_labels, roc_counts

MAX_HIDDEN = 64
ROWS_PER_WORKGROUP = 64    # MLP_TILE_ROWS of v2e_amd/csrc/mlpf.hip: the rows of one tile
MAX_WORKGROUPS = 2048      # MLP_MAX_BLOCKS: above MAX_WORKGROUPS * ROWS_PER_WORKGROUP valid rows a pass takes a second grid-stride trip


def _f32_array(name, a):
    """`a` (tensor, array or numpy scalar) as a float32 numpy array; ValueError for every other type: nothing is rounded"""
    if torch.is_tensor(a):
        if a.dtype != torch.float32:
            raise ValueError("MLPFilter: %s must be float32, got %s" % (name, a.dtype))
        a = a.detach().cpu().numpy()
    elif isinstance(a, (np.ndarray, np.generic)):
        if a.dtype != np.float32:
            raise ValueError("MLPFilter: %s must be float32, got %s" % (name, a.dtype))
        a = np.asarray(a)
    elif isinstance(a, (int, float)) and not isinstance(a, bool):
        with np.errstate(over="ignore"):
            f = np.float32(a)
        if not (float(f) == float(a) or a != a):
            raise ValueError("MLPFilter: %s = %r is not a float32 value" % (name, a))
        a = np.asarray(f)
    else:
        raise ValueError("MLPFilter: %s must be a float32 tensor or array, got %s" % (name, type(a).__name__))
    if not np.all(np.isfinite(a)):
        raise ValueError("MLPFilter: %s must be finite" % name)
    return np.ascontiguousarray(a)


class MLPFilter(object):
    """The scores of a clip's rows under a patch MLP, run by run, with the maps carried on the device (module docstring)."""

    def __init__(self, height, width, w1, b1, w2, b2, radius=3, tau=0.1, thresholds=None, device="cuda",
                 max_rows_per_pass=DEFAULT_ROWS_PER_PASS):
        # every ValueError before the library or the device is touched
        self.height, self.width = _rowpasses.check_sensor("MLPFilter", height, width)
        if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
            raise ValueError("MLPFilter: radius must be 1, 2 or %d, got %r" % (MAX_RADIUS, radius))
        self.radius = int(radius)
        self.size = 2 * self.radius + 1
        self.n_inputs = K = 2 * self.size * self.size
        try:
            self.tau = float(tau)
        except (TypeError, ValueError):
            raise ValueError("MLPFilter: tau must be a number, got %r" % (tau,)) from None
        if not (math.isfinite(self.tau) and self.tau > 0):
            raise ValueError("MLPFilter: needs a finite tau > 0, got %r" % (tau,))
        w1, b1, w2, b2 = _f32_array("w1", w1), _f32_array("b1", b1), _f32_array("w2", w2), _f32_array("b2", b2)
        if w1.ndim != 2 or w1.shape[1] != K:
            raise ValueError("MLPFilter: w1 must be [hidden, K] with K = 2 * %d * %d = %d inputs at radius %d, got %r"
                             % (self.size, self.size, K, self.radius, tuple(w1.shape)))
        hidden = int(w1.shape[0])
        if not 1 <= hidden <= MAX_HIDDEN:
            raise ValueError("MLPFilter: hidden must be in 1 .. %d, got %d" % (MAX_HIDDEN, hidden))
        if b1.shape != (hidden,):
            raise ValueError("MLPFilter: b1 must be [%d], got %r" % (hidden, tuple(b1.shape)))
        if w2.shape not in ((hidden,), (1, hidden)):
            raise ValueError("MLPFilter: w2 must be [1, %d] or [%d], got %r" % (hidden, hidden, tuple(w2.shape)))
        if b2.shape not in ((), (1,)):
            raise ValueError("MLPFilter: b2 must be [1] or a scalar, got %r" % (tuple(b2.shape),))
        self.hidden = hidden
        self.w1, self.b1, self.w2, self.b2 = w1.copy(), b1.copy(), w2.reshape(hidden).copy(), b2.reshape(1).copy()
        self.thresholds = None
        if thresholds is not None:
            t = np.array(thresholds, dtype=np.float64).reshape(-1)
            if len(t) < 1 or not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
                raise ValueError("MLPFilter: thresholds must be finite and strictly ascending, at least one")
            self.thresholds = t
        self.max_rows_per_pass = _rowpasses.check_rows_per_pass("MLPFilter", max_rows_per_pass)
        self.device = torch.device(device)
        self.passes = 0        # row blocks processed so far
        self._state = None     # the device buffers, allocated by the first call that needs them

    @classmethod
    def from_module(cls, height, width, module, **kw):
        """From nn.Sequential(nn.Linear(K, hidden), nn.ReLU(), nn.Linear(hidden, 1)); a trailing nn.Sigmoid is allowed and ignored
        (the score is the logit).  Any other structure: ValueError."""
        nn = torch.nn
        layers = list(module.children()) if isinstance(module, nn.Sequential) else None
        if layers is not None and len(layers) == 4 and isinstance(layers[3], nn.Sigmoid):
            layers = layers[:3]
        if layers is None or len(layers) != 3 or not (isinstance(layers[0], nn.Linear) and isinstance(layers[1], nn.ReLU)
                                                      and isinstance(layers[2], nn.Linear)):
            raise ValueError("MLPFilter.from_module takes nn.Sequential(nn.Linear(K, hidden), nn.ReLU(), nn.Linear(hidden, 1)) "
                             "with an optional trailing nn.Sigmoid")
        if layers[0].bias is None or layers[2].bias is None or layers[2].out_features != 1:
            raise ValueError("MLPFilter.from_module: both nn.Linear layers need a bias, and the second one a single output")
        return cls(height, width, layers[0].weight, layers[0].bias, layers[2].weight, layers[2].bias, **kw)

    @staticmethod
    def logit(p):
        """The score threshold of the probability threshold p, 0 < p < 1: log(p / (1 - p))."""
        p = float(p)
        if not 0.0 < p < 1.0:
            raise ValueError("MLPFilter.logit: p must be in (0, 1), got %r" % (p,))
        return math.log(p / (1.0 - p))

    # ------------------------------------------------------------------------------------------------------------ device state
    def _dev(self):
        if self._state is None:
            _capi.require_gpu("MLPFilter")
            dev, H, W = self.device, self.height, self.width
            self._state = {
                "last_t": torch.full((H, W), -math.inf, dtype=torch.float32, device=dev),
                "last_p": torch.zeros((H, W), dtype=torch.int8, device=dev),
                "seg": _rowpasses.new_seg(H, W, dev),
                "w1": torch.from_numpy(self.w1).to(dev), "b1": torch.from_numpy(self.b1).to(dev),
                "w2": torch.from_numpy(self.w2).to(dev), "b2": torch.from_numpy(self.b2).to(dev),
            }
            if self.thresholds is not None:
                self._state["thr"] = torch.from_numpy(self.thresholds).to(dev)
                self._state["passed"] = torch.zeros((2, len(self.thresholds)), dtype=torch.int64, device=dev)
                self._state["total"] = torch.zeros((2,), dtype=torch.int64, device=dev)
        return self._state

    def reset(self):
        """The maps back to -inf and 0, the ROC counts to zero (enqueued on the current stream)."""
        if self._state is not None:
            self._state["last_t"].fill_(-math.inf)
            self._state["last_p"].zero_()
            if self.thresholds is not None:
                self._state["passed"].zero_()
                self._state["total"].zero_()

    @property
    def last_t(self):
        """The carried time map, float32 [H,W] on the device (-inf: no row yet): a copy."""
        return self._dev()["last_t"].clone()

    @property
    def last_p(self):
        """The carried polarity map, int8 [H,W] on the device (+1 / -1; 0: no row yet): a copy."""
        return self._dev()["last_p"].clone()

    # ------------------------------------------------------------------------------------------------------------ the run
    def add_run(self, rows, counts=None, frame0=0, n_signal=None, labels=None, keep=None, out=None):
        """The scores of one run's rows (device float32 [n,4]; None or empty: empty results), and the maps moved past them.

        labels (bool [n], True = signal) or n_signal with counts (`DenoiseSweep.add_run`'s rule) are needed only when `thresholds`
        was given: the call then adds its rows to the ROC counts `result()` reads; with thresholds and neither, every row counts as
        signal.  frame0 is not needed and ignored: the signature is on_events'.  keep: a float threshold; mask[i] = valid[i] and
        float64(score[i]) >= float64(keep).  out: a contiguous device float32 [>= n] tensor that takes the scores; only its first n
        entries are written.
        Returns {"scores": float32 [n], "valid": bool [n], "mask": bool [n] or None, "n": valid rows, "n_bad": bad rows}: device
        tensors, n and n_bad 0-dim int64 (reading one waits for the device; the call does not)."""
        # every ValueError before the library or the device is touched
        if keep is not None:
            try:
                keep = float(keep)
            except (TypeError, ValueError):
                raise ValueError("MLPFilter.add_run: keep must be a float threshold, got %r" % (keep,)) from None
            if math.isnan(keep):
                raise ValueError("MLPFilter.add_run: keep must not be NaN")
        n, labels, _ = _rowpasses.check_run("MLPFilter", rows, counts, n_signal, labels)
        if out is not None:
            if not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_cuda or out.dim() != 1 or int(out.shape[0]) < n or \
                    not out.is_contiguous():
                raise ValueError("MLPFilter.add_run: out must be a contiguous device float32 [>= %d] tensor" % n)
            if rows is not None and out.device != rows.device:
                raise ValueError("MLPFilter.add_run: out is on %s, the rows on %s" % (out.device, rows.device))
        st = self._dev()
        dev = self.device
        if n == 0:
            return dict(_rowpasses.no_rows(dev, mask=True, keep=keep), valid=torch.zeros((0,), dtype=torch.bool, device=dev),
                        scores=out[:0] if out is not None else torch.empty((0,), dtype=torch.float32, device=dev))
        rows = rows.to(dev).contiguous()
        lib = _capi.lib()
        stream = stream_ptr(dev)
        H, W = self.height, self.width
        scores = out[:n] if out is not None else torch.empty((n,), dtype=torch.float32, device=dev)
        valid = torch.empty((n,), dtype=torch.uint8, device=dev)
        mask = _rowpasses.new_mask(keep, n, dev)
        run = _rowpasses.RowPasses(self, rows, st["seg"])
        for r0, m, ev, skeys in run:
            check(lib.v2e_patches_mlp_scores(ptr(ev), m, H, W, ptr(skeys), ptr(st["seg"]), ptr(st["last_t"]), ptr(st["last_p"]),
                                             self.radius, self.tau, ptr(st["w1"]), ptr(st["b1"]), self.hidden, ptr(st["w2"]),
                                             ptr(st["b2"]), ptr(scores[r0:r0 + m]), ptr(valid[r0:r0 + m]), 0.0 if keep is None else keep,
                                             None if mask is None else ptr(mask[r0:r0 + m]), stream), "v2e_patches_mlp_scores")
            check(lib.v2e_patches_map_update(ptr(ev), ptr(skeys), ptr(st["seg"]), H, W, ptr(st["last_t"]), ptr(st["last_p"]), stream),
                  "v2e_patches_map_update")
        valid = valid.view(torch.bool)
        if self.thresholds is not None:
            if labels is not None:
                lab = labels.to(dev, non_blocking=True)
            elif n_signal is not None:
                lab = frame_labels(counts, n_signal).pin_memory().to(dev, non_blocking=True)
            else:
                lab = torch.ones((n,), dtype=torch.bool, device=dev)
            passed, total = roc_counts(scores, lab, st["thr"], valid)
            st["passed"] += passed
            st["total"] += total
        return {"scores": scores, "valid": valid, "mask": None if mask is None else mask.view(torch.bool), "n": run.n, "n_bad": run.n_bad}

    def result(self):
        """The ROC counts so far, `score_roc`'s meaning, as numpy: {"passed": int64 [2,T] (noise row first, signal second), "tpr",
        "fpr": float64 [T] (NaN where a label has no valid row), "n_signal", "n_noise"}.  One small read-back (it waits for the runs
        enqueued so far)."""
        if self.thresholds is None:
            raise ValueError("MLPFilter.result: the filter was made without thresholds")
        st = self._dev()
        T = len(self.thresholds)
        flat = torch.cat([st["passed"].reshape(-1), st["total"]]).cpu().numpy()
        passed, total = flat[:2 * T].reshape(2, T).copy(), flat[2 * T:]
        with np.errstate(invalid="ignore", divide="ignore"):
            rate = passed.astype(np.float64) / total.astype(np.float64)[:, None]
        return {"passed": passed, "tpr": rate[1], "fpr": rate[0], "n_signal": int(total[1]), "n_noise": int(total[0])}
