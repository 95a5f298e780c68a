"""Dense event tensors next to the model: `EventTensorizer` turns the rows of device-resident runs into per-polarity count
images, voxel grids with bilinear time weights and time surfaces, window by window, without a trip through the host.

Rows are what every run hands out: device float32 [N,4] = (t, x = column, y = row, p = +-1).  The clip is cut into windows
[B_k, B_k+1), float64 with the float32 t widened: uniform, B_k = t_start + k * window_s (one product, one sum), or an explicit
ascending table `bounds` (K + 1 entries, K windows).  A row belongs to window searchsorted(B, t, 'right') - 1.  Output index is
[k, c, y, x]:

  count         int32   [K,2,H,W]  events per pixel, channel 0 = OFF, 1 = ON
  voxel         float32 [K,B,H,W]  tau = (B - 1) * ((t - B_k) / (B_k+1 - B_k)), b0 = floor(tau), frac = tau - b0; the weights are
                                   integers in units of 2^-24, q1 = rint(frac * 2^24) (half to even), q0 = 2^24 - q1; p * q0 goes to
                                   bin b0 and (when q1 != 0) p * q1 to bin b0 + 1, summed in int64; the value is
                                   float32(float64(sum) * 2^-24).  Per window and pixel the bins sum to exactly ON - OFF.
  time_surface  float32 [K,2,H,W]  the time stamp (the row's float32 t itself) of the latest event of that polarity at that pixel
                                   with t < B_k+1, counted from the clip's first window; -inf where there is none

Every scattered update is an integer atomic (v2e_amd/csrc/tensorize.hip), so the tensors do not depend on the order of the rows
or on how the clip is cut into runs: the window a run ends in stays open, its accumulators (a count plane, an int64 voxel plane,
the surface's key planes) are carried on the device to the next `add_run`, and `flush` hands it out at the end of the clip.
`add_run` fits the `on_events` callbacks of `VideoToEvents.run_stream` and `SyntheticToEvents.run`; it enqueues on the current
stream and, given the run's end time (`t_end` or `frame_times`), never waits for the device.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from ._capi import check, ptr, stream_ptr

REPRESENTATIONS = ("count", "voxel", "time_surface")
MAX_RUN_WINDOWS = 1 << 22  # windows one run may touch before add_run refuses (a time stamp far from the others)
_KEY_NEG_INF = 0x007FFFFF  # the surface key of -inf (tensorize.hip)


def _uniform_done(t_end, t_start, window_s):
    """Number of uniform windows that are complete at t_end: the largest j >= 0 with B_j <= t_end, B_j = t_start + j * window_s as
    the kernel forms it (floor of the quotient, corrected by one against the bounds)."""
    if not t_end >= t_start:
        return 0
    j = int(math.floor((t_end - t_start) / window_s))
    if t_start + float(j) * window_s > t_end:
        j -= 1
    elif t_start + float(j + 1) * window_s <= t_end:
        j += 1
    return max(j, 0)


def plan_windows(t_end, k_open=0, window_s=None, t_start=0.0, bounds=None, voxel_plane_bytes=0, max_scratch_bytes=1 << 30):
    """Host arithmetic of one run: which windows it completes and how the voxel scratch is cut.  The clip's windows from
    `k_open` on (the first one not handed out yet) are complete where B_k+1 <= t_end.  voxel_plane_bytes: int64 scratch of one
    window (8 * bins * H * W; 0 without voxel grids).  Returns (n_complete, has_open, blocks): the run hands out windows k_open ..
    k_open + n_complete - 1, the next one stays open (has_open; False once an explicit table is used up), and blocks is the list of
    [a, b) ranges of the complete windows (run-local) whose scratch stays within max_scratch_bytes -- at least one window per
    block.  Raises ValueError for more than MAX_RUN_WINDOWS windows in one run."""
    if (window_s is None) == (bounds is None):
        raise ValueError("plan_windows: exactly one of window_s / bounds")
    t_end = float(t_end)
    if math.isnan(t_end):
        raise ValueError("plan_windows: t_end is NaN")
    k_open = int(k_open)
    if bounds is None:
        if not (window_s > 0 and math.isfinite(window_s) and math.isfinite(t_start)):
            raise ValueError("plan_windows: window_s must be positive and finite")
        if t_end == math.inf:
            raise ValueError("plan_windows: uniform windows need a finite t_end")
        done, has_open = _uniform_done(t_end, float(t_start), float(window_s)), True
    else:
        b = np.asarray(bounds, dtype=np.float64).reshape(-1)
        K = len(b) - 1
        done = min(max(int(np.searchsorted(b, t_end, side="right")) - 1, 0), K)
        has_open = max(done, k_open) < K
    n_complete = max(done - k_open, 0)
    if n_complete + (1 if has_open else 0) > MAX_RUN_WINDOWS:
        raise ValueError("one run would touch %d windows (more than %d): t_end = %r" % (n_complete + 1, MAX_RUN_WINDOWS, t_end))
    blocks = []
    if n_complete:
        per = n_complete if voxel_plane_bytes <= 0 else max(1, int(max_scratch_bytes) // int(voxel_plane_bytes))
        blocks = [(a, min(a + per, n_complete)) for a in range(0, n_complete, per)]
    return n_complete, has_open, blocks


class EventTensorizer(object):
    """Count images, voxel grids and time surfaces of a clip's windows from the device rows of its runs (module docstring)."""

    def __init__(self, height, width, representations=("count",), window_s=None, t_start=0.0, bounds=None, voxel_bins=5,
                 frame_times=None, max_scratch_bytes=1 << 30, device="cuda:0"):
        self.height, self.width = int(height), int(width)
        if self.height < 1 or self.width < 1:
            raise ValueError("EventTensorizer: height and width must be positive")
        reps = (representations,) if isinstance(representations, str) else tuple(representations)
        if not reps or len(set(reps)) != len(reps) or any(r not in REPRESENTATIONS for r in reps):
            raise ValueError("EventTensorizer: representations must be a non-empty subset of %r, got %r" % (REPRESENTATIONS, reps))
        self.representations = reps
        if (window_s is None) == (bounds is None):
            raise ValueError("EventTensorizer: exactly one of window_s / bounds must be given")
        self.window_s = self.bounds = None
        self.t_start = float(t_start)
        if bounds is None:
            self.window_s = float(window_s)
            if not (self.window_s > 0 and math.isfinite(self.window_s) and math.isfinite(self.t_start)):
                raise ValueError("EventTensorizer: window_s must be positive and finite")
            if not self.t_start + self.window_s > self.t_start:
                raise ValueError("EventTensorizer: window_s %g does not advance t_start %g" % (self.window_s, self.t_start))
        else:
            b = np.array(bounds, dtype=np.float64).reshape(-1)
            if len(b) < 2 or not np.all(np.isfinite(b)) or np.any(np.diff(b) < 0):
                raise ValueError("EventTensorizer: bounds must be at least two finite ascending values")
            self.bounds = b
        self.voxel_bins = int(voxel_bins)
        if "voxel" in reps and self.voxel_bins < 1:
            raise ValueError("EventTensorizer: voxel_bins must be at least 1")
        self.max_scratch_bytes = int(max_scratch_bytes)
        if self.max_scratch_bytes < 1:
            raise ValueError("EventTensorizer: max_scratch_bytes must be positive")
        self.frame_times = None if frame_times is None else np.asarray(frame_times, dtype=np.float64).reshape(-1)
        _capi.require_gpu("EventTensorizer")
        self.device = dev = torch.device(device)
        H, W, B = self.height, self.width, self.voxel_bins
        self.k_open = 0          # clip index of the open window: the first one not handed out yet
        self.host_syncs = 0
        self.scatter_launches = 0
        self._t_end = -math.inf
        self._counters = torch.zeros((3,), dtype=torch.int64, device=dev)
        self._bounds_dev = None if self.bounds is None else torch.from_numpy(self.bounds).to(dev)
        # the open window's accumulators, and the surface's running maximum over the windows handed out
        self._count_open = torch.zeros((2, H, W), dtype=torch.int32, device=dev) if "count" in reps else None
        self._voxel_open = torch.zeros((B, H, W), dtype=torch.int64, device=dev) if "voxel" in reps else None
        self._surf_open = torch.zeros((2, H, W), dtype=torch.int32, device=dev) if "time_surface" in reps else None
        self._surf_state = torch.full((2, H, W), _KEY_NEG_INF, dtype=torch.int32, device=dev) if "time_surface" in reps else None

    # ------------------------------------------------------------------------------------------------------------ helpers
    _DTYPES = {"count": torch.int32, "voxel": torch.float32, "time_surface": torch.float32}

    def _channels(self, rep):
        return self.voxel_bins if rep == "voxel" else 2

    def _output(self, rep, n, out):
        shape = (self._channels(rep), self.height, self.width)
        if out is None or rep not in out:
            return torch.empty((n,) + shape, dtype=self._DTYPES[rep], device=self.device)
        o = out[rep]
        if not (torch.is_tensor(o) and o.device == self.device and o.dtype == self._DTYPES[rep] and o.is_contiguous()
                and o.dim() == 4 and tuple(o.shape[1:]) == shape and o.shape[0] >= n):
            raise ValueError("out[%r] must be a contiguous %s device tensor [>= %d, %d, %d, %d]" % ((rep, self._DTYPES[rep], n) + shape))
        return o[:n]

    def _run_t_end(self, events, n, counts, frame0, t_end):
        if t_end is not None:
            return float(t_end)
        if self.frame_times is not None and counts is not None:
            return float(self.frame_times[(0 if frame0 is None else int(frame0)) + len(counts) - 1])
        if n:
            self.host_syncs += 1
            return float(events[n - 1, 0].item())  # ONE 4-byte read-back
        return self._t_end

    # ------------------------------------------------------------------------------------------------------------ the run
    def add_run(self, events, counts=None, frame0=None, t_end=None, out=None):
        """Add one run's rows (device float32 [N,4]; None or empty for a run without events) and hand out the windows it
        completes: those with B_k+1 <= t_end, where t_end is the argument, else frame_times[frame0 + len(counts) - 1] (frame0
        None: 0), else the last row's t (one 4-byte read-back, counted in `host_syncs`).  Returns {"windows": (first_index, n),
        <representation>: device tensor [n, ...]}.  Rows of later windows than the one t_end falls in are skipped and counted
        (n_after), as are rows of windows already handed out (n_before) and malformed rows (n_bad): see `check`.
        out: {representation: tensor}: write the run's planes into the first n planes of caller-supplied tensors."""
        if events is not None and not (torch.is_tensor(events) and events.is_cuda):
            raise TypeError("EventTensorizer.add_run takes the run's rows as a device tensor")
        n = 0 if events is None else int(events.shape[0])
        if n:
            if events.dim() != 2 or events.shape[1] != 4:
                raise ValueError("EventTensorizer.add_run: rows must be [N,4]")
            events = events.to(self.device, torch.float32).contiguous()
        t_end = self._run_t_end(events, n, counts, frame0, t_end)
        H, W, B = self.height, self.width, self.voxel_bins
        voxel = "voxel" in self.representations
        nc, has_open, blocks = plan_windows(t_end, self.k_open, self.window_s, self.t_start, self.bounds,
                                            8 * B * H * W if voxel else 0, self.max_scratch_bytes)
        self._t_end = max(self._t_end, t_end)
        lib, stream, first = _capi.lib(), stream_ptr(self.device), self.k_open
        res = {"windows": (first, nc)}
        for rep in self.representations:
            res[rep] = self._output(rep, nc, out)
        pw = 2 * H * W  # 32-bit words of a count / surface plane
        if nc:
            for rep, carry in (("count", self._count_open), ("time_surface", self._surf_open)):
                if carry is not None:
                    check(lib.v2e_tensorize_move_zero(ptr(res[rep]), nc * pw, ptr(carry), pw, stream), "v2e_tensorize_move_zero")
        acc = None
        if voxel and blocks:
            acc = torch.empty((max(b - a for a, b in blocks), B, H, W), dtype=torch.int64, device=self.device)
        bounds_ptr = None if self._bounds_dev is None else C.c_void_p(self._bounds_dev.data_ptr() + 8 * first)

        def scatter(nk, open_, block, all_reps):
            a, b = block
            check(lib.v2e_tensorize_scatter(ptr(events) if n else None, n, H, W, self.t_start, self.window_s or 0.0, bounds_ptr, first,
                                            nk, open_, ptr(res.get("count")) if all_reps and nc else None,
                                            ptr(self._count_open) if all_reps else None, ptr(acc) if b > a else None,
                                            ptr(self._voxel_open), a, b, B, ptr(res.get("time_surface")) if all_reps and nc else None,
                                            ptr(self._surf_open) if all_reps else None, ptr(self._counters) if all_reps else None,
                                            stream), "v2e_tensorize_scatter")
            self.scatter_launches += 1 if n else 0

        def voxel_block(a, b):
            vw = 2 * B * H * W  # 32-bit words of an int64 voxel plane
            check(lib.v2e_tensorize_move_zero(ptr(acc), (b - a) * vw, ptr(self._voxel_open) if a == 0 else None, vw if a == 0 else 0,
                                              stream), "v2e_tensorize_move_zero")

        # the first launch feeds every representation, the open window and the counters; the voxel blocks after the first re-read
        # the rows for their own windows only
        first_block = blocks[0] if voxel and blocks else (0, 0)
        if first_block[1] > first_block[0]:
            voxel_block(*first_block)
        scatter(nc + (1 if has_open else 0), 1 if has_open else 0, first_block, True)
        if voxel:
            for i, (a, b) in enumerate(blocks):
                if i:
                    voxel_block(a, b)
                    scatter(nc, 0, (a, b), False)
                check(lib.v2e_tensorize_voxel_finish(ptr(acc), (b - a) * B * H * W, ptr(res["voxel"][a:b]), 0, stream),
                      "v2e_tensorize_voxel_finish")
        if nc and self._surf_state is not None:
            check(lib.v2e_tensorize_surface_finish(ptr(res["time_surface"]), nc, pw, ptr(self._surf_state), stream),
                  "v2e_tensorize_surface_finish")
        self.k_open = first + nc
        return res

    def flush(self, out=None):
        """The open window as the clip's final, partial one: {"windows": (index, 1), <representation>: [1, ...]}; the next window
        is open afterwards.  With an explicit table that is used up: (K, 0) and empty tensors."""
        lib, stream, first = _capi.lib(), stream_ptr(self.device), self.k_open
        n = 0 if self.bounds is not None and first >= len(self.bounds) - 1 else 1
        res = {"windows": (first, n)}
        for rep in self.representations:
            res[rep] = self._output(rep, n, out)
        if n == 0:
            return res
        H, W, B = self.height, self.width, self.voxel_bins
        pw = 2 * H * W
        for rep, carry in (("count", self._count_open), ("time_surface", self._surf_open)):
            if carry is not None:
                check(lib.v2e_tensorize_move_zero(ptr(res[rep]), pw, ptr(carry), pw, stream), "v2e_tensorize_move_zero")
        if self._voxel_open is not None:
            check(lib.v2e_tensorize_voxel_finish(ptr(self._voxel_open), B * H * W, ptr(res["voxel"]), 1, stream),
                  "v2e_tensorize_voxel_finish")
        if self._surf_state is not None:
            check(lib.v2e_tensorize_surface_finish(ptr(res["time_surface"]), 1, pw, ptr(self._surf_state), stream),
                  "v2e_tensorize_surface_finish")
        self.k_open = first + 1
        return res

    def open_window(self):
        """The accumulators of the open window as they stand, copies: {"index": k, "count": int32 [2,H,W], "voxel_acc": int64
        [B,H,W] in units of 2^-24 (its bins sum to exactly 2^24 * (ON - OFF) per pixel), "time_surface_keys": int32 [2,H,W]}."""
        res = {"index": self.k_open}
        for name, t in (("count", self._count_open), ("voxel_acc", self._voxel_open), ("time_surface_keys", self._surf_open)):
            if t is not None:
                res[name] = t.clone()
        return res

    def surface_state(self):
        """The time surface behind the last window handed out, float32 [2,H,W] (-inf: no event yet): a copy."""
        if self._surf_state is None:
            raise ValueError("EventTensorizer: no time_surface representation")
        k = self._surf_state.to(torch.int64) & 0xFFFFFFFF
        bits = torch.where(k >= 0x80000000, k ^ 0x80000000, k ^ 0xFFFFFFFF)
        return torch.where(bits >= 0x80000000, bits - (1 << 32), bits).to(torch.int32).view(torch.float32)

    def check(self):
        """Read the row counters back (one read-back) and return {"n_bad", "n_before", "n_after"}; ValueError if any row was
        malformed (x outside [0,W), y outside [0,H), a fractional coordinate, p other than +-1, a NaN time stamp)."""
        self.host_syncs += 1
        n_bad, n_before, n_after = (int(v) for v in self._counters.tolist())
        if n_bad > 0:
            raise ValueError("EventTensorizer: %d malformed rows were skipped (n_before %d, n_after %d)" % (n_bad, n_before, n_after))
        return {"n_bad": n_bad, "n_before": n_before, "n_after": n_after}

    def counters(self):
        """{"n_bad", "n_before", "n_after"} read back without raising."""
        self.host_syncs += 1
        return dict(zip(("n_bad", "n_before", "n_after"), (int(v) for v in self._counters.tolist())))
