"""What the `add_run` of the row consumers shares (`DenoiseSweep`, `WindowSweep`, `DoubleWindowSweep`, `EventStats`, `MLPFilter`,
`EventPatches`): the check of (rows, counts, n_signal, labels), the labels' way to the device and into an entry point's arguments,
the return of a run without rows, and the two ways a call's rows are taken in passes of at most `max_rows_per_pass` rows.
`RowPasses` builds the row index of v2e_amd/csrc/rowkeys.h per pass -- each row gets the key pixel << 32 | row (v2e_denoise_keys),
the keys are sorted (torch.sort) and each pixel's stretch of the sorted keys is found (v2e_denoise_segments); `WindowPasses`
compacts the packed words of a pass's valid rows behind the carried ones (v2e_window_compact) -- before the caller's own kernels read
it.  The checks take the caller's name: the messages are the caller's."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import check, ptr, stream_ptr

DEFAULT_ROWS_PER_PASS = 1 << 25


def check_sensor(name, height, width):
    height, width = int(height), int(width)
    if height < 1 or width < 1 or height * width > 0x7FFFFFFF:
        raise ValueError("%s: height and width must be positive (and height * width below 2^31)" % name)
    return height, width


def check_rows_per_pass(name, max_rows_per_pass):
    max_rows_per_pass = int(max_rows_per_pass)
    if not 1 <= max_rows_per_pass <= 1 << 30:
        raise ValueError("%s: max_rows_per_pass must be in 1 .. 2^30" % name)
    return max_rows_per_pass


def label_bounds(counts, n_signal, who="DenoiseSweep.add_run"):
    """The frame table of `add_run(counts=, n_signal=)` as one ascending int64 table of row indices, [2F]: frame f's signal rows
    start at entry 2f (the sum of the counts before it), its noise rows at entry 2f + 1 (n_signal[f] rows later).  A row is a signal
    row iff an odd number of entries is <= its index.  Returns (table, rows the counts cover)."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    s = np.asarray(n_signal, dtype=np.int64).reshape(-1)
    if len(s) != len(c):
        raise ValueError("%s: n_signal has %d entries, counts %d" % (who, len(s), len(c)))
    if np.any(c < 0) or np.any(s < 0) or np.any(s > c):
        raise ValueError("%s: need 0 <= n_signal[f] <= counts[f] in every frame" % who)
    off = np.concatenate([[0], np.cumsum(c)])
    b = np.empty(2 * len(c), dtype=np.int64)
    b[0::2] = off[:-1]
    b[1::2] = off[:-1] + s
    return b, int(off[-1])


def check_run(name, rows, counts=None, n_signal=None, labels=None, host_error=ValueError):
    """The arguments of `name`.add_run, checked before the library or the device is touched, in this order: the label sources, the
    frame table, the rows, the labels, the rows the counts cover, and last that the rows are on a device.  host_error: what rows
    that are no tensor, or a host tensor, raise -- TypeError (the sweeps) or ValueError.  Returns (n, labels as a bool tensor or
    None, the table of label_bounds or None)."""
    who = name + ".add_run"
    if labels is not None and n_signal is not None:
        raise ValueError("%s: labels or n_signal, not both" % who)
    if n_signal is not None and counts is None:
        raise ValueError("%s: n_signal needs the run's counts" % who)
    bounds = covered = None
    if n_signal is not None:
        bounds, covered = label_bounds(counts, n_signal, who)
    if host_error is TypeError:
        not_device, bad_rows = "%s takes the run's rows as a device tensor" % who, "%s: rows must be float32 [n,4]" % who
    else:
        not_device = bad_rows = "%s: rows must be a device float32 [n,4] tensor" % who
    if rows is not None:
        if not torch.is_tensor(rows):
            raise host_error(not_device)
        if rows.dim() != 2 or rows.shape[1] != 4 or rows.dtype != torch.float32:
            raise ValueError(bad_rows)
    n = 0 if rows is None else int(rows.shape[0])
    if labels is not None:
        if not torch.is_tensor(labels):
            labels = torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
        if labels.dtype != torch.bool or labels.dim() != 1 or int(labels.shape[0]) != n:
            raise ValueError("%s: labels must be bool [%d]" % (who, n))
    if covered is not None and covered != n:
        raise ValueError("%s: counts sum to %d rows, the run has %d" % (who, covered, n))
    if rows is not None and not rows.is_cuda:
        raise host_error(not_device)
    return n, labels, bounds


def labels_to_device(labels, bounds, device):
    """check_run's labels and table on the device without waiting for it: (uint8 [n] or None, int64 [2F] or None).  The table goes
    through pinned memory of torch's caching host allocator, which keeps the block until the copy has run."""
    lab = None if labels is None else labels.to(device, non_blocking=True).to(torch.uint8).contiguous()
    lb = None if bounds is None else torch.from_numpy(bounds).pin_memory().to(device, non_blocking=True)
    return lab, lb


def row_ptr(t, r0):
    """A one-byte-per-row tensor from row r0 on as the pointer the entry points take; None stays None (NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr() + r0)


def label_args(lab, lb, r0):
    """(labels, label_bounds, n_label_bounds, row0) of a labelled entry point for the pass that starts at row r0."""
    return row_ptr(lab, r0), ptr(lb), 0 if lb is None else int(lb.shape[0]), r0


def new_seg(height, width, device):
    """The stretch table of a pass, int32 [H*W + 1]: one per sweep, rewritten by every pass."""
    return torch.empty((height * width + 1,), dtype=torch.int32, device=device)


def new_mask(keep, n, device):
    """The keep mask of a call of n rows as the uint8 [n] the kernels write, None for keep None; add_run returns its bool view."""
    return None if keep is None else torch.empty((n,), dtype=torch.uint8, device=device)


def no_rows(device, mask=False, keep=None):
    """What add_run returns for a run without rows: {"n", "n_bad"}, 0-dim int64 zeros on the device, and for a caller whose result
    has one (mask=True) "mask": None, or an empty bool tensor when keep was asked for."""
    zero = torch.zeros((), dtype=torch.int64, device=device)
    out = {"n": zero, "n_bad": zero.clone()}
    if mask:
        out["mask"] = None if keep is None else torch.zeros((0,), dtype=torch.bool, device=device)
    return out


class RowPasses(object):
    """The passes of one add_run call of `owner` (its height, width, device and max_rows_per_pass; its .passes counts them).
    Iterating yields (r0, m, rows[r0:r0 + m], sorted keys) per pass with `seg` holding that pass's stretches; the caller's kernels go
    in the loop body.  keep: a uint8 [n] mask in which v2e_denoise_keys clears the bad rows, or None.  n and n_bad are the call's
    valid and bad rows, 0-dim int64 device tensors the passes add to."""

    def __init__(self, owner, rows, seg, keep=None):
        self.owner, self.rows, self.seg, self.keep = owner, rows, seg, keep
        cnt = torch.zeros((2,), dtype=torch.int64, device=owner.device)
        self.cnt, self.n, self.n_bad = cnt, cnt[0], cnt[1]

    def keep_ptr(self, r0):
        """The keep mask from row r0 on as the pointer the entry points take (None without a mask)."""
        return row_ptr(self.keep, r0)

    def __iter__(self):
        o, lib, stream = self.owner, _capi.lib(), stream_ptr(self.owner.device)
        n = int(self.rows.shape[0])
        for r0 in range(0, n, o.max_rows_per_pass):
            m = min(o.max_rows_per_pass, n - r0)
            ev = self.rows[r0:r0 + m]
            keys = torch.empty((m,), dtype=torch.int64, device=o.device)
            check(lib.v2e_denoise_keys(ptr(ev), m, o.height, o.width, ptr(keys), self.keep_ptr(r0), stream), "v2e_denoise_keys")
            skeys = torch.sort(keys)[0]
            del keys
            check(lib.v2e_denoise_segments(ptr(skeys), m, o.height, o.width, ptr(self.seg), ptr(self.cnt), stream), "v2e_denoise_segments")
            yield r0, m, ev, skeys
            o.passes += 1


class WindowPasses(RowPasses):
    """The passes of one add_run call of a compaction-based `owner`.  Each pass owns its scratch -- xy, int32 [len(tail) + m]: the
    words x | y << 16 of the pass's valid rows, in order, behind the carried words of `tail`; idx, int32 [m]: each word's row; a
    block table whose last entry, n_valid, is the pass's valid rows -- and fills it with v2e_window_compact, which also adds to
    `seen` (the owner's valid and bad rows so far) and clears the bad rows of keep.  Iterating yields (r0, m, xy, idx, n_valid);
    keep, keep_ptr, n and n_bad are RowPasses'."""

    def __init__(self, owner, rows, tail, seen, keep=None):
        RowPasses.__init__(self, owner, rows, None, keep)
        self.tail, self.seen = tail, seen

    def __iter__(self):
        o, lib, stream = self.owner, _capi.lib(), stream_ptr(self.owner.device)
        n, carried, dev = int(self.rows.shape[0]), int(self.tail.shape[0]), self.owner.device
        for r0 in range(0, n, o.max_rows_per_pass):
            m = min(o.max_rows_per_pass, n - r0)
            ev = self.rows[r0:r0 + m]
            xy = torch.empty((carried + m,), dtype=torch.int32, device=dev)
            idx = torch.empty((m,), dtype=torch.int32, device=dev)
            blk = torch.empty(((m + 255) // 256 + 1,), dtype=torch.int32, device=dev)  # (the last entry: the pass's valid rows)
            n_valid = blk[-1:]
            check(lib.v2e_window_compact(ptr(ev), m, o.height, o.width, ptr(self.tail), carried, ptr(xy), ptr(idx), ptr(blk), ptr(n_valid),
                                         ptr(self.cnt), ptr(self.seen), self.keep_ptr(r0), stream), "v2e_window_compact")
            yield r0, m, xy, idx, n_valid
            o.passes += 1
