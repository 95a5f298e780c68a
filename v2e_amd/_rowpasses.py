"""What `DenoiseSweep` and `EventPatches` share: a call's rows are taken in passes of at most `max_rows_per_pass` rows, and every
pass builds the row index of v2e_amd/csrc/rowkeys.h -- each row gets the key pixel << 32 | row (v2e_denoise_keys), the keys are
sorted (torch.sort) and each pixel's stretch of the sorted keys is found (v2e_denoise_segments) -- before the caller's own kernels
read it.  The checks take the caller's name: the messages are the caller's."""
import ctypes as C

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


def new_seg(height, width, device):
    """The stretch table of a pass, int32 [H*W + 1]: one per sweep, rewritten by every pass."""
    return torch.empty((height * width + 1,), dtype=torch.int32, device=device)


def no_rows(device):
    """(n, n_bad) of a run without rows: 0-dim int64 zeros on the device."""
    zero = torch.zeros((), dtype=torch.int64, device=device)
    return zero, zero.clone()


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
        return None if self.keep is None else C.c_void_p(self.keep.data_ptr() + r0)

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
