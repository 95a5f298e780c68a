"""The numpy statement of DoubleWindowSweep's definition (v2e_amd/dwindow.py): the double-window filter as a plain loop for one
setting, the same filter for a whole table of settings (vectorised over the settings, pinned by the plain loop in
tests/test_double_window_sweep.py), and the cases the tests share.  No GPU, and no code shared with the kernels."""
import numpy as np

from denoise_ref import labels_from_counts, row_is_bad  # noqa: F401  (the bad-row rule is DenoiseSweep's)
from window_filter_ref import border_rows, full_window_rows  # noqa: F401  (the rows are WindowSweep's cases)

XY_NONE = 0xFFFFFFFF

BORDER_LENGTHS = (1, 2, 3, 5, 8)
BORDER_SIGMAS = (0, 1, 3)
BORDER_SUPPORTS = (1, 2, 3, 4)
BORDER_KEEPS = ((3, 1, 1), (8, 1, 3))  # (L, sigma, k): entries of all three tables
FULL_LENGTHS = (1, 33, 64, 65, 129, 512)  # both sides of the 64-lane stride, and the longest window
FULL_SIGMAS = (0, 2, 12)
FULL_SUPPORTS = (1, 2, 4)
FULL_KEEP = (512, 0, 4)
FULL_N, FULL_BAD, FULL_H, FULL_W = 6000, 250, 33, 37
# the real-rows case: the first CLIP_FRAMES frames of philox_moving_dot_64x64 with shot noise
CLIP_FRAMES, CLIP_LENGTHS, CLIP_SIGMAS, CLIP_SUPPORTS, CLIP_KEEP = 100, (1, 2, 4, 8, 16, 32, 64, 128), (1, 2, 4), (1, 2), (16, 2, 1)


def dwf_bruteforce(rows, H, W, L, sigma, k):
    """DWF(L, sigma, k) applied directly, two Python lists as the windows.  Returns (passed bool [n], valid bool [n], R, N): the
    lists of (x, y) the windows hold after the rows, the oldest first."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n = len(rows)
    passed, valid = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    R, N = [], []
    for i in range(n):
        if row_is_bad(rows[i], H, W):
            continue
        valid[i] = True
        x, y = int(rows[i, 1]), int(rows[i, 2])
        c = sum(1 for (xx, yy) in R + N if abs(xx - x) + abs(yy - y) <= sigma)
        passed[i] = c >= k
        win = R if passed[i] else N
        win.append((x, y))
        if len(win) > L:
            del win[0]
    return passed, valid, R, N


def window_words(win, lmax):
    """A window's list of (x, y), the oldest first, in the layout of DoubleWindowSweep.windows: int64 [lmax], the latest last."""
    words = [x | (y << 16) for (x, y) in win]
    return np.array([XY_NONE] * (lmax - len(words)) + words, dtype=np.int64)


def dwf_serial(rows, H, W, lengths, sigmas, supports, labels=None, windows=None, keep=None):
    """The whole table row by row, every setting at once.  rows float32 [n,4]; labels bool [n] or None (all signal); windows: the
    windows carried in, int64 [NK,S,NL,2,Lmax] in DoubleWindowSweep.windows' layout, or None (all empty); not modified.
    keep = (L, sigma, k), entries of the tables, or None.  Returns (passed int64 [NK,S,NL,2], n_signal, n_noise, n_bad, mask bool
    [n] or None, the windows after the rows)."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    lengths, sigmas, supports = (np.asarray(t, dtype=np.int64).reshape(-1) for t in (lengths, sigmas, supports))
    NK, S, NL, lmax = len(supports), len(sigmas), len(lengths), int(lengths[-1])
    F, n = NK * S * NL, len(rows)
    kk, ss, ll = (a.reshape(-1) for a in np.meshgrid(supports, sigmas, lengths, indexing="ij"))  # per setting, in C order
    # per setting and window a row of lmax slots of which the first L are used round-robin; age[f, w, slot]: the number of the
    # insertion that filled the slot, -1 while it is empty
    wx = np.zeros((F, 2, lmax), dtype=np.int64)
    wy = np.zeros((F, 2, lmax), dtype=np.int64)
    age = np.full((F, 2, lmax), -1, dtype=np.int64)
    clock = np.zeros((F, 2), dtype=np.int64)  # insertions into each window so far
    if windows is not None:
        carried = np.asarray(windows, dtype=np.int64).reshape(F, 2, lmax)
        for f in range(F):
            for w in range(2):
                words = [int(v) for v in carried[f, w] if int(v) != XY_NONE]
                assert len(words) <= ll[f]
                for v in words:
                    slot = clock[f, w] % ll[f]
                    wx[f, w, slot], wy[f, w, slot], age[f, w, slot] = v & 0xFFFF, v >> 16, clock[f, w]
                    clock[f, w] += 1
    passed = np.zeros((F, 2), dtype=np.int64)
    mask = None if keep is None else np.zeros(n, dtype=bool)
    keep_f = None
    if keep is not None:
        keep_f = int(np.flatnonzero((ll == keep[0]) & (ss == keep[1]) & (kk == keep[2]))[0])
    n_bad, totals = 0, [0, 0]
    every = np.arange(F)
    for i in range(n):
        if row_is_bad(rows[i], H, W):
            n_bad += 1
            continue
        x, y = int(rows[i, 1]), int(rows[i, 2])
        label = 1 if labels is None else int(bool(labels[i]))
        totals[label] += 1
        near = (np.abs(wx - x) + np.abs(wy - y) <= ss[:, None, None]) & (age >= 0)
        ok = near.sum(axis=(1, 2)) >= kk
        passed[ok, label] += 1
        if keep_f is not None:
            mask[i] = ok[keep_f]
        w = np.where(ok, 0, 1)
        slot = clock[every, w] % ll
        wx[every, w, slot], wy[every, w, slot], age[every, w, slot] = x, y, clock[every, w]
        clock[every, w] += 1
    out = np.full((F, 2, lmax), XY_NONE, dtype=np.int64)
    for f in range(F):
        for w in range(2):
            order = [s for s in np.argsort(age[f, w], kind="stable") if age[f, w, s] >= 0]
            out[f, w] = window_words([(int(wx[f, w, s]), int(wy[f, w, s])) for s in order], lmax)
    return passed.reshape(NK, S, NL, 2), totals[1], totals[0], n_bad, mask, out.reshape(NK, S, NL, 2, lmax)


def burst_rows():
    """The packet that tells the two filters apart, at 64x64 with (L, sigma, k) = (4, 1, 1): three rows at one pixel (the second
    and third pass and sit in R), nine rows on pixels at least 3 apart from everything else (all fail: a burst of noise that
    flushes a window of 4 and of 8), then one row next to the first pixel.  Returns rows float32 [13,4]."""
    xy = [(10, 10)] * 3 + [(20 + 5 * (j % 3), 30 + 5 * (j // 3)) for j in range(9)] + [(11, 10)]
    return np.array([[j * 1e-3, x, y, 1.0] for j, (x, y) in enumerate(xy)], dtype=np.float32)
