"""The numpy statement of WindowSweep's definition (v2e_amd/window.py), a brute-force evaluation of the fixed-window filter per
setting, and the rows the tests share.  No GPU, and no code shared with the kernels."""
import numpy as np

from denoise_ref import labels_from_counts, row_is_bad  # noqa: F401  (the bad-row rule is DenoiseSweep's)

MAX_SUPPORT = 4
XY_NONE = 0xFFFFFFFF


def fwf_serial(rows, H, W, lengths, sigmas, labels=None, tail=None, keep=None):
    """The plain loop: row by row, a Python list as the window.  rows float32 [n,4]; labels bool [n] or None (all signal); tail: the
    window carried in, int64 [Lmax] of words x | y << 16, the latest last, XY_NONE where there is no row yet, or None (empty); not
    modified.  keep = (L, sigma, k) or None.  Returns (hist int64 [4,S,2,NL+1], n_bad, mask bool [n] or None, the tail after the
    rows)."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    lengths = np.asarray(lengths, dtype=np.int64)
    sigmas = [int(s) for s in sigmas]
    lmax, NL, S = int(lengths[-1]), len(lengths), len(sigmas)
    n = len(rows)
    wx, wy = [], []  # the window: x and y of the valid rows so far, the oldest first, at most lmax of them
    if tail is not None:
        words = [int(w) for w in np.asarray(tail).tolist() if int(w) != XY_NONE]
        wx, wy = [w & 0xFFFF for w in words], [w >> 16 for w in words]
    hist = np.zeros((MAX_SUPPORT, S, 2, NL + 1), dtype=np.int64)
    mask = None if keep is None else np.zeros(n, dtype=bool)
    n_bad = 0

    def depths(dist, sigma):
        """d[k-1], k = 1 .. 4, of one row: dist[j-1] is the distance to the row at depth j"""
        at = np.flatnonzero(dist <= sigma) + 1
        return [int(at[k]) if k < len(at) else lmax + 1 for k in range(MAX_SUPPORT)]

    for i in range(n):
        if row_is_bad(rows[i], H, W):
            n_bad += 1
            continue
        x, y = int(rows[i, 1]), int(rows[i, 2])
        label = 1 if labels is None else int(bool(labels[i]))
        dist = (np.abs(np.array(wx, dtype=np.int64) - x) + np.abs(np.array(wy, dtype=np.int64) - y))[::-1]  # depth 1 first
        for s, sigma in enumerate(sigmas):
            for k, d in enumerate(depths(dist, sigma)):
                hist[k, s, label, int(np.searchsorted(lengths, d, side="left"))] += 1
        if keep is not None:
            mask[i] = depths(dist, int(keep[1]))[int(keep[2]) - 1] <= int(keep[0])
        wx.append(x)
        wy.append(y)
        if len(wx) > lmax:
            del wx[0], wy[0]
    words = [xx | (yy << 16) for xx, yy in zip(wx, wy)]
    tail_out = np.array([XY_NONE] * (lmax - len(words)) + words, dtype=np.int64)
    return hist, n_bad, mask, tail_out


def fwf_bruteforce(rows, H, W, L, sigma, k):
    """FWF(L, sigma, k) applied directly: a row passes iff at least k of the last L valid rows before it lie within L1 distance
    sigma.  Returns (passed bool [n], valid bool [n])."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n = len(rows)
    passed, valid = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    window = []
    for i in range(n):
        if row_is_bad(rows[i], H, W):
            continue
        valid[i] = True
        x, y = int(rows[i, 1]), int(rows[i, 2])
        passed[i] = sum(1 for (xx, yy) in window if abs(xx - x) + abs(yy - y) <= sigma) >= k
        window.append((x, y))
        if len(window) > L:
            del window[0]
    return passed, valid


BORDER_LENGTHS = (1, 2, 3, 5, 8)
BORDER_SIGMAS = (0, 1, 3)
BORDER_KEEPS = ((3, 1, 1), (7, 2, 3))  # (L, sigma, k): the second one's L and sigma are no table entries


def border_rows(H=5, W=7, n=3000, seed=3):
    """Seeded uniform rows on a small sensor, about 120 of them bad in four ways in turn: NaN t, x + 0.5, y = H, x = -1.
    Returns (rows float32 [n,4], labels bool [n])."""
    rng = np.random.RandomState(seed)
    t = np.cumsum(rng.randint(0, 4, size=n)) * 2.0 ** -10
    x = rng.randint(0, W, size=n).astype(np.float64)
    y = rng.randint(0, H, size=n).astype(np.float64)
    rows = np.stack([t, x, y, rng.choice([-1.0, 1.0], size=n)], axis=1).astype(np.float32)
    bad = np.flatnonzero(rng.rand(n) < 0.036)
    for j, i in enumerate(bad):
        kind = j % 4
        if kind == 0:
            rows[i, 0] = np.nan
        elif kind == 1:
            rows[i, 1] += 0.5
        elif kind == 2:
            rows[i, 2] = H
        else:
            rows[i, 1] = -1
    labels = rng.rand(n) < 0.6
    return rows, labels


# 52 lengths from 1 to 1024: 1 .. 16, then 36 log-spaced ones from 20 on (their ratio, 1.12, keeps them apart)
FULL_LENGTHS = tuple(range(1, 17)) + tuple(int(v) for v in np.round(np.geomspace(20, 1024, 36)))
FULL_SIGMAS = (0, 1, 2, 3, 4, 6, 8, 12)
# the real-rows case: the first CLIP_FRAMES frames of philox_moving_dot_64x64 with shot noise, and its tables and keep = (L, sigma, k)
CLIP_FRAMES, CLIP_LENGTHS, CLIP_SIGMAS, CLIP_KEEP = 100, (1, 2, 4, 8, 16, 32, 64, 128), (1, 2, 4), (16, 2, 1)


def full_window_rows(H=33, W=37, n=12000, n_bad=500, frames=40, seed=21):
    """Rows that fill the longest window: 30 % on one pixel and its eight neighbours, the rest uniform, n_bad bad rows sprinkled in,
    labelled by a frame table.  Returns (rows float32 [n,4], counts, n_signal)."""
    rng = np.random.RandomState(seed)
    hot = rng.rand(n) < 0.3
    x = np.where(hot, 17 + rng.randint(-1, 2, size=n), rng.randint(0, W, size=n)).astype(np.float64)
    y = np.where(hot, 12 + rng.randint(-1, 2, size=n), rng.randint(0, H, size=n)).astype(np.float64)
    t = np.cumsum(rng.randint(0, 3, size=n)) * 2.0 ** -14
    rows = np.stack([t, x, y, np.ones(n)], axis=1).astype(np.float32)
    for j, i in enumerate(rng.choice(n, size=n_bad, replace=False)):
        if j % 2:
            rows[i, 0] = np.inf
        else:
            rows[i, 2] = -1
    counts = np.bincount(rng.randint(0, frames, size=n), minlength=frames)
    n_signal = (counts * rng.rand(frames)).astype(np.int64)
    return rows, counts, n_signal
