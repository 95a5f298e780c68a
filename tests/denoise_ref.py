"""Two numpy implementations of DenoiseSweep's definition (v2e_amd/denoise.py) and the rows the tests share.  No GPU."""
import numpy as np

_NEIGHBOURS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


def row_is_bad(row, H, W):
    t, x, y = float(row[0]), float(row[1]), float(row[2])
    return not (np.isfinite(t) and x == np.floor(x) and y == np.floor(y) and 0 <= x < W and 0 <= y < H)


def _finish(ages, valid, taus, labels, keep):
    """ages: float64 [n,8] (rows of bad events unused) -> (hist, n_bad, mask)."""
    taus = np.asarray(taus, dtype=np.float64)
    T = len(taus)
    n = len(ages)
    hist = np.zeros((8, 2, T + 1), dtype=np.int64)
    mask = None if keep is None else np.zeros(n, dtype=bool)
    a = np.sort(ages, axis=1)
    lab = np.ones(n, dtype=np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    for k in range(8):
        b = np.searchsorted(taus, a[valid, k], side="left")
        np.add.at(hist[k], (lab[valid], b), 1)
    if keep is not None:
        mask[valid] = a[valid, keep[0] - 1] <= float(keep[1])
    return hist, int(n - valid.sum()), mask


def stcf_serial(rows, H, W, taus, labels, last_t=None, keep=None):
    """The plain loop with a timestamp map.  rows float32 [n,4]; labels bool [n] or None (all signal); last_t float32 [H,W] or None
    (-inf), not modified.  Returns (hist int64 [8,2,T+1], n_bad, mask bool [n] or None, the map after the rows)."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n = len(rows)
    m = np.full((H, W), -np.inf, dtype=np.float32) if last_t is None else np.array(last_t, dtype=np.float32)
    ages = np.full((n, 8), np.inf, dtype=np.float64)
    valid = np.zeros(n, dtype=bool)
    for i in range(n):
        if row_is_bad(rows[i], H, W):
            continue
        valid[i] = True
        x, y = int(rows[i, 1]), int(rows[i, 2])
        for j, (dx, dy) in enumerate(_NEIGHBOURS):
            qx, qy = x + dx, y + dy
            if 0 <= qx < W and 0 <= qy < H:
                ages[i, j] = np.float64(rows[i, 0]) - np.float64(m[qy, qx])
        m[y, x] = rows[i, 0]
    hist, n_bad, mask = _finish(ages, valid, taus, labels, keep)
    return hist, n_bad, mask, m


def stcf_bruteforce(rows, H, W, taus, labels, last_t=None, keep=None):
    """For every row, scan all earlier rows for the latest one at each neighbour pixel: O(n^2), for n <= 2000.  No map is kept:
    the one returned is built from the last row of every pixel."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n = len(rows)
    assert n <= 2000
    m0 = np.full((H, W), -np.inf, dtype=np.float32) if last_t is None else np.array(last_t, dtype=np.float32)
    bad = np.array([row_is_bad(r, H, W) for r in rows], dtype=bool)
    ages = np.full((n, 8), np.inf, dtype=np.float64)
    for i in range(n):
        if bad[i]:
            continue
        x, y = int(rows[i, 1]), int(rows[i, 2])
        for j, (dx, dy) in enumerate(_NEIGHBOURS):
            qx, qy = x + dx, y + dy
            if not (0 <= qx < W and 0 <= qy < H):
                continue
            tq = m0[qy, qx]
            for e in range(i - 1, -1, -1):
                if not bad[e] and rows[e, 1] == qx and rows[e, 2] == qy:
                    tq = rows[e, 0]
                    break
            ages[i, j] = np.float64(rows[i, 0]) - np.float64(tq)
    m = m0.copy()
    for i in range(n):
        if not bad[i]:
            m[int(rows[i, 2]), int(rows[i, 1])] = rows[i, 0]
    hist, n_bad, mask = _finish(ages, ~bad, taus, labels, keep)
    return hist, n_bad, mask, m


def labels_from_counts(counts, n_signal):
    """bool [sum(counts)]: frame f's first n_signal[f] rows are signal."""
    out = []
    for c, s in zip(np.asarray(counts).tolist(), np.asarray(n_signal).tolist()):
        out.append(np.arange(c) < s)
    return np.concatenate(out) if out else np.zeros(0, dtype=bool)


def border_rows(H=5, W=7, n=3000, seed=7):
    """Hand-made rows for the border / tie cases: times are multiples of 2^-10 (ages exact) that advance by 0 .. 3 units, so many
    rows share a time stamp; about 5 % of the rows are out of order (up to 40 units back); a tenth sit in the corners, a tenth on
    the edges; 3 % are bad (NaN t, inf t, x = W, y = -1, x = 2.5 in turn).  Returns (rows float32 [n,4], labels bool [n])."""
    rng = np.random.RandomState(seed)
    u = 2.0 ** -10
    t = np.cumsum(rng.randint(0, 4, size=n)).astype(np.float64)
    late = rng.rand(n) < 0.05
    t[late] -= rng.randint(1, 41, size=int(late.sum()))
    x = rng.randint(0, W, size=n).astype(np.float64)
    y = rng.randint(0, H, size=n).astype(np.float64)
    where = rng.rand(n)
    corner = where < 0.1
    x[corner] = rng.choice([0, W - 1], size=int(corner.sum()))
    y[corner] = rng.choice([0, H - 1], size=int(corner.sum()))
    edge = (where >= 0.1) & (where < 0.2)
    y[edge] = rng.choice([0, H - 1], size=int(edge.sum()))
    rows = np.stack([t * u, x, y, rng.choice([-1.0, 1.0], size=n)], axis=1).astype(np.float32)
    bad = np.flatnonzero(rng.rand(n) < 0.03)
    for j, i in enumerate(bad):
        kind = j % 5
        if kind == 0:
            rows[i, 0] = np.nan
        elif kind == 1:
            rows[i, 0] = np.inf
        elif kind == 2:
            rows[i, 1] = W
        elif kind == 3:
            rows[i, 2] = -1
        else:
            rows[i, 1] = 2.5
    labels = rng.rand(n) < 0.6
    return rows, labels


BORDER_TAUS = [0.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6, 1.0]
NOISY_DOT_RATE_HZ = 5.0  # shot_noise_rate_hz of the labelled clip: philox_moving_dot_64x64's frames and other parameters
