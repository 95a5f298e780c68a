"""Two numpy implementations of EventPatches' definition (v2e_amd/patches.py).  No GPU.

Rows and validity.  Rows are float32 [n,4] = (t, x = column, y = row, p), taken in row order.  A row is bad under exactly
DenoiseSweep's rule (denoise_ref.row_is_bad): t not finite, or x / y not an integer value inside [0,W) / [0,H).  p is not examined
for validity.  A bad row reads and writes no map and gets valid = False.  Its features are the "none" values below.

Carried maps.  last_t is float32 [H,W] and starts at -inf.  last_p is int8 [H,W] and starts at 0.

Per-row patch.  For a valid row i at (x, y) and every offset (dy, dx) in [-r, r]^2: the patch index is [dy + r, dx + r]; r is 1, 2
or 3; the centre is included.  Let q = (x + dx, y + dy).  If q is outside the sensor, the entry is none.  Otherwise T_q and P_q are
taken from the latest valid row j < i at q in this call: T_q is its t, P_q is the sign of its p (+1 if p > 0, else -1).  If no such
row exists in this call, the carried maps supply T_q and P_q.  A carried T_q of -inf means none.  age = float64(t_i) - float64(T_q).
A T_q later than t_i gives a negative age, which is kept.  The centre entry is the previous event at the same pixel.  The row is
never in its own patch.

After reading, the row stamps last_t[y,x] = t_i and last_p[y,x] = sign(p_i).

Output.  features is float32 [n, 2, P, P] with P = 2r+1.  mode="age": channel 0 is float32(age), rounded to nearest even; +inf
where none.  Channel 1 is P_q as +-1.0; 0 where none.  mode="linear" (tau > 0 finite), channel 0: 0 where none or age >= tau; 1
where age <= 0; otherwise float32(1 - age / tau), with the division and the subtraction each rounded in float64.  Channel 1: P_q
where channel 0's entry is not of the first kind, that is, not none and age < tau; otherwise 0.
"""
import numpy as np

from denoise_ref import row_is_bad


def _maps(H, W, last_t, last_p):
    t = np.full((H, W), -np.inf, dtype=np.float32) if last_t is None else np.array(last_t, dtype=np.float32)
    p = np.zeros((H, W), dtype=np.int8) if last_p is None else np.array(last_p, dtype=np.int8)
    assert t.shape == (H, W) and p.shape == (H, W)
    return t, p


def patches_serial(rows, H, W, r, mode, tau=None, last_t=None, last_p=None):
    """The plain loop over maps padded by r pixels of "none", the features of all rows made from the stored ages at the end.
    Returns (features float32 [n,2,P,P], valid bool [n], last_t float32 [H,W], last_p int8 [H,W]); the maps given are not modified."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n, P = len(rows), 2 * r + 1
    t0, p0 = _maps(H, W, last_t, last_p)
    mt = np.full((H + 2 * r, W + 2 * r), -np.inf, dtype=np.float32)
    mp = np.zeros((H + 2 * r, W + 2 * r), dtype=np.int8)
    mt[r:r + H, r:r + W], mp[r:r + H, r:r + W] = t0, p0
    age = np.full((n, P, P), np.inf, dtype=np.float64)
    pol = np.zeros((n, P, P), dtype=np.float32)
    none = np.ones((n, P, P), dtype=bool)
    valid = np.zeros(n, dtype=bool)
    for i in range(n):
        if row_is_bad(rows[i], H, W):
            continue
        valid[i] = True
        x, y = int(rows[i, 1]), int(rows[i, 2])
        win = mt[y:y + P, x:x + P]                                                  # (the window's centre is [y + r, x + r])
        none[i] = win == -np.inf
        age[i] = np.float64(rows[i, 0]) - win.astype(np.float64)
        pol[i] = mp[y:y + P, x:x + P]
        mt[y + r, x + r] = rows[i, 0]
        mp[y + r, x + r] = 1 if rows[i, 3] > 0 else -1
    feat = np.zeros((n, 2, P, P), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == "age":
            feat[:, 0] = np.where(none, np.float32(np.inf), age.astype(np.float32))
            feat[:, 1] = np.where(none, np.float32(0), pol)
        else:
            assert mode == "linear" and tau > 0 and np.isfinite(tau)
            tau = np.float64(tau)
            zero = none | (age >= tau)
            feat[:, 0] = np.where(zero, np.float32(0), np.where(age <= 0, np.float32(1), (1.0 - age / tau).astype(np.float32)))
            feat[:, 1] = np.where(zero, np.float32(0), pol)
    return feat, valid, mt[r:r + H, r:r + W].copy(), mp[r:r + H, r:r + W].copy()


def patches_bruteforce(rows, H, W, r, mode, tau=None, last_t=None, last_p=None):
    """For every entry of every patch, scan all earlier rows for the latest valid one at that pixel, and make the entry's two
    features on the spot, one scalar at a time: O(n^2), for n <= 2000.  No map is kept: the ones returned are built from the last
    row of every pixel."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n, P = len(rows), 2 * r + 1
    assert n <= 2000
    t0, p0 = _maps(H, W, last_t, last_p)
    bad = np.array([row_is_bad(e, H, W) for e in rows], dtype=bool)
    pix = np.where(bad, -1, rows[:, 2].astype(np.float64) * W + rows[:, 1].astype(np.float64))
    feat = np.empty((n, 2, P, P), dtype=np.float32)
    for i in range(n):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                f0, f1 = (np.float32(np.inf) if mode == "age" else np.float32(0)), np.float32(0)
                qx, qy = rows[i, 1] + dx, rows[i, 2] + dy
                if not bad[i] and 0 <= qx < W and 0 <= qy < H:
                    earlier = np.flatnonzero(pix[:i] == qy * W + qx)
                    if len(earlier):
                        tq, pq = rows[earlier[-1], 0], (1.0 if rows[earlier[-1], 3] > 0 else -1.0)
                    else:
                        tq, pq = t0[int(qy), int(qx)], float(p0[int(qy), int(qx)])
                    if tq != -np.inf:
                        a = np.float64(rows[i, 0]) - np.float64(tq)
                        if mode == "age":
                            with np.errstate(over="ignore"):
                                f0, f1 = np.float32(a), np.float32(pq)
                        elif a < tau:
                            f0, f1 = (np.float32(1) if a <= 0 else np.float32(np.float64(1) - a / np.float64(tau))), np.float32(pq)
                feat[i, 0, dy + r, dx + r], feat[i, 1, dy + r, dx + r] = f0, f1
    mt, mp = t0.copy(), p0.copy()
    for i in range(n):
        if not bad[i]:
            mt[int(rows[i, 2]), int(rows[i, 1])] = rows[i, 0]
            mp[int(rows[i, 2]), int(rows[i, 1])] = 1 if rows[i, 3] > 0 else -1
    return feat, ~bad, mt, mp
