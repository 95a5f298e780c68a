"""Two numpy statements of EventStats' definition (v2e_amd/stats.py) and the rows the tests share.  No GPU.

Rows are float32 [n,4] = (t, x = column, y = row, p), taken in row order.  A row is bad if t is not finite or x / y is not an integer
value inside [0,W) / [0,H): it is counted in n_bad and touches nothing.  A valid row is ON iff p > 0.  labels: bool [n] (True =
signal, label 1) or None (all signal).
  count[label, pol, y, x] += 1 for every valid row (pol 0 = OFF, 1 = ON), whatever roi and bounds are.
  roi = ((x0, x1), (y0, y1)) inclusive; everything below counts valid rows inside it only; the maps are stamped by every valid row.
  The previous event of row i is the latest valid row j < i at the same pixel, else the carried last_t (float32, -inf: none) /
  last_p (int8 +-1, 0: none).  None: n_first[label, pol] += 1.  Otherwise d = float64(t_i) - float64(T_prev), kept when negative,
  tr = 2 * (previous ON) + (this ON), isi_hist[label, tr, searchsorted(edges, d, 'right')] += 1; d < 0: n_backwards[label] += 1;
  min_isi[label, tr] = the smallest d >= 0 (+inf where none).
  bounds (K + 1 ascending float64) or None: k = searchsorted(bounds, float64(t), 'right') - 1; time_hist[label, pol, k] += 1 for
  0 <= k < K, else n_before += 1 (k < 0) or n_after += 1.
  t_first / t_last: the smallest / largest t of the valid rows (float32 values), None without one.
`stats_loop` is the definition: a plain loop in row order with dict maps.  `stats_vectorised` is the same sums from a stable sort by
pixel, for the large cases.  Both return the same dict (KEYS), the maps after the rows included."""
import numpy as np

from denoise_ref import row_is_bad

KEYS = ("count", "isi_hist", "time_hist", "n_first", "n_backwards", "n_before", "n_after", "min_isi", "t_first", "t_last", "n_bad",
        "last_t", "last_p")


def _empty(H, W, E, K):
    return {"count": np.zeros((2, 2, H, W), np.int64), "isi_hist": np.zeros((2, 4, E + 1), np.int64),
            "time_hist": None if K is None else np.zeros((2, 2, K), np.int64), "n_first": np.zeros((2, 2), np.int64),
            "n_backwards": np.zeros(2, np.int64), "n_before": 0, "n_after": 0, "min_isi": np.full((2, 4), np.inf), "t_first": None,
            "t_last": None, "n_bad": 0}


def _args(rows, H, W, edges, bounds, roi, labels):
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    edges = np.asarray(edges, dtype=np.float64)
    bounds = None if bounds is None else np.asarray(bounds, dtype=np.float64)
    roi = ((0, W - 1), (0, H - 1)) if roi is None else roi
    lab = np.ones(len(rows), np.int64) if labels is None else np.asarray(labels).astype(bool).astype(np.int64)
    return rows, edges, bounds, roi, lab


def stats_loop(rows, H, W, edges, bounds=None, roi=None, labels=None, last_t=None, last_p=None):
    rows, edges, bounds, ((x0, x1), (y0, y1)), lab = _args(rows, H, W, edges, bounds, roi, labels)
    out = _empty(H, W, len(edges), None if bounds is None else len(bounds) - 1)
    prev = {}  # pixel -> (float32 t, ON)
    if last_t is not None:
        for y in range(H):
            for x in range(W):
                if last_t[y, x] != -np.inf:
                    prev[x, y] = (np.float32(last_t[y, x]), int(last_p[y, x] > 0))
    for i in range(len(rows)):
        if row_is_bad(rows[i], H, W):
            out["n_bad"] += 1
            continue
        t, x, y, on, l = rows[i, 0], int(rows[i, 1]), int(rows[i, 2]), int(rows[i, 3] > 0), int(lab[i])
        out["count"][l, on, y, x] += 1
        out["t_first"] = float(t) if out["t_first"] is None else min(out["t_first"], float(t))
        out["t_last"] = float(t) if out["t_last"] is None else max(out["t_last"], float(t))
        before = prev.get((x, y))
        prev[x, y] = (t, on)
        if not (x0 <= x <= x1 and y0 <= y <= y1):
            continue
        if bounds is not None:
            k = int(np.searchsorted(bounds, np.float64(t), side="right")) - 1
            if k < 0:
                out["n_before"] += 1
            elif k >= len(bounds) - 1:
                out["n_after"] += 1
            else:
                out["time_hist"][l, on, k] += 1
        if before is None:
            out["n_first"][l, on] += 1
            continue
        d = np.float64(t) - np.float64(before[0])
        tr = 2 * before[1] + on
        out["isi_hist"][l, tr, int(np.searchsorted(edges, d, side="right"))] += 1
        if d < 0:
            out["n_backwards"][l] += 1
        else:
            out["min_isi"][l, tr] = min(out["min_isi"][l, tr], d)
    m_t = np.full((H, W), -np.inf, np.float32) if last_t is None else np.array(last_t, dtype=np.float32)
    m_p = np.zeros((H, W), np.int8) if last_p is None else np.array(last_p, dtype=np.int8)
    for (x, y), (t, on) in prev.items():
        m_t[y, x], m_p[y, x] = t, 1 if on else -1
    out["last_t"], out["last_p"] = m_t, m_p
    return out


def stats_vectorised(rows, H, W, edges, bounds=None, roi=None, labels=None, last_t=None, last_p=None):
    rows, edges, bounds, ((x0, x1), (y0, y1)), lab = _args(rows, H, W, edges, bounds, roi, labels)
    out = _empty(H, W, len(edges), None if bounds is None else len(bounds) - 1)
    m_t = np.full((H, W), -np.inf, np.float32) if last_t is None else np.array(last_t, dtype=np.float32)
    m_p = np.zeros((H, W), np.int8) if last_p is None else np.array(last_p, dtype=np.int8)
    t, x, y = rows[:, 0], rows[:, 1], rows[:, 2]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(t) & (x == np.floor(x)) & (y == np.floor(y)) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    out["n_bad"] = int((~valid).sum())
    idx = np.flatnonzero(valid)
    if len(idx):
        t, on, l = t[idx], (rows[idx, 3] > 0).astype(np.int64), lab[idx]
        x, y = x[idx].astype(np.int64), y[idx].astype(np.int64)
        np.add.at(out["count"], (l, on, y, x), 1)
        out["t_first"], out["t_last"] = float(t.min()), float(t.max())
        pix = y * W + x
        order = np.argsort(pix, kind="stable")          # a pixel's rows together, in row order
        sp = pix[order]
        follows = np.concatenate([[False], sp[1:] == sp[:-1]])   # the row before it in this order is its previous event
        before = np.concatenate([[0], order[:-1]])
        t_prev = np.where(follows, t[before], m_t.reshape(-1)[sp])
        on_prev = np.where(follows, on[before], m_p.reshape(-1)[sp] > 0).astype(np.int64)
        ts, ons, ls = t[order], on[order], l[order]
        inside = (x[order] >= x0) & (x[order] <= x1) & (y[order] >= y0) & (y[order] <= y1)
        if bounds is not None:
            K = len(bounds) - 1
            k = np.searchsorted(bounds, ts.astype(np.float64), side="right") - 1
            out["n_before"] = int((inside & (k < 0)).sum())
            out["n_after"] = int((inside & (k >= K)).sum())
            ok = inside & (k >= 0) & (k < K)
            np.add.at(out["time_hist"], (ls[ok], ons[ok], k[ok]), 1)
        none = t_prev == -np.inf
        first = inside & none
        np.add.at(out["n_first"], (ls[first], ons[first]), 1)
        has = inside & ~none
        d = ts[has].astype(np.float64) - t_prev[has].astype(np.float64)
        tr = 2 * on_prev[has] + ons[has]
        np.add.at(out["isi_hist"], (ls[has], tr, np.searchsorted(edges, d, side="right")), 1)
        np.add.at(out["n_backwards"], ls[has][d < 0], 1)
        np.minimum.at(out["min_isi"], (ls[has][d >= 0], tr[d >= 0]), d[d >= 0])
        last = np.concatenate([sp[1:] != sp[:-1], [True]])      # each pixel's last row stamps the maps
        m_t.reshape(-1)[sp[last]] = ts[last]
        m_p.reshape(-1)[sp[last]] = np.where(ons[last] > 0, 1, -1)
    out["last_t"], out["last_p"] = m_t, m_p
    return out


def same(a, b, keys=KEYS):
    """Every entry of two reference dicts (or of one and result_dict's) equal: arrays exactly (inf as a value), scalars by value."""
    for k in keys:
        u, v = a[k], b[k]
        if u is None or v is None:
            if u is not v:
                return False
        elif not np.array_equal(np.asarray(u), np.asarray(v)):
            return False
    return True


def result_dict(res, last_t=None, last_p=None):
    """An EventStatsResult (and the maps, where given) as the dict the references return."""
    out = {k: getattr(res, k) for k in KEYS[:-2]}
    out["last_t"], out["last_p"] = last_t, last_p
    return out


def stats_rows(H, W, n, seed=11, bad=0.05, unit=2.0 ** -10, backwards=0.05, hot=0.0):
    """Random rows with duplicates: times are multiples of `unit` (intervals exact, many on an edge) that advance by 0 .. 3 units, a
    share of them out of order (up to 40 units back); `bad` of the rows are bad (NaN t, inf t, x = W, y = -1, x = 2.5 in turn); p is
    drawn from {1, -1, 0, 0.5}, mostly +-1; `hot` of the rows lie on the 3 x 3 pixels at the sensor's middle, so that a pixel's
    previous event is often a later one.  Returns (rows float32 [n,4], labels bool [n])."""
    rng = np.random.RandomState(seed)
    t = np.cumsum(rng.randint(0, 4, size=n)).astype(np.float64)
    late = rng.rand(n) < backwards
    t[late] -= rng.randint(1, 41, size=int(late.sum()))
    p = rng.choice([1.0, -1.0, 0.0, 0.5], size=n, p=[0.45, 0.45, 0.05, 0.05])
    rows = np.stack([t * unit, rng.randint(0, W, size=n), rng.randint(0, H, size=n), p], axis=1).astype(np.float32)
    if hot > 0:
        rng_hot = np.random.RandomState(seed + 1000)
        on_hot = rng_hot.rand(n) < hot
        rows[on_hot, 1] = W // 2 + rng_hot.randint(-1, 2, size=int(on_hot.sum()))
        rows[on_hot, 2] = H // 2 + rng_hot.randint(-1, 2, size=int(on_hot.sum()))
    for j, i in enumerate(np.flatnonzero(rng.rand(n) < bad)):
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
    return rows, rng.rand(n) < 0.6


def pearson(a, b):
    """Pearson r written out: sum((a - ma)(b - mb)) / sqrt(sum((a - ma)^2) sum((b - mb)^2)); NaN where a side is constant."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    da, db = a - a.mean(), b - b.mean()
    den = np.sqrt((da ** 2).sum() * (db ** 2).sum())
    return float("nan") if den == 0 else float((da * db).sum() / den)


def jsd(p, q):
    """Jensen-Shannon divergence in base 2 of two count vectors, written out with a loop."""
    p, q = np.asarray(p, np.float64).reshape(-1), np.asarray(q, np.float64).reshape(-1)
    p, q = p / p.sum(), q / q.sum()
    total = 0.0
    for pi, qi in zip(p, q):
        mi = 0.5 * (pi + qi)
        if pi > 0:
            total += 0.5 * pi * np.log2(pi / mi)
        if qi > 0:
            total += 0.5 * qi * np.log2(qi / mi)
    return float(total)
