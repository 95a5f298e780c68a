"""Tiled rows: an exact reference for inputs too large for the serial definitions (tests/denoise_ref.py, tests/patches_ref.py).

K copies of a small base case (denoise_ref.border_rows on an H0 x W0 sensor) are placed side by side on one wide sensor of
H0 x (K * (W0 + gap) - gap) pixels, with `gap` guard columns between neighbouring tiles; tile t adds t * (W0 + gap) to x.  The
tiles' rows are merged in a seeded random order that keeps each tile's own order.

A guard pixel never receives a row, so its carried time stays -inf: an infinite age for DenoiseSweep, a "none" patch entry for
EventPatches -- exactly what a neighbour outside the small sensor gives.  With gap >= the reach of the lookup (1 for DenoiseSweep,
the patch radius r for EventPatches) no row of one tile sees a pixel of another, every tile behaves as if alone, and the reference
of the big case is the small case's:
    histogram = K x the base histogram, n_bad = K x the base n_bad,
    mask, features and valid flag of a row = those of its base row (`base_index`),
    final maps = the base maps under each tile, -inf / 0 on the guard columns (`tile_map`).

One kind of bad row would turn valid when shifted: x == W0 lands on a guard column (or on the next tile).  Those rows get x = the
wide sensor's width instead.  The other kinds (NaN t, inf t, y = -1, x = 2.5) stay bad as they are.  tests/test_tiled_rows.py pins
all of this to the serial definitions at small K.  No GPU."""
import numpy as np


def wide_width(W0, K, gap):
    return K * (W0 + gap) - gap


def tile_rows(rows, labels, W0, K, gap, seed=1):
    """rows float32 [n,4] and labels bool [n] of the base case on a sensor W0 wide -> (wide rows float32 [K*n,4], their labels
    bool [K*n], base_index int64 [K*n]: the base row each wide row is a copy of, tile int64 [K*n]: the tile it lies in)."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 4)
    n = len(rows)
    assert K >= 1 and gap >= 1 and wide_width(W0, K, gap) + W0 < 1 << 23  # (x + 0.5 stays exact in float32)
    tile = np.random.RandomState(seed).permutation(np.repeat(np.arange(K, dtype=np.int64), n))
    base_index = np.empty(K * n, dtype=np.int64)
    base_index[np.argsort(tile, kind="stable")] = np.tile(np.arange(n, dtype=np.int64), K)  # each tile's rows keep their order
    wide = rows[base_index]
    wide[:, 1] += (tile * (W0 + gap)).astype(np.float32)
    wide[rows[base_index, 1] == W0, 1] = wide_width(W0, K, gap)
    return wide, np.asarray(labels, dtype=bool)[base_index], base_index, tile


def tile_map(base_map, K, gap, fill):
    """The final map of the wide sensor: base_map [H0,W0] under each tile, `fill` on the guard columns."""
    H0, W0 = base_map.shape
    out = np.full((H0, wide_width(W0, K, gap)), fill, dtype=base_map.dtype)
    for t in range(K):
        out[:, t * (W0 + gap):t * (W0 + gap) + W0] = base_map
    return out
