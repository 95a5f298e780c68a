"""tests/tiled_rows.py against the serial definitions: K tiles of a base case on one wide sensor give K times the base histogram,
every row the mask / features / valid flag of its base row, and the base maps under each tile.  The GPU tests of
tests/test_size_thresholds_gpu.py take their reference for half a million rows and more from these identities.  No GPU."""
import numpy as np
import pytest

from denoise_ref import BORDER_TAUS, border_rows, row_is_bad, stcf_serial
from patches_ref import patches_serial
from tiled_rows import tile_map, tile_rows, wide_width

H0, W0, N0 = 5, 7, 600


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_tiling_keeps_each_tiles_order_and_every_kind_of_bad_row():
    rows, labels = border_rows(H0, W0, N0)
    K, gap = 4, 3
    Ww = wide_width(W0, K, gap)
    wide, wlab, base, tile = tile_rows(rows, labels, W0, K, gap, seed=2)
    assert Ww == 37 and wide.shape == (K * N0, 4) and wide.dtype == np.float32
    for t in range(K):
        assert np.array_equal(base[tile == t], np.arange(N0))       # every tile holds the base rows, in their order
    assert (np.diff(tile) != 0).sum() > N0                           # and the tiles are interleaved
    assert np.array_equal(wlab, labels[base])
    assert np.array_equal(bits(wide[:, [0, 2, 3]]), bits(rows[base][:, [0, 2, 3]]))
    bad0 = np.array([row_is_bad(r, H0, W0) for r in rows])
    badw = np.array([row_is_bad(r, H0, Ww) for r in wide])
    assert np.array_equal(badw, bad0[base]) and bad0.sum() >= 10
    moved = rows[base, 1] == W0
    assert moved.sum() >= 2 * K and (wide[moved, 1] == Ww).all()
    good = ~badw
    assert np.array_equal(wide[good, 1], rows[base][good, 1] + tile[good] * (W0 + gap))
    guard = np.ones(Ww, bool)
    for t in range(K):
        guard[t * (W0 + gap):t * (W0 + gap) + W0] = False
    assert guard.sum() == (K - 1) * gap and not guard[wide[good, 1].astype(int)].any()  # no row ever lands on a guard column


@pytest.mark.parametrize("K", [3, 4])
def test_denoise_of_the_tiles_is_the_base_case(K):
    rows, labels = border_rows(H0, W0, N0)
    keep = (3, 2.0 ** -6)
    hist, n_bad, mask, last_t = stcf_serial(rows, H0, W0, BORDER_TAUS, labels, keep=keep)
    wide, wlab, base, _ = tile_rows(rows, labels, W0, K, 1, seed=K)
    w_hist, w_bad, w_mask, w_last = stcf_serial(wide, H0, wide_width(W0, K, 1), BORDER_TAUS, wlab, keep=keep)
    assert np.array_equal(w_hist, K * hist) and w_bad == K * n_bad and n_bad > 0 and 0 < mask.sum() < N0 - n_bad
    assert np.array_equal(w_mask, mask[base])
    assert np.array_equal(bits(w_last), bits(tile_map(last_t, K, 1, -np.inf)))


@pytest.mark.parametrize("mode,tau", [("age", None), ("linear", 2.0 ** -6)])
@pytest.mark.parametrize("K,r", [(3, 1), (4, 3)])
def test_patches_of_the_tiles_are_the_base_case(K, r, mode, tau):
    rows, labels = border_rows(H0, W0, N0)
    feat, valid, last_t, last_p = patches_serial(rows, H0, W0, r, mode, tau)
    wide, _, base, _ = tile_rows(rows, labels, W0, K, r, seed=K)
    w_feat, w_valid, w_t, w_p = patches_serial(wide, H0, wide_width(W0, K, r), r, mode, tau)
    assert np.array_equal(bits(w_feat), bits(feat[base])) and np.array_equal(w_valid, valid[base]) and not valid.all()
    assert np.array_equal(bits(w_t), bits(tile_map(last_t, K, r, -np.inf))) and np.array_equal(w_p, tile_map(last_p, K, r, 0))
    assert np.isfinite(feat[:, 0]).any() and (feat[:, 1] != 0).any()


def test_a_gap_too_narrow_for_the_patch_breaks_the_identity():
    """The guard columns are what the identities rest on: with gap 1 under r = 3 patches a tile sees its neighbour."""
    rows, labels = border_rows(H0, W0, N0)
    feat = patches_serial(rows, H0, W0, 3, "age")[0]
    wide, _, base, _ = tile_rows(rows, labels, W0, 3, 1)
    assert not np.array_equal(bits(patches_serial(wide, H0, wide_width(W0, 3, 1), 3, "age")[0]), bits(feat[base]))
