"""CPU-only: the numpy statement of DoubleWindowSweep's definition (tests/double_window_ref.py) against the double-window filter
applied directly per setting, what sets the filter apart from the fixed-window filter, DoubleWindowResult's arithmetic, the
argument checks of DoubleWindowSweep (all raised before the library or a device is touched), and the conditions of the inputs
tests/test_double_window_sweep_gpu.py runs on the GPU, pinned here with the reference alone."""
import numpy as np
import pytest
import torch

from double_window_ref import (BORDER_KEEPS, BORDER_LENGTHS, BORDER_SIGMAS, BORDER_SUPPORTS, FULL_BAD, FULL_H, FULL_KEEP, FULL_LENGTHS,
                               FULL_N, FULL_SIGMAS, FULL_SUPPORTS, FULL_W, XY_NONE, border_rows, burst_rows, dwf_bruteforce, dwf_serial,
                               full_window_rows, labels_from_counts, row_is_bad, window_words)
from window_filter_ref import fwf_bruteforce

H5, W7 = 5, 7


@pytest.fixture(scope="module")
def border():
    rows, labels = border_rows(H5, W7, 3000)
    return rows, labels, dwf_serial(rows, H5, W7, BORDER_LENGTHS, BORDER_SIGMAS, BORDER_SUPPORTS, labels)


@pytest.fixture(scope="module")
def full():
    rows, counts, n_signal = full_window_rows(FULL_H, FULL_W, FULL_N, FULL_BAD)
    labels = labels_from_counts(counts, n_signal)
    return rows, labels, dwf_serial(rows, FULL_H, FULL_W, FULL_LENGTHS, FULL_SIGMAS, FULL_SUPPORTS, labels, keep=FULL_KEEP)


def test_serial_reference_is_the_plain_loop(border):
    """All 60 settings of the border case: counts, totals, windows and the keep masks of the vectorised reference against the
    plain loop with two Python lists."""
    rows, labels, (passed, n_signal, n_noise, n_bad, mask, windows) = border
    valid = np.array([not row_is_bad(r, H5, W7) for r in rows])
    assert mask is None and n_bad == int((~valid).sum()) and n_bad > 5
    assert (n_signal, n_noise) == (int((valid & labels).sum()), int((valid & ~labels).sum()))
    assert passed.shape == (4, 3, 5, 2) and passed.dtype == np.int64 and windows.shape == (4, 3, 5, 2, 8) and windows.dtype == np.int64
    partly = 0
    for ki, k in enumerate(BORDER_SUPPORTS):
        for s, sigma in enumerate(BORDER_SIGMAS):
            for li, L in enumerate(BORDER_LENGTHS):
                p, v, R, N = dwf_bruteforce(rows, H5, W7, L, sigma, k)
                assert np.array_equal(v, valid) and not p[~valid].any()
                assert passed[ki, s, li].tolist() == [int((p & ~labels).sum()), int((p & labels).sum())]
                assert np.array_equal(windows[ki, s, li, 0], window_words(R, 8)) and np.array_equal(windows[ki, s, li, 1], window_words(N, 8))
                assert (windows[ki, s, li] == XY_NONE).sum(axis=1).min() >= 8 - L
                partly += 0 < p.sum() < valid.sum()
    assert partly >= 30  # (38 here) settings that pass some valid rows but not all
    for keep in BORDER_KEEPS:
        got = dwf_serial(rows, H5, W7, BORDER_LENGTHS, BORDER_SIGMAS, BORDER_SUPPORTS, labels, keep=keep)
        assert np.array_equal(got[4], dwf_bruteforce(rows, H5, W7, *keep)[0]) and np.array_equal(got[0], passed)


def test_reference_is_cut_invariant(border):
    rows, labels, whole = border
    keep = BORDER_KEEPS[1]
    whole_mask = dwf_serial(rows, H5, W7, BORDER_LENGTHS, BORDER_SIGMAS, BORDER_SUPPORTS, labels, keep=keep)[4]
    passed, n_signal, n_noise, n_bad, masks, windows = 0, 0, 0, 0, [], None
    for a, b in ((0, 1), (1, 1777), (1777, 1777), (1777, 3000)):
        p, ns, nn, nb, mk, windows = dwf_serial(rows[a:b], H5, W7, BORDER_LENGTHS, BORDER_SIGMAS, BORDER_SUPPORTS, labels[a:b],
                                                windows=windows, keep=keep)
        passed, n_signal, n_noise, n_bad = passed + p, n_signal + ns, n_noise + nn, n_bad + nb
        masks.append(mk)
    assert np.array_equal(passed, whole[0]) and (n_signal, n_noise, n_bad) == whole[1:4]
    assert np.array_equal(np.concatenate(masks), whole_mask) and np.array_equal(windows, whole[5])


def test_border_keeps_are_neither_fixed_window_filter(border):
    """The keep settings of the GPU test differ from FWF(L) and from FWF(2 L), the filter of the same memory, on some rows."""
    rows, labels, _ = border
    differ = {}
    for keep in BORDER_KEEPS:
        L, sigma, k = keep
        p = dwf_bruteforce(rows, H5, W7, L, sigma, k)[0]
        differ[keep] = tuple(int((p != fwf_bruteforce(rows, H5, W7, length, sigma, k)[0]).sum()) for length in (L, 2 * L))
        assert min(differ[keep]) >= 1 and 0 < p.sum() < len(p)
    assert differ == {(3, 1, 1): (630, 282), (8, 1, 3): (739, 465)}


def test_full_window_rows_wrap_both_windows(full):
    """6000 rows at 33x37, 250 of them bad: for every length the sigma-0, k = 1 setting has pushed more than L rows into each of
    its windows, and the keep mask keeps some rows and drops others."""
    rows, labels, (passed, n_signal, n_noise, n_bad, mask, windows) = full
    assert rows.shape == (FULL_N, 4) and n_bad == FULL_BAD and n_signal + n_noise == FULL_N - FULL_BAD and n_signal > 0 and n_noise > 0
    for li, L in enumerate(FULL_LENGTHS):
        into_r = int(passed[0, 0, li].sum())
        into_n = FULL_N - FULL_BAD - into_r
        assert into_r > L and into_n > L
        assert not (windows[0, 0, li, :, 512 - L:] == XY_NONE).any() and (windows[0, 0, li, :, :512 - L] == XY_NONE).all()
    assert (int(passed[0, 0, 5].sum()), FULL_N - FULL_BAD - int(passed[0, 0, 5].sum())) == (3467, 2283)
    assert (int(passed[0, 0, 0].sum()), FULL_N - FULL_BAD - int(passed[0, 0, 0].sum())) == (219, 5531)
    valid = np.array([not row_is_bad(r, FULL_H, FULL_W) for r in rows])
    assert mask.any() and not mask[valid].all() and not mask[~valid].any()
    # one long setting against the plain loop
    p, v, R, N = dwf_bruteforce(rows, FULL_H, FULL_W, 129, 2, 2)
    assert passed[1, 1, 4].tolist() == [int((p & ~labels).sum()), int((p & labels).sum())]
    assert np.array_equal(windows[1, 1, 4, 0], window_words(R, 512)) and np.array_equal(windows[1, 1, 4, 1], window_words(N, 512))


def test_a_noise_burst_does_not_flush_the_real_window():
    """The property that defines the filter: after nine isolated rows DWF(4) still remembers the pixel before them; FWF(4) and
    FWF(8), the filter of the same memory, have forgotten it."""
    rows = burst_rows()
    xy = rows[:, 1:3].astype(int)
    for j in range(3, 12):  # at least 3 apart from everything else
        assert min(abs(xy[j] - xy[i]).sum() for i in range(13) if i != j) >= 3
    p, v, R, N = dwf_bruteforce(rows, 64, 64, 4, 1, 1)
    assert v.all() and p.tolist() == [False, True, True] + [False] * 9 + [True]
    assert R == [(10, 10), (10, 10), (11, 10)] and len(N) == 4
    assert not fwf_bruteforce(rows, 64, 64, 4, 1, 1)[0][12] and not fwf_bruteforce(rows, 64, 64, 8, 1, 1)[0][12]
    got = dwf_serial(rows, 64, 64, [4], [1], [1], keep=(4, 1, 1))
    assert got[4].tolist() == p.tolist() and got[0].tolist() == [[[[0, 3]]]]


def test_closed_form_on_one_pixel():
    """A 1x1 sensor, 300 rows: (L, 0, k) fails every row if L < k (N never holds k rows and R stays empty), else exactly the first
    k rows (N holds k rows from then on)."""
    rows = np.zeros((300, 4), dtype=np.float32)
    lengths, supports = (1, 2, 3, 4, 7), (1, 2, 3, 4)
    passed = dwf_serial(rows, 1, 1, lengths, [0], supports)[0]
    for ki, k in enumerate(supports):
        for li, L in enumerate(lengths):
            assert passed[ki, 0, li].tolist() == [0, 0 if L < k else 300 - k]
            assert int(dwf_bruteforce(rows, 1, 1, L, 0, k)[0].sum()) == (0 if L < k else 300 - k)


def test_result_arithmetic_on_hand_written_counts():
    from v2e_amd import DoubleWindowResult
    lengths, sigmas, supports = [2, 8, 32], [0, 3], [1, 3]
    passed = np.zeros((2, 2, 3, 2), dtype=np.int64)
    passed[0, 0, :, 1], passed[0, 0, :, 0] = [2, 5, 9], [1, 1, 2]      # k = 1, sigma 0
    passed[1, 1, :, 1], passed[1, 1, :, 0] = [1, 2, 5], [0, 0, 1]      # k = 3, sigma 3
    r = DoubleWindowResult(passed, lengths, sigmas, supports, n_signal=10, n_noise=4, n_bad=7)
    assert (r.n_signal, r.n_noise, r.n_bad) == (10, 4, 7) and r.passed.dtype == np.int64 and r.passed.shape == (2, 2, 3, 2)
    assert r.lengths.dtype == np.int64 and r.sigmas.dtype == np.int64 and r.supports.dtype == np.int64
    assert r.tpr.shape == (2, 2, 3) and r.fpr.shape == (2, 2, 3) and r.tpr.dtype == np.float64
    assert np.array_equal(r.tpr[0, 0], np.array([2, 5, 9]) / 10) and np.array_equal(r.fpr[0, 0], np.array([1, 1, 2]) / 4)
    # tpr - fpr: (k 1, sigma 0): -0.05, 0.25, 0.4; (k 3, sigma 3): 0.1, 0.2, 0.25; the rest 0
    assert r.best() == (32, 0, 1, 0.9, 0.5)
    # the first maximum in (k, sigma, L) order, and the k of the table, not its index
    tie = np.zeros((2, 2, 2, 2), dtype=np.int64)
    tie[1, 0, 1, 1] = tie[1, 1, 0, 1] = 5
    assert DoubleWindowResult(tie, [3, 9], [1, 2], [2, 4], n_signal=5, n_noise=5).best() == (9, 1, 4, 1.0, 0.0)
    # NaN where the denominator is 0
    r = DoubleWindowResult(np.ones((2, 2, 2, 2), dtype=np.int64), [3, 9], [1, 2], [2, 4], n_signal=1, n_noise=0)
    assert np.isnan(r.fpr).all() and np.array_equal(r.tpr, np.ones((2, 2, 2)))
    with pytest.raises(ValueError):
        r.best()
    r = DoubleWindowResult(np.zeros((2, 2, 2, 2), dtype=np.int64), [3, 9], [1, 2], [2, 4], n_signal=0, n_noise=3)
    assert np.isnan(r.tpr).all() and not r.fpr.any()
    with pytest.raises(ValueError):
        DoubleWindowResult(np.zeros((2, 2, 2, 2), dtype=np.int64), [1, 2, 3], [1, 2], [2, 4], 0, 0)
    with pytest.raises(ValueError):
        DoubleWindowResult(np.zeros((2, 2, 2, 2), dtype=np.int64), [1, 2], [1, 2], [1, 2, 4], 0, 0)


@pytest.mark.parametrize("lengths", [[], list(range(1, 66)), [4, 4], [5, 4], [0, 1], [1, 513], [1.5, 2], [float("nan")], ["a"]])
def test_constructor_refuses_bad_length_tables(lengths):
    from v2e_amd import DoubleWindowSweep
    with pytest.raises(ValueError, match="DoubleWindowSweep: "):
        DoubleWindowSweep(4, 4, lengths, [1])


@pytest.mark.parametrize("sigmas", [[], list(range(9)), [2, 2], [3, 2], [-1, 1], [1, 65536], [0.5], [float("inf")]])
def test_constructor_refuses_bad_sigma_tables(sigmas):
    from v2e_amd import DoubleWindowSweep
    with pytest.raises(ValueError, match="DoubleWindowSweep: "):
        DoubleWindowSweep(4, 4, [1, 2], sigmas)


@pytest.mark.parametrize("supports", [[], [1, 2, 3, 4, 5], [2, 2], [3, 2], [0, 1], [5], [1.5], [float("nan")], ["k"]])
def test_constructor_refuses_bad_support_tables(supports):
    from v2e_amd import DoubleWindowSweep
    with pytest.raises(ValueError, match="DoubleWindowSweep: "):
        DoubleWindowSweep(4, 4, [1, 2], [1], supports)


def test_constructor_and_add_run_argument_checks(monkeypatch):
    from v2e_amd import DoubleWindowSweep, _capi

    def touched(*a, **k):
        raise AssertionError("the library or the device was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)
    monkeypatch.setattr(_capi, "require_gpu", touched)
    for bad in (dict(height=0), dict(width=0), dict(height=65536), dict(width=65536), dict(max_rows_per_pass=0),
                dict(max_rows_per_pass=(1 << 30) + 1)):
        kw = dict(height=4, width=4, lengths=[1, 2], sigmas=[0, 1])
        kw.update(bad)
        with pytest.raises(ValueError):
            DoubleWindowSweep(**kw)
    big = DoubleWindowSweep(65535, 65535, [512], [65535], [4])  # the limits themselves are allowed
    assert (big.height, big.width, big.max_length, big.n_settings) == (65535, 65535, 512, 1)
    ws = DoubleWindowSweep(4, 6, np.arange(1, 65) * 8, range(8), max_rows_per_pass=1)  # 64 lengths up to 512, 8 sigmas, one-row passes
    assert (ws.height, ws.width, len(ws.lengths), len(ws.sigmas), ws.max_length, ws.lengths.dtype) == (4, 6, 64, 8, 512, np.int64)
    assert ws.supports.tolist() == [1, 2, 3, 4] and ws.n_settings == 2048
    default = DoubleWindowSweep(4, 6, [1], [1]).max_rows_per_pass
    assert default & (default - 1) == 0 and default < 1 << 25  # a power of two below the other sweeps' default
    rows = torch.zeros((6, 4), dtype=torch.float32)
    lab = torch.ones(6, dtype=torch.bool)
    cases = [
        dict(labels=lab, counts=[6], n_signal=[3]),        # both label sources
        dict(n_signal=[3]),                                # n_signal without counts
        dict(counts=[3, 3], n_signal=[3]),                 # lengths
        dict(counts=[3, 3], n_signal=[3, 4]),              # more signal rows than rows
        dict(counts=[3, 2], n_signal=[1, 1]),              # counts do not cover the rows
        dict(labels=torch.ones(5, dtype=torch.bool)),      # one label per row
        dict(labels=torch.ones(6, dtype=torch.uint8)),     # bool
        dict(keep=(0, 1, 1)), dict(keep=(513, 1, 1)), dict(keep=(1.5, 1, 1)), dict(keep=(8, -1, 1)), dict(keep=(8, 0.5, 1)),
        dict(keep=(8, 1, 0)), dict(keep=(8, 1, 5)), dict(keep=(8, 1, 1.5)), dict(keep=(8, 1)), dict(keep=3),
        dict(keep=(8, float("nan"), 1)),
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            ws.add_run(rows, **kw)
    # a keep that is a valid filter but no entry of the tables: the offending value is named
    few = DoubleWindowSweep(4, 6, [2, 8], [1, 3], [1, 4])
    for keep, name, value in (((4, 1, 1), "L", 4), ((8, 2, 1), "sigma", 2), ((8, 3, 2), "k", 2)):
        with pytest.raises(ValueError, match="keep's %s must be an entry of the sweep's table, got %d" % (name, value)):
            few.add_run(rows, keep=keep)
    with pytest.raises(ValueError):  # the keep check comes first, as in WindowSweep.add_run
        few.add_run(torch.zeros((6, 3)), keep=(4, 1, 1))
    for r in (torch.zeros((6, 3)), torch.zeros((6, 4), dtype=torch.float64), torch.zeros((24,))):
        with pytest.raises(ValueError):
            ws.add_run(r)
    with pytest.raises(TypeError):  # host rows: the run's rows are a device tensor
        ws.add_run(rows, keep=(8, 1, 1))
    with pytest.raises(TypeError):
        ws.add_run(np.zeros((6, 4), np.float32))
    ws.reset()  # nothing allocated yet: nothing to do


def test_needs_a_gpu_and_says_so(monkeypatch):
    from v2e_amd import DoubleWindowSweep, V2EAmdError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(V2EAmdError, match="DoubleWindowSweep needs a ROCm GPU"):
        DoubleWindowSweep(4, 4, [1, 2], [1]).result()


def test_exports_and_entry_points():
    import v2e_amd
    from v2e_amd import _capi
    assert "DoubleWindowSweep" in v2e_amd.__all__ and "DoubleWindowResult" in v2e_amd.__all__
    assert v2e_amd.DoubleWindowSweep is v2e_amd.dwindow.DoubleWindowSweep
    for name, n_args in (("v2e_dwindow_labels", 10), ("v2e_dwindow_sweep", 19)):
        assert len(_capi.SIGNATURES[name][1]) == n_args and hasattr(_capi.lib(), name)
