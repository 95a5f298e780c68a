"""CPU-only: the numpy statement of WindowSweep's definition (tests/window_filter_ref.py) against the fixed-window filter applied
directly per setting, WindowResult's arithmetic, the argument checks of WindowSweep (all raised before the library or a device is
touched), and the conditions of the inputs tests/test_window_sweep_gpu.py runs on the GPU, pinned here with the reference alone."""
import os

import numpy as np
import pytest
import torch

from denoise_ref import NOISY_DOT_RATE_HZ
from window_filter_ref import (BORDER_KEEPS, BORDER_LENGTHS, BORDER_SIGMAS, CLIP_FRAMES, CLIP_KEEP, CLIP_LENGTHS, CLIP_SIGMAS, FULL_LENGTHS,
                               FULL_SIGMAS, XY_NONE, border_rows, full_window_rows, fwf_bruteforce, fwf_serial, labels_from_counts,
                               row_is_bad)


def test_depth_histogram_is_the_filter():
    """400 rows at 5x7 with bad rows: the cumulative histogram of the reference, and its keep masks, against FWF(L, sigma, k)
    applied directly for every setting of the tables and for keep settings outside them."""
    rows, labels = border_rows(n=400, seed=11)
    H, W = 5, 7
    lengths, sigmas = (1, 2, 3, 5, 8, 20), (0, 1, 3)
    hist, n_bad, _, tail = fwf_serial(rows, H, W, lengths, sigmas, labels)
    valid = np.array([not row_is_bad(r, H, W) for r in rows])
    assert n_bad == int((~valid).sum()) and n_bad > 5
    passed = np.cumsum(hist[:, :, :, :-1], axis=3)
    for li, L in enumerate(lengths):
        for s, sigma in enumerate(sigmas):
            for k in range(1, 5):
                p, v = fwf_bruteforce(rows, H, W, L, sigma, k)
                assert np.array_equal(v, valid)
                assert passed[k - 1, s, 1, li] == int((p & labels).sum()) and passed[k - 1, s, 0, li] == int((p & ~labels).sum())
    for keep in ((4, 2, 2), (20, 0, 4), (1, 100, 1), (7, 1, 3)):
        mask = fwf_serial(rows, H, W, lengths, sigmas, labels, keep=keep)[2]
        assert np.array_equal(mask, fwf_bruteforce(rows, H, W, *keep)[0]) and not mask[~valid].any()
    # the tail: the last 20 valid rows, the latest last
    good = rows[valid]
    assert tail.dtype == np.int64 and tail.tolist() == [int(r[1]) | (int(r[2]) << 16) for r in good[-20:]]


def test_reference_is_cut_invariant_and_carries_no_row_yet_words():
    rows, labels = border_rows(n=900, seed=5)
    lengths, sigmas, keep = (1, 4, 1024), (0, 2), (600, 1, 2)
    whole = fwf_serial(rows, 5, 7, lengths, sigmas, labels, keep=keep)
    hist, n_bad, masks, tail = 0, 0, [], None
    for a, b in ((0, 1), (1, 500), (500, 500), (500, 900)):
        h, nb, mk, tail = fwf_serial(rows[a:b], 5, 7, lengths, sigmas, labels[a:b], tail=tail, keep=keep)
        assert len(tail) == 1024
        hist, n_bad = hist + h, n_bad + nb
        masks.append(mk)
    assert np.array_equal(hist, whole[0]) and n_bad == whole[1] and np.array_equal(np.concatenate(masks), whole[2])
    assert np.array_equal(tail, whole[3]) and (tail == XY_NONE).sum() == 1024 - (900 - n_bad)
    assert whole[2].any()


def test_border_rows_hold_what_the_gpu_test_needs():
    rows, labels = border_rows()
    H, W = 5, 7
    assert rows.shape == (3000, 4) and rows.dtype == np.float32 and labels.shape == (3000,)
    bad = np.array([row_is_bad(r, H, W) for r in rows])
    assert 100 <= bad.sum() <= 140
    assert np.isnan(rows[:, 0]).any() and (rows[:, 1] != np.floor(rows[:, 1])).any() and (rows[:, 2] == H).any() and (rows[:, 1] == -1).any()
    hist, n_bad, _, _ = fwf_serial(rows, H, W, BORDER_LENGTHS, BORDER_SIGMAS, labels)
    assert n_bad == bad.sum()
    assert hist[0, :, :, 0].min() > 0                      # k = 1: every (s, label) has rows in bin 0
    assert hist[:, :, :, -1].min() > 0                     # every (k, s, label) has rows that pass no length
    for k in range(2, 5):
        assert not hist[k - 1, :, :, :k - 1].any()         # depth >= k
    assert all(hist[k, s].sum() == 3000 - n_bad for k in range(4) for s in range(len(BORDER_SIGMAS)))
    for keep in BORDER_KEEPS:
        mask = fwf_serial(rows, H, W, BORDER_LENGTHS, BORDER_SIGMAS, labels, keep=keep)[2]
        assert 300 < mask.sum() < 2500


def test_full_window_rows_hold_what_the_gpu_test_needs():
    assert len(FULL_LENGTHS) == 52 and FULL_LENGTHS[0] == 1 and FULL_LENGTHS[-1] == 1024 and np.all(np.diff(FULL_LENGTHS) > 0)
    rows, counts, n_signal = full_window_rows()
    assert rows.shape == (12000, 4) and counts.sum() == 12000 and np.all(n_signal <= counts)
    bad = np.array([row_is_bad(r, 33, 37) for r in rows])
    assert bad.sum() == 500 and bad[:256].any() and bad[-256:].any()
    hist, n_bad, _, _ = fwf_serial(rows, 33, 37, FULL_LENGTHS, FULL_SIGMAS, labels_from_counts(counts, n_signal))
    populated = (hist.sum(axis=2) > 0).sum(axis=2)
    assert n_bad == 500 and populated.shape == (4, 8) and populated.min() >= 30


def test_result_arithmetic_on_a_hand_written_histogram():
    from v2e_amd import WindowResult
    lengths, sigmas = [2, 8, 32], [0, 3]
    hist = np.zeros((4, 2, 2, 4), dtype=np.int64)
    hist[:, :, 1, 3], hist[:, :, 0, 3] = 10, 4           # everything passes no length ...
    hist[0, 0, 1] = [2, 3, 4, 1]                         # ... but k = 1, sigma 0: signal
    hist[0, 0, 0] = [1, 0, 1, 2]                         #                           noise
    hist[1, 1, 1] = [1, 1, 3, 5]                         # k = 2, sigma 3
    hist[1, 1, 0] = [0, 0, 1, 3]
    r = WindowResult(hist, lengths, sigmas, n_bad=7)
    assert (r.n_signal, r.n_noise, r.n_bad) == (10, 4, 7) and r.hist.dtype == np.int64
    assert r.lengths.dtype == np.int64 and r.sigmas.dtype == np.int64
    assert r.passed.shape == (4, 2, 2, 3) and r.passed.dtype == np.int64
    assert r.passed[0, 0].tolist() == [[1, 1, 2], [2, 5, 9]] and r.passed[1, 1].tolist() == [[0, 0, 1], [1, 2, 5]]
    assert r.passed.sum() == 2 + 1 + 1 + 2 + 5 + 9 + 1 + 1 + 2 + 5
    assert r.tpr.shape == (4, 2, 3) and r.fpr.shape == (4, 2, 3) and r.tpr.dtype == np.float64
    assert np.array_equal(r.tpr[0, 0], np.array([2, 5, 9]) / 10) and np.array_equal(r.fpr[0, 0], np.array([1, 1, 2]) / 4)
    # tpr - fpr: (k 1, sigma 0): -0.05, 0.25, 0.4; (k 2, sigma 3): 0.1, 0.2, 0.25; the rest 0
    assert r.best() == (32, 0, 1, 0.9, 0.5)
    # the first maximum in (k, sigma, L) order
    tie = np.zeros((4, 2, 2, 3), dtype=np.int64)
    tie[:, :, 1, 2], tie[:, :, 0, 2] = 5, 5
    tie[2, 1, 1] = [0, 5, 0]
    tie[2, 0, 1] = [0, 5, 0]
    tie[3, 0, 1] = [5, 0, 0]
    assert WindowResult(tie, [3, 9], [1, 2]).best() == (9, 1, 3, 1.0, 0.0)
    # NaN where the denominator is 0
    only_signal = np.zeros((4, 2, 2, 3), dtype=np.int64)
    only_signal[:, :, 1, 0] = 3
    r = WindowResult(only_signal, [3, 9], [1, 2])
    assert np.isnan(r.fpr).all() and np.array_equal(r.tpr, np.ones((4, 2, 2)))
    with pytest.raises(ValueError):
        r.best()
    with pytest.raises(ValueError):
        WindowResult(np.zeros((4, 2, 2, 3), dtype=np.int64), [1, 2, 3], [1, 2])
    with pytest.raises(ValueError):
        WindowResult(np.zeros((4, 2, 2, 3), dtype=np.int64), [1, 2], [1, 2, 3])


@pytest.mark.parametrize("lengths", [[], list(range(1, 66)), [4, 4], [5, 4], [0, 1], [1, 1025], [1.5, 2], [float("nan")], ["a"]])
def test_constructor_refuses_bad_length_tables(lengths):
    from v2e_amd import WindowSweep
    with pytest.raises(ValueError):
        WindowSweep(4, 4, lengths, [1])


@pytest.mark.parametrize("sigmas", [[], list(range(9)), [2, 2], [3, 2], [-1, 1], [1, 65536], [0.5], [float("inf")]])
def test_constructor_refuses_bad_sigma_tables(sigmas):
    from v2e_amd import WindowSweep
    with pytest.raises(ValueError):
        WindowSweep(4, 4, [1, 2], sigmas)


def test_constructor_and_add_run_argument_checks(monkeypatch):
    from v2e_amd import WindowSweep, _capi

    def touched(*a, **k):
        raise AssertionError("the library or the device was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)
    monkeypatch.setattr(_capi, "require_gpu", touched)
    for bad in (dict(height=0), dict(width=0), dict(height=65536), dict(width=65536), dict(max_rows_per_pass=0),
                dict(max_rows_per_pass=(1 << 30) + 1)):
        kw = dict(height=4, width=4, lengths=[1, 2], sigmas=[0, 1])
        kw.update(bad)
        with pytest.raises(ValueError):
            WindowSweep(**kw)
    big = WindowSweep(65535, 65535, [1], [65535])  # the limits themselves are allowed
    assert (big.height, big.width, big.max_length) == (65535, 65535, 1)
    ws = WindowSweep(4, 6, np.arange(1, 65) * 16, range(8), max_rows_per_pass=1)  # 64 lengths up to 1024, 8 sigmas, one-row passes
    assert (ws.height, ws.width, len(ws.lengths), len(ws.sigmas), ws.max_length, ws.lengths.dtype) == (4, 6, 64, 8, 1024, np.int64)
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
        dict(keep=(0, 1, 1)), dict(keep=(1025, 1, 1)), dict(keep=(1.5, 1, 1)), dict(keep=(1, -1, 1)), dict(keep=(1, 0.5, 1)),
        dict(keep=(1, 1, 0)), dict(keep=(1, 1, 5)), dict(keep=(1, 1, 1.5)), dict(keep=(1, 1)), dict(keep=3),
        dict(keep=(1, float("nan"), 1)),
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            ws.add_run(rows, **kw)
    with pytest.raises(ValueError):  # L beyond the longest length of the table
        WindowSweep(4, 6, [1, 8], [1]).add_run(rows, keep=(9, 1, 1))
    for r in (torch.zeros((6, 3)), torch.zeros((6, 4), dtype=torch.float64), torch.zeros((24,))):
        with pytest.raises(ValueError):
            ws.add_run(r)
    with pytest.raises(TypeError):  # host rows: the run's rows are a device tensor
        ws.add_run(rows)
    with pytest.raises(TypeError):
        ws.add_run(np.zeros((6, 4), np.float32))
    ws.reset()  # nothing allocated yet: nothing to do


def test_needs_a_gpu_and_says_so(monkeypatch):
    from v2e_amd import V2EAmdError, WindowSweep
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(V2EAmdError, match="WindowSweep needs a ROCm GPU"):
        WindowSweep(4, 4, [1, 2], [1]).result()


def test_ctypes_table_lists_the_entry_points():
    import v2e_amd
    from v2e_amd import _capi
    assert "WindowSweep" in v2e_amd.__all__ and "WindowResult" in v2e_amd.__all__
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "v2e_amd.h")).read()
    for name, n_args in (("v2e_window_compact", 14), ("v2e_window_depths", 19), ("v2e_window_tail", 6)):
        assert name in _capi.SIGNATURES and ("int %s(" % name) in header
        assert len(_capi.SIGNATURES[name][1]) == n_args
        assert hasattr(_capi.lib(), name)


def test_labelled_clip_conditions_with_the_oracle(oracle_lib):
    """The clip of test_window_sweep_gpu.py's real-rows case, on the CPU oracle: the first 100 frames of philox_moving_dot_64x64
    with shot_noise_rate_hz = 5 hold signal and noise rows, the keep mask keeps some rows and drops others, and the window filter
    separates the two kinds (a moving dot's events sit together, shot noise does not)."""
    from fixtures import PhiloxFixture
    from v2e_amd import WindowResult
    fx = PhiloxFixture("philox_moving_dot_64x64")
    emu = oracle_lib.OracleEmulator(seed=fx.seed, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))
    rows, counts, n_signal = [], [], []
    for f, t in zip(fx.frames[:CLIP_FRAMES], fx.times[:CLIP_FRAMES]):
        e = emu.generate_events(f, float(t))
        n = 0 if e is None else len(e)
        noise = int(np.sum(emu.last["shot_on"]) + np.sum(emu.last["shot_off"])) if n else 0
        counts.append(n)
        n_signal.append(n - noise)
        if n:
            rows.append(e)
    rows = np.concatenate(rows)
    hist, n_bad, mask, _ = fwf_serial(rows, 64, 64, CLIP_LENGTHS, CLIP_SIGMAS, labels_from_counts(counts, n_signal), keep=CLIP_KEEP)
    r = WindowResult(hist, CLIP_LENGTHS, CLIP_SIGMAS, n_bad)
    assert r.n_bad == 0 and r.n_signal >= 200 and r.n_noise >= 50 and r.n_signal + r.n_noise == len(rows)
    assert 50 < mask.sum() < len(mask) - 50
    L, sigma, k, tpr, fpr = r.best()
    assert tpr - fpr > 0.5
