"""CPU-only: the two numpy statements of DenoiseSweep's definition agree (tests/denoise_ref.py), DenoiseResult's arithmetic, the
argument checks of DenoiseSweep (all raised before the library or a device is touched), and the conditions of the labelled clip
tests/test_denoise_gpu.py runs on the GPU, pinned here with the CPU oracle alone."""
import numpy as np
import pytest
import torch

from denoise_ref import BORDER_TAUS, NOISY_DOT_RATE_HZ, border_rows, labels_from_counts, row_is_bad, stcf_bruteforce, stcf_serial


def test_border_rows_hold_what_the_gpu_test_needs():
    rows, labels = border_rows()
    H, W = 5, 7
    assert rows.shape == (3000, 4) and rows.dtype == np.float32 and labels.shape == (3000,)
    bad = np.array([row_is_bad(r, H, W) for r in rows])
    assert 60 <= bad.sum() <= 120
    assert np.isnan(rows[:, 0]).any() and np.isinf(rows[:, 0]).any() and (rows[:, 1] == W).any() and (rows[:, 2] == -1).any()
    assert (rows[:, 1] == 2.5).any()
    good = rows[~bad]
    assert np.array_equal(good[:, 0] * 1024, np.round(good[:, 0] * 1024))
    dt = np.diff(good[:, 0].astype(np.float64))
    assert (dt == 0).sum() > 300 and 0.03 < (dt < 0).mean() < 0.08
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (3, 0), (0, 2)):
        assert ((good[:, 1] == x) & (good[:, 2] == y)).sum() > 10
    assert 0.3 < labels.mean() < 0.8


def test_serial_loop_equals_bruteforce():
    """1500 random rows at 5x7 with equal time stamps, rows out of order and bad rows; a carried map; both keep masks."""
    rows, labels = border_rows(n=1500, seed=11)
    rng = np.random.RandomState(3)
    carried = np.where(rng.rand(5, 7) < 0.5, -np.inf, -rng.randint(0, 64, size=(5, 7)) * 2.0 ** -10).astype(np.float32)
    for last_t in (None, carried):
        for keep in ((1, 2.0 ** -10), (3, 2.0 ** -6), None):
            a = stcf_serial(rows, 5, 7, BORDER_TAUS, labels, last_t=last_t, keep=keep)
            b = stcf_bruteforce(rows, 5, 7, BORDER_TAUS, labels, last_t=last_t, keep=keep)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[3], b[3])
            assert (a[2] is None and b[2] is None) if keep is None else np.array_equal(a[2], b[2])
    hist, n_bad = a[0], a[1]
    assert n_bad > 20 and all(hist[k].sum() == 1500 - n_bad for k in range(8))
    assert hist[0, :, 0].sum() > 0 and hist[0, :, 1].sum() > 0  # age <= 0 and age == 2^-10 both occur
    assert hist[7, :, -1].sum() > 0


def test_serial_loop_is_split_invariant():
    rows, labels = border_rows(n=1200, seed=5)
    whole = stcf_serial(rows, 5, 7, BORDER_TAUS, labels, keep=(2, 2.0 ** -6))
    hist, n_bad, masks, m = 0, 0, [], None
    for a, b in ((0, 1), (1, 700), (700, 700), (700, 1200)):
        h, nb, mk, m = stcf_serial(rows[a:b], 5, 7, BORDER_TAUS, labels[a:b], last_t=m, keep=(2, 2.0 ** -6))
        hist, n_bad = hist + h, n_bad + nb
        masks.append(mk)
    assert np.array_equal(hist, whole[0]) and n_bad == whole[1] and np.array_equal(np.concatenate(masks), whole[2])
    assert np.array_equal(m, whole[3])


def test_result_arithmetic_on_a_hand_written_histogram():
    from v2e_amd import DenoiseResult
    taus = [0.001, 0.01, 0.1]
    hist = np.zeros((8, 2, 4), dtype=np.int64)
    hist[0, 1] = [2, 3, 4, 1]   # k = 1, signal: 10 rows
    hist[0, 0] = [1, 0, 1, 2]   # k = 1, noise: 4 rows
    hist[1, 1] = [1, 1, 3, 5]
    hist[1, 0] = [0, 0, 1, 3]
    for k in range(2, 8):
        hist[k, 1, 3], hist[k, 0, 3] = 10, 4
    r = DenoiseResult(hist, taus, n_bad=7)
    assert (r.n_signal, r.n_noise, r.n_bad) == (10, 4, 7) and r.hist.dtype == np.int64 and r.taus.dtype == np.float64
    assert r.passed.shape == (8, 2, 3) and r.passed.dtype == np.int64
    assert r.passed[0].tolist() == [[1, 1, 2], [2, 5, 9]] and r.passed[1].tolist() == [[0, 0, 1], [1, 2, 5]]
    assert not r.passed[2:].any()
    assert np.array_equal(r.tpr[0], np.array([2, 5, 9]) / 10) and np.array_equal(r.fpr[0], np.array([1, 1, 2]) / 4)
    assert r.tpr.shape == (8, 3) and r.fpr.shape == (8, 3)
    # tpr - fpr: k = 1: -0.05, 0.25, 0.4; k = 2: 0.1, 0.2, 0.25; the rest 0
    assert r.best() == (1, 0.1, 0.9, 0.5)
    # the first maximum in (k ascending, tau ascending) order
    tie = np.zeros((8, 2, 3), dtype=np.int64)
    tie[:, 1, 2], tie[:, 0, 2] = 5, 5
    tie[2, 1] = [0, 5, 0]
    tie[4, 1] = [5, 0, 0]
    assert DenoiseResult(tie, [1.0, 2.0]).best() == (3, 2.0, 1.0, 0.0)
    # NaN where the denominator is 0
    only_signal = np.zeros((8, 2, 3), dtype=np.int64)
    only_signal[:, 1, 0] = 3
    r = DenoiseResult(only_signal, [1.0, 2.0])
    assert np.isnan(r.fpr).all() and np.array_equal(r.tpr, np.ones((8, 2)))
    with pytest.raises(ValueError):
        r.best()
    with pytest.raises(ValueError):
        DenoiseResult(np.zeros((8, 2, 3), dtype=np.int64), [1.0, 2.0, 3.0])


@pytest.mark.parametrize("taus", [[], list(range(257)), [0.1, 0.1], [0.2, 0.1], [-1.0, 1.0], [0.0, np.inf], [np.nan]])
def test_constructor_refuses_bad_tau_tables(taus):
    from v2e_amd import DenoiseSweep
    with pytest.raises(ValueError):
        DenoiseSweep(4, 4, taus)


def test_constructor_and_add_run_argument_checks(monkeypatch):
    from v2e_amd import DenoiseSweep, _capi, denoise_rows

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)
    for bad in (dict(height=0), dict(width=0), dict(max_rows_per_pass=0), dict(max_rows_per_pass=(1 << 30) + 1)):
        kw = dict(height=4, width=4, taus=[0.0, 1.0])
        kw.update(bad)
        with pytest.raises(ValueError):
            DenoiseSweep(**kw)
    ds = DenoiseSweep(4, 6, np.arange(256) * 1e-3, max_rows_per_pass=1)  # 256 taus, tau 0 and a one-row pass are all allowed
    assert (ds.height, ds.width, len(ds.taus), ds.taus.dtype) == (4, 6, 256, np.float64)
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
        dict(keep=(0, 0.1)), dict(keep=(9, 0.1)), dict(keep=(1.5, 0.1)), dict(keep=(1, -0.1)), dict(keep=(1, float("nan"))),
        dict(keep=3),
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            ds.add_run(rows, **kw)
    for r in (torch.zeros((6, 3)), torch.zeros((6, 4), dtype=torch.float64), torch.zeros((24,))):
        with pytest.raises(ValueError):
            ds.add_run(r)
    with pytest.raises(TypeError):  # host rows: the run's rows are a device tensor
        ds.add_run(rows)
    with pytest.raises(TypeError):
        ds.add_run(np.zeros((6, 4), np.float32))
    with pytest.raises(ValueError):
        denoise_rows(rows, [6], torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError):
        denoise_rows(rows, [5], lab)
    kept, counts_kept = denoise_rows(rows, [2, 0, 4], torch.tensor([True, False, False, True, True, False]))  # (torch alone: any device)
    assert kept.shape == (3, 4) and counts_kept.tolist() == [1, 0, 2] and counts_kept.dtype == np.int64


def test_label_bounds_table():
    from v2e_amd.denoise import label_bounds
    counts, n_signal = [0, 3, 2, 0, 4], [0, 3, 0, 0, 1]
    b, covered = label_bounds(counts, n_signal)
    assert covered == 9 and b.dtype == np.int64 and np.all(np.diff(b) >= 0) and len(b) == 10
    want = labels_from_counts(counts, n_signal)
    got = np.array([np.searchsorted(b, g, side="right") & 1 for g in range(9)], dtype=bool)
    assert np.array_equal(got, want) and want.tolist() == [True] * 3 + [False] * 2 + [True] + [False] * 3


def test_labelled_clip_conditions_with_the_oracle(oracle_lib):
    """The clip of test_denoise_gpu.py's end-to-end case, on the CPU oracle: philox_moving_dot_64x64's frames and parameters with
    shot_noise_rate_hz = 5 give 8486 signal and 961 noise rows, and the correlation filter separates them (a moving dot is
    correlated, shot noise is not): the best (k, tau) of a 16-entry table has tpr 0.98 against fpr 0.065."""
    from fixtures import PhiloxFixture
    from v2e_amd import DenoiseResult
    fx = PhiloxFixture("philox_moving_dot_64x64")
    kw = dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ)
    emu = oracle_lib.OracleEmulator(seed=fx.seed, rng_mode="philox", **kw)
    rows, counts, n_signal = [], [], []
    for f, t in zip(fx.frames, fx.times):
        e = emu.generate_events(f, float(t))
        n = 0 if e is None else len(e)
        noise = int(np.sum(emu.last["shot_on"]) + np.sum(emu.last["shot_off"])) if n else 0
        counts.append(n)
        n_signal.append(n - noise)
        if n:
            rows.append(e)
    rows = np.concatenate(rows)
    taus = np.geomspace(1e-4, 1e-1, 16)
    hist, n_bad, _, _ = stcf_serial(rows, 64, 64, taus, labels_from_counts(counts, n_signal))
    r = DenoiseResult(hist, taus, n_bad)
    assert (r.n_signal, r.n_noise, r.n_bad) == (8486, 961, 0)
    k, tau, tpr, fpr = r.best()
    assert tpr > 0.9 and fpr < 0.1
