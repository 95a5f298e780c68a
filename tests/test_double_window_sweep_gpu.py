"""v2e_amd.DoubleWindowSweep on the MI355X against the numpy definition (tests/double_window_ref.py): every comparison is exact.
What the inputs must hold for these cases to mean something is pinned on the CPU in tests/test_double_window_sweep.py."""
import numpy as np
import pytest
import torch

from denoise_ref import NOISY_DOT_RATE_HZ
from double_window_ref import (BORDER_KEEPS, BORDER_LENGTHS, BORDER_SIGMAS, BORDER_SUPPORTS, CLIP_FRAMES, CLIP_KEEP, CLIP_LENGTHS,
                               CLIP_SIGMAS, CLIP_SUPPORTS, FULL_BAD, FULL_H, FULL_KEEP, FULL_LENGTHS, FULL_N, FULL_SIGMAS, FULL_SUPPORTS,
                               FULL_W, XY_NONE, border_rows, burst_rows, dwf_serial, full_window_rows, labels_from_counts, row_is_bad)
from fixtures import PhiloxFixture

pytestmark = pytest.mark.gpu

H5, W7 = 5, 7
BORDER_TABLES = (BORDER_LENGTHS, BORDER_SIGMAS, BORDER_SUPPORTS)


@pytest.fixture(scope="module")
def border():
    """The shared rows of cases 1 and 2 and their reference, computed once: (rows, labels, reference without a mask, {keep: mask})."""
    rows, labels = border_rows(H5, W7, 3000)
    ref = dwf_serial(rows, H5, W7, *BORDER_TABLES, labels=labels)
    masks = {keep: dwf_serial(rows, H5, W7, *BORDER_TABLES, labels=labels, keep=keep)[4] for keep in BORDER_KEEPS}
    return rows, labels, ref, masks


def sweep(H, W, lengths, sigmas, supports, **kw):
    from v2e_amd import DoubleWindowSweep
    return DoubleWindowSweep(H, W, lengths, sigmas, supports, device="cuda", **kw)


def same_counts(res, ref):
    passed, n_signal, n_noise, n_bad = ref[:4]
    return (res.passed.dtype == np.int64 and np.array_equal(res.passed, passed)
            and (res.n_signal, res.n_noise, res.n_bad) == (n_signal, n_noise, n_bad))


@pytest.mark.parametrize("labels_on_host", [False, True])
def test_borders_and_bad_rows(border, labels_on_host):
    rows, labels, ref, masks = border
    n_bad = ref[3]
    dev_rows = torch.from_numpy(rows).cuda()
    lab = torch.from_numpy(labels)
    for keep in BORDER_KEEPS:
        ws = sweep(H5, W7, *BORDER_TABLES)
        out = ws.add_run(dev_rows, labels=lab if labels_on_host else lab.cuda(), keep=keep)
        res = ws.result()
        assert out["mask"].dtype == torch.bool and out["mask"].is_cuda
        assert np.array_equal(out["mask"].cpu().numpy(), masks[keep])
        assert out["n"].is_cuda and out["n"].dim() == 0 and out["n_bad"].dim() == 0 and out["n"].dtype == torch.int64
        assert (int(out["n"]), int(out["n_bad"])) == (3000 - n_bad, n_bad)
        assert res.passed.shape == (4, 3, 5, 2) and same_counts(res, ref) and res.n_signal + res.n_noise == 3000 - n_bad
        win = ws.windows
        assert win.dtype == torch.int64 and win.is_cuda and win.shape == (4, 3, 5, 2, 8)
        assert np.array_equal(win.cpu().numpy(), ref[5])


def test_cut_invariance_and_carry(border):
    rows, labels, ref, masks = border
    keep = BORDER_KEEPS[1]
    dev_rows, lab = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()

    def feed(ws, cuts):
        got = [ws.add_run(dev_rows[a:b], labels=lab[a:b], keep=keep)["mask"] for a, b in cuts]
        return torch.cat(got).cpu().numpy(), ws.result(), ws.windows.cpu().numpy()

    one = sweep(H5, W7, *BORDER_TABLES)
    four = sweep(H5, W7, *BORDER_TABLES)
    blocks = sweep(H5, W7, *BORDER_TABLES, max_rows_per_pass=257)
    for ws, cuts in ((one, [(0, 3000)]), (four, [(0, 1), (1, 1777), (1777, 1777), (1777, 3000)]), (blocks, [(0, 3000)])):
        mask, res, win = feed(ws, cuts)
        assert np.array_equal(mask, masks[keep]) and same_counts(res, ref) and np.array_equal(win, ref[5])
    assert (one.passes, four.passes, blocks.passes) == (1, 3, 12)
    blocks.reset()
    res = blocks.result()
    assert not res.passed.any() and (res.n_signal, res.n_noise, res.n_bad) == (0, 0, 0) and bool((blocks.windows == XY_NONE).all())
    mask, res, win = feed(blocks, [(0, 3000)])
    assert np.array_equal(mask, masks[keep]) and same_counts(res, ref) and np.array_equal(win, ref[5])
    # cuts after exactly 64 and 128 valid rows: the chunk boundaries of the kernel
    valid = np.array([not row_is_bad(r, H5, W7) for r in rows])
    at = [int(np.flatnonzero(np.cumsum(valid) == m)[0]) + 1 for m in (64, 128)]
    assert valid[:at[0]].sum() == 64 and valid[:at[1]].sum() == 128
    chunked = sweep(H5, W7, *BORDER_TABLES)
    mask, res, win = feed(chunked, [(0, at[0]), (at[0], at[1]), (at[1], 3000)])
    assert np.array_equal(mask, masks[keep]) and same_counts(res, ref) and np.array_equal(win, ref[5])


def test_full_windows():
    """6000 rows at 33x37, 250 of them bad: windows that wrap, lengths on both sides of the 64-lane stride, an early stop for the
    large sigma and a full walk for sigma 0; labels from a frame table."""
    rows, counts, n_signal = full_window_rows(FULL_H, FULL_W, FULL_N, FULL_BAD)
    ref = dwf_serial(rows, FULL_H, FULL_W, FULL_LENGTHS, FULL_SIGMAS, FULL_SUPPORTS, labels_from_counts(counts, n_signal), keep=FULL_KEEP)
    ws = sweep(FULL_H, FULL_W, FULL_LENGTHS, FULL_SIGMAS, FULL_SUPPORTS)
    out = ws.add_run(torch.from_numpy(rows).cuda(), counts, 0, n_signal=n_signal, keep=FULL_KEEP)
    res = ws.result()
    assert (int(out["n"]), int(out["n_bad"])) == (FULL_N - FULL_BAD, FULL_BAD)
    assert same_counts(res, ref) and np.array_equal(ws.windows.cpu().numpy(), ref[5])
    assert np.array_equal(out["mask"].cpu().numpy(), ref[4]) and ref[4].any()


def test_real_rows_end_to_end():
    """The first 100 frames of philox_moving_dot_64x64.npz through EventEmulator(rng_mode="philox") with shot_noise_rate_hz = 5 in
    two device-resident runs, labelled by emu.last_n_signal; the keep mask through denoise_rows."""
    from v2e_amd import EventEmulator, denoise_rows
    fx = PhiloxFixture("philox_moving_dot_64x64")
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))
    ws = sweep(64, 64, CLIP_LENGTHS, CLIP_SIGMAS, CLIP_SUPPORTS)
    host, dev, masks, all_counts, all_signal = [], [], [], [], []
    for a, b in ((0, 60), (60, CLIP_FRAMES)):
        rows, counts = emu.generate_events_batch(fx.frames[a:b], fx.times[a:b], return_device=True)
        n_signal = emu.last_n_signal
        out = ws.add_run(rows, counts, a, n_signal=n_signal, keep=CLIP_KEEP)
        masks.append(out["mask"])
        dev.append(rows.clone())
        host.append(rows.cpu().numpy())
        all_counts.append(np.array(counts))
        all_signal.append(np.array(n_signal))
    counts, n_signal = np.concatenate(all_counts), np.concatenate(all_signal)
    rows, mask = np.concatenate(host), torch.cat(masks)
    res = ws.result()
    ref = dwf_serial(rows, 64, 64, CLIP_LENGTHS, CLIP_SIGMAS, CLIP_SUPPORTS, labels_from_counts(counts, n_signal), keep=CLIP_KEEP)
    want = ref[4]
    assert ref[3] == 0 and same_counts(res, ref) and np.array_equal(ws.windows.cpu().numpy(), ref[5])
    assert res.n_signal == n_signal.sum() and res.n_noise == counts.sum() - n_signal.sum() and res.n_signal > 0 and res.n_noise > 0
    assert np.array_equal(mask.cpu().numpy(), want) and 0 < want.sum() < len(want)
    kept, counts_kept = denoise_rows(torch.cat(dev), counts, mask)
    assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), rows[want])
    frame = np.repeat(np.arange(len(counts)), counts)
    assert np.array_equal(counts_kept, np.bincount(frame[want], minlength=len(counts)))
    L, sigma, k, tpr, fpr = res.best()
    assert tpr > fpr


def test_degenerate_inputs():
    ws = sweep(4, 6, [2, 4], [0, 1], [1, 2])
    for empty in (None, torch.zeros((0, 4), dtype=torch.float32, device="cuda")):
        out = ws.add_run(empty, keep=(2, 0, 1))
        assert (int(out["n"]), int(out["n_bad"])) == (0, 0) and out["mask"].shape == (0,) and out["mask"].dtype == torch.bool
        assert ws.add_run(empty, counts=[0, 0], n_signal=[0, 0])["mask"] is None
    assert not ws.result().passed.any() and ws.passes == 0 and bool((ws.windows == XY_NONE).all())
    # one row: both windows are empty, it fails and sits in N
    out = ws.add_run(torch.tensor([[0.5, 5.0, 3.0, 1.0]], device="cuda"), keep=(4, 1, 1))
    res = ws.result()
    assert (int(out["n"]), int(out["n_bad"]), out["mask"].tolist()) == (1, 0, [False])
    assert not res.passed.any() and (res.n_signal, res.n_noise, res.n_bad) == (1, 0, 0)
    win = ws.windows
    assert win.shape == (2, 2, 2, 2, 4) and bool((win[:, :, :, 0] == XY_NONE).all())
    assert win[:, :, :, 1].reshape(-1, 4).tolist() == [[XY_NONE] * 3 + [5 | (3 << 16)]] * 8
    # all rows bad: nothing but n_bad moves
    bad = torch.tensor([[float("nan"), 1, 1, 1], [float("-inf"), 1, 1, 1], [0.1, 6, 1, 1], [0.1, 1, -1, 1], [0.1, 1, 4, 1], [0.1, 0.5, 1, -1]],
                       dtype=torch.float32, device="cuda")
    out = ws.add_run(bad, labels=torch.zeros(6, dtype=torch.bool), keep=(4, 1, 2))
    res2 = ws.result()
    assert (int(out["n"]), int(out["n_bad"]), out["mask"].tolist(), res2.n_bad) == (0, 6, [False] * 6, 6)
    assert not res2.passed.any() and (res2.n_signal, res2.n_noise) == (1, 0) and torch.equal(ws.windows, win)
    # the same pixel over and over: (L, 0, k) fails every row if L < k, else exactly the first k
    lengths, supports = (1, 2, 3, 4, 7), (1, 2, 3, 4)
    one = sweep(1, 1, lengths, [0], supports)
    rows = torch.zeros((300, 4), dtype=torch.float32, device="cuda")
    out = one.add_run(rows, labels=torch.arange(300) % 3 == 0, keep=(3, 0, 3))
    res = one.result()
    assert out["mask"].tolist() == [False] * 3 + [True] * 297 and (res.n_signal, res.n_noise) == (100, 200)
    for ki, k in enumerate(supports):
        for li, L in enumerate(lengths):
            assert int(res.passed[ki, 0, li].sum()) == (0 if L < k else 300 - k)
    assert res.passed[2, 0, 2].tolist() == [198, 99]  # k = 3, L = 3: rows 3 .. 299 pass, 99 of them signal (rows 3, 6, ..)
    # a burst of noise does not flush the real window
    burst = sweep(64, 64, [4], [1], [1])
    out = burst.add_run(torch.from_numpy(burst_rows()).cuda(), keep=(4, 1, 1))
    assert out["mask"].tolist() == [False, True, True] + [False] * 9 + [True]
    assert burst.windows[0, 0, 0, 0].tolist() == [XY_NONE, 10 | (10 << 16), 10 | (10 << 16), 11 | (10 << 16)]
