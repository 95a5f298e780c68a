"""v2e_amd.WindowSweep on the MI355X against the numpy definition (tests/window_filter_ref.py): every comparison is exact.  What the
inputs must hold for these cases to mean something is pinned on the CPU in tests/test_window_sweep.py."""
import numpy as np
import pytest
import torch

from denoise_ref import NOISY_DOT_RATE_HZ
from fixtures import PhiloxFixture
from window_filter_ref import (BORDER_KEEPS, BORDER_LENGTHS, BORDER_SIGMAS, CLIP_FRAMES, CLIP_KEEP, CLIP_LENGTHS, CLIP_SIGMAS, FULL_LENGTHS,
                               FULL_SIGMAS, XY_NONE, border_rows, full_window_rows, fwf_serial, labels_from_counts)

pytestmark = pytest.mark.gpu

H5, W7 = 5, 7
LONG_LENGTHS = BORDER_LENGTHS + (1024,)


@pytest.fixture(scope="module")
def border():
    """The shared rows of cases 1 and 2 and their reference, computed once: (rows, labels, hist, n_bad, {keep: mask}, final tail)."""
    rows, labels = border_rows(H5, W7, 3000)
    masks = {}
    for keep in BORDER_KEEPS:
        hist, n_bad, masks[keep], tail = fwf_serial(rows, H5, W7, BORDER_LENGTHS, BORDER_SIGMAS, labels, keep=keep)
    return rows, labels, hist, n_bad, masks, tail


def sweep(H, W, lengths, sigmas, **kw):
    from v2e_amd import WindowSweep
    return WindowSweep(H, W, lengths, sigmas, device="cuda", **kw)


@pytest.mark.parametrize("labels_on_host", [False, True])
def test_borders_ties_and_bad_rows(border, labels_on_host):
    rows, labels, hist, n_bad, masks, tail = border
    n_valid = len(rows) - n_bad
    dev_rows = torch.from_numpy(rows).cuda()
    lab = torch.from_numpy(labels)
    for keep in BORDER_KEEPS:
        ws = sweep(H5, W7, BORDER_LENGTHS, BORDER_SIGMAS)
        out = ws.add_run(dev_rows, labels=lab if labels_on_host else lab.cuda(), keep=keep)
        res = ws.result()
        assert out["mask"].dtype == torch.bool and out["mask"].is_cuda
        assert np.array_equal(out["mask"].cpu().numpy(), masks[keep])
        assert out["n"].is_cuda and out["n"].dim() == 0 and out["n_bad"].dim() == 0
        assert (int(out["n"]), int(out["n_bad"]), res.n_bad) == (n_valid, n_bad, n_bad)
        assert res.hist.dtype == np.int64 and res.hist.shape == (4, 3, 2, 6) and np.array_equal(res.hist, hist)
        assert all(res.hist[k, s].sum() == n_valid for k in range(4) for s in range(3))
        assert res.n_signal + res.n_noise == n_valid
        assert np.array_equal(ws.tail.cpu().numpy(), tail)


def test_cut_invariance_and_carry(border):
    rows, labels, hist, n_bad, masks, tail = border
    keep = BORDER_KEEPS[1]
    dev_rows, lab = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()

    def feed(ws, cuts, keep=keep):
        got = [ws.add_run(dev_rows[a:b], labels=lab[a:b], keep=keep)["mask"] for a, b in cuts]
        return torch.cat(got).cpu().numpy(), ws.result(), ws.tail.cpu().numpy()

    one = sweep(H5, W7, BORDER_LENGTHS, BORDER_SIGMAS)
    four = sweep(H5, W7, BORDER_LENGTHS, BORDER_SIGMAS)
    blocks = sweep(H5, W7, BORDER_LENGTHS, BORDER_SIGMAS, max_rows_per_pass=257)
    for ws, cuts in ((one, [(0, 3000)]), (four, [(0, 1), (1, 1777), (1777, 1777), (1777, 3000)]), (blocks, [(0, 3000)])):
        mask, res, t = feed(ws, cuts)
        assert np.array_equal(mask, masks[keep]) and np.array_equal(res.hist, hist) and res.n_bad == n_bad
        assert np.array_equal(t, tail)
    assert (one.passes, four.passes, blocks.passes) == (1, 3, 12)
    blocks.reset()
    assert not blocks.result().hist.any() and blocks.result().n_bad == 0 and bool((blocks.tail == XY_NONE).all())
    mask, res, t = feed(blocks, [(0, 3000)])
    assert np.array_equal(mask, masks[keep]) and np.array_equal(res.hist, hist) and res.n_bad == n_bad and np.array_equal(t, tail)

    # a window longer than the first call's rows: "no row yet" words cross a call boundary
    keep_long = (700, 0, 4)
    hist_l, n_bad_l, mask_l, tail_l = fwf_serial(rows, H5, W7, LONG_LENGTHS, BORDER_SIGMAS, labels, keep=keep_long)
    assert (tail_l == XY_NONE).sum() == 0 and mask_l.any() and not mask_l.all()
    long = sweep(H5, W7, LONG_LENGTHS, BORDER_SIGMAS)
    first = long.add_run(dev_rows[:300], labels=lab[:300], keep=keep_long)["mask"]
    t300 = long.tail.cpu().numpy()
    assert (t300 == XY_NONE).sum() == 1024 - int(first.numel() - int(long.result().n_bad)) and t300[0] == XY_NONE and t300[-1] != XY_NONE
    rest = long.add_run(dev_rows[300:], labels=lab[300:], keep=keep_long)["mask"]
    res = long.result()
    assert np.array_equal(torch.cat([first, rest]).cpu().numpy(), mask_l)
    assert np.array_equal(res.hist, hist_l) and res.n_bad == n_bad_l and np.array_equal(long.tail.cpu().numpy(), tail_l)


def test_full_window():
    """12 000 rows at 33x37, 500 of them bad, 52 lengths up to 1024 and 8 sigmas: the walk runs to the end of a full window for the
    small sigmas and stops early for the large ones; labels from a frame table."""
    rows, counts, n_signal = full_window_rows()
    hist, n_bad, mask, tail = fwf_serial(rows, 33, 37, FULL_LENGTHS, FULL_SIGMAS, labels_from_counts(counts, n_signal), keep=(1000, 0, 4))
    assert ((hist.sum(axis=2) > 0).sum(axis=2) >= 30).all()  # at least 30 populated bins for every (k, sigma)
    ws = sweep(33, 37, FULL_LENGTHS, FULL_SIGMAS)
    out = ws.add_run(torch.from_numpy(rows).cuda(), counts, 0, n_signal=n_signal, keep=(1000, 0, 4))
    res = ws.result()
    assert (int(out["n"]), int(out["n_bad"]), res.n_bad) == (12000 - n_bad, n_bad, n_bad) and n_bad == 500
    assert np.array_equal(res.hist, hist) and np.array_equal(ws.tail.cpu().numpy(), tail)
    assert np.array_equal(out["mask"].cpu().numpy(), mask) and mask.any() and not mask[rows[:, 2] >= 0].all()
    valid_signal = int(labels_from_counts(counts, n_signal)[np.isfinite(rows[:, 0]) & (rows[:, 2] >= 0)].sum())
    assert res.n_signal == valid_signal and res.n_noise == 12000 - n_bad - valid_signal


def test_real_rows_end_to_end():
    """The first 100 frames of philox_moving_dot_64x64.npz through EventEmulator(rng_mode="philox") with shot_noise_rate_hz = 5 in
    two device-resident runs, labelled by emu.last_n_signal; the keep mask through denoise_rows."""
    from v2e_amd import EventEmulator, denoise_rows
    fx = PhiloxFixture("philox_moving_dot_64x64")
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))
    ws = sweep(64, 64, CLIP_LENGTHS, CLIP_SIGMAS)
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
    hist, n_bad, want, tail = fwf_serial(rows, 64, 64, CLIP_LENGTHS, CLIP_SIGMAS, labels_from_counts(counts, n_signal), keep=CLIP_KEEP)
    assert n_bad == 0 and res.n_bad == 0 and np.array_equal(res.hist, hist) and np.array_equal(ws.tail.cpu().numpy(), tail)
    assert res.n_signal == n_signal.sum() and res.n_noise == counts.sum() - n_signal.sum() and res.n_signal > 0 and res.n_noise > 0
    assert np.array_equal(mask.cpu().numpy(), want) and 0 < want.sum() < len(want)
    kept, counts_kept = denoise_rows(torch.cat(dev), counts, mask)
    assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), rows[want])
    frame = np.repeat(np.arange(len(counts)), counts)
    assert np.array_equal(counts_kept, np.bincount(frame[want], minlength=len(counts)))
    L, sigma, k, tpr, fpr = res.best()
    assert tpr > fpr


def test_degenerate_inputs():
    ws = sweep(4, 6, [2, 4], [0, 1])
    for empty in (None, torch.zeros((0, 4), dtype=torch.float32, device="cuda")):
        out = ws.add_run(empty, keep=(1, 0, 1))
        assert (int(out["n"]), int(out["n_bad"])) == (0, 0) and out["mask"].shape == (0,) and out["mask"].dtype == torch.bool
        assert ws.add_run(empty, counts=[0, 0], n_signal=[0, 0])["mask"] is None
    assert not ws.result().hist.any() and ws.passes == 0
    # one row: the window is empty, every depth is Lmax + 1
    out = ws.add_run(torch.tensor([[0.5, 5.0, 3.0, 1.0]], device="cuda"), keep=(4, 1 << 40, 1))
    res = ws.result()
    assert (int(out["n"]), int(out["n_bad"]), out["mask"].tolist()) == (1, 0, [False])
    assert res.hist[:, :, 1, 2].tolist() == [[1, 1]] * 4 and res.hist.sum() == 8
    assert ws.tail.tolist() == [XY_NONE] * 3 + [5 | (3 << 16)]
    # all rows bad: nothing but n_bad moves
    bad = torch.tensor([[float("nan"), 1, 1, 1], [float("-inf"), 1, 1, 1], [0.1, 6, 1, 1], [0.1, 1, -1, 1], [0.1, 1, 4, 1], [0.1, 0.5, 1, -1]],
                       dtype=torch.float32, device="cuda")
    out = ws.add_run(bad, labels=torch.zeros(6, dtype=torch.bool), keep=(4, 9, 4))
    res2 = ws.result()
    assert (int(out["n"]), int(out["n_bad"]), out["mask"].tolist(), res2.n_bad) == (0, 6, [False] * 6, 6)
    assert np.array_equal(res2.hist, res.hist) and ws.tail.tolist() == [XY_NONE] * 3 + [5 | (3 << 16)]
    # the same pixel over and over: depth k for every sigma, and a huge keep sigma never counts a "no row yet" word
    one = sweep(1, 1, [1, 2, 3, 4], [0, 65535])
    rows = torch.zeros((300, 4), dtype=torch.float32, device="cuda")
    out = one.add_run(rows, labels=torch.arange(300) % 3 == 0, keep=(3, 1 << 40, 3))
    res = one.result()
    assert out["mask"].tolist() == [False] * 3 + [True] * 297
    for k in range(4):  # row m has m rows before it: d_k = k for m >= k, else Lmax + 1 = 5 (bin 4)
        want = np.zeros(5, dtype=np.int64)
        want[k], want[4] = 300 - (k + 1), k + 1
        assert np.array_equal(res.hist[k, 0].sum(axis=0), want) and np.array_equal(res.hist[k, 1], res.hist[k, 0])
    assert res.n_signal == 100 and res.n_noise == 200
