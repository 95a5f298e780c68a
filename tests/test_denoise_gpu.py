"""v2e_amd.DenoiseSweep on the MI355X against the numpy definition (tests/denoise_ref.py): every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from denoise_ref import BORDER_TAUS, NOISY_DOT_RATE_HZ, border_rows, labels_from_counts, row_is_bad, stcf_serial
from fixtures import GOLDEN, PhiloxFixture

pytestmark = pytest.mark.gpu

H5, W7 = 5, 7
KEEPS = ((1, 2.0 ** -10), (3, 2.0 ** -6))


@pytest.fixture(scope="module")
def border():
    """The shared rows of cases 1 and 2 and their reference, computed once: (rows, labels, hist, n_bad, {keep: mask}, final map)."""
    rows, labels = border_rows(H5, W7, 3000)
    masks = {}
    for keep in KEEPS:
        hist, n_bad, masks[keep], last_t = stcf_serial(rows, H5, W7, BORDER_TAUS, labels, keep=keep)
    return rows, labels, hist, n_bad, masks, last_t


def sweep(H, W, taus, **kw):
    from v2e_amd import DenoiseSweep
    return DenoiseSweep(H, W, taus, device="cuda", **kw)


@pytest.mark.parametrize("labels_on_host", [False, True])
def test_borders_and_ties(border, labels_on_host):
    rows, labels, hist, n_bad, masks, last_t = border
    n_valid = len(rows) - n_bad
    dev_rows = torch.from_numpy(rows).cuda()
    lab = torch.from_numpy(labels)
    for keep in KEEPS:
        ds = sweep(H5, W7, BORDER_TAUS)
        out = ds.add_run(dev_rows, labels=lab if labels_on_host else lab.cuda(), keep=keep)
        res = ds.result()
        assert out["mask"].dtype == torch.bool and out["mask"].is_cuda
        assert np.array_equal(out["mask"].cpu().numpy(), masks[keep])
        assert (int(out["n"]), int(out["n_bad"]), res.n_bad) == (n_valid, n_bad, n_bad)
        assert res.hist.dtype == np.int64 and np.array_equal(res.hist, hist)
        assert all(res.hist[k].sum() == n_valid for k in range(8))
        assert res.n_signal + res.n_noise == n_valid and res.n_signal == int(labels[[not row_is_bad(r, H5, W7) for r in rows]].sum())
        assert np.array_equal(ds.last_t.cpu().numpy(), last_t)
    # what the table was made for: age == 0 and age == tau both occur, and some rows pass no tau
    assert hist[0, :, 0].sum() > 0 and hist[0, :, 1].sum() > 0 and hist[7, :, -1].sum() > 0


def test_split_invariance(border):
    rows, labels, hist, n_bad, masks, last_t = border
    keep = KEEPS[1]
    dev_rows, lab = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()

    def feed(ds, cuts):
        got = [ds.add_run(dev_rows[a:b], labels=lab[a:b], keep=keep)["mask"] for a, b in cuts]
        return torch.cat(got).cpu().numpy(), ds.result(), ds.last_t.cpu().numpy()

    one = sweep(H5, W7, BORDER_TAUS)
    three = sweep(H5, W7, BORDER_TAUS)
    blocks = sweep(H5, W7, BORDER_TAUS, max_rows_per_pass=257)
    for ds, cuts in ((one, [(0, 3000)]), (three, [(0, 1), (1, 1777), (1777, 1777), (1777, 3000)]), (blocks, [(0, 3000)])):
        mask, res, m = feed(ds, cuts)
        assert np.array_equal(mask, masks[keep]) and np.array_equal(res.hist, hist) and res.n_bad == n_bad
        assert np.array_equal(m, last_t)
    assert (one.passes, three.passes, blocks.passes) == (1, 3, 12)
    blocks.reset()
    assert not blocks.result().hist.any() and bool(torch.isinf(blocks.last_t).all())
    mask, res, m = feed(blocks, [(0, 3000)])
    assert np.array_equal(mask, masks[keep]) and np.array_equal(res.hist, hist) and res.n_bad == n_bad and np.array_equal(m, last_t)


LONG_TAUS = np.geomspace(2.0 ** -14, 4.0, 256)
_long = {}


def long_case(frames):
    """33x37, 70 000 rows, 40 000 of them on one pixel and its eight neighbours, labelled by a table of `frames` frames, and the
    reference (computed once): (rows, counts, n_signal, hist, final map)."""
    if frames not in _long:
        H, W, n = 33, 37, 70000
        rng = np.random.RandomState(21)
        hot = rng.rand(n) < 40000 / n
        x = np.where(hot, 17 + rng.randint(-1, 2, size=n), rng.randint(0, W, size=n))
        y = np.where(hot, 12 + rng.randint(-1, 2, size=n), rng.randint(0, H, size=n))
        t = np.cumsum(rng.randint(0, 3, size=n)) * 2.0 ** -14
        rows = np.stack([t, x, y, np.ones(n)], axis=1).astype(np.float32)
        counts = np.bincount(rng.randint(0, frames, size=n), minlength=frames)
        n_signal = (counts * rng.rand(frames)).astype(np.int64)
        hist, n_bad, _, last_t = stcf_serial(rows, H, W, LONG_TAUS, labels_from_counts(counts, n_signal))
        assert n_bad == 0 and len(np.flatnonzero(hist[0].sum(axis=0))) > 20
        _long[frames] = rows, counts, n_signal, hist, last_t
    return _long[frames]


@pytest.mark.parametrize("frames", [50, 3000])
def test_long_per_pixel_lists(frames):
    """Row indices pass 2^16, stretches of thousands of rows to search, 256 taus; labels from a frame table that the kernel stages
    in LDS (50 frames) and one it reads from memory (3000 frames)."""
    rows, counts, n_signal, hist, last_t = long_case(frames)
    ds = sweep(33, 37, LONG_TAUS)
    ds.add_run(torch.from_numpy(rows).cuda(), counts, 0, n_signal=n_signal)
    res = ds.result()
    assert res.n_bad == 0 and np.array_equal(res.hist, hist) and np.array_equal(ds.last_t.cpu().numpy(), last_t)
    assert res.n_signal == int(n_signal.sum()) and res.n_noise == 70000 - res.n_signal


def test_emulator_labels_end_to_end():
    """The frames of philox_moving_dot_64x64.npz through EventEmulator(rng_mode="philox") with shot_noise_rate_hz = 5 (the fixture's
    other parameters) in two device-resident runs, labelled by emu.last_n_signal: on the CPU oracle this clip has 8486 signal and
    961 noise rows and the best filter of the table has tpr 0.98, fpr 0.065 (tests/test_denoise.py pins both)."""
    from v2e_amd import EventEmulator
    fx = PhiloxFixture("philox_moving_dot_64x64")
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))
    taus = np.geomspace(1e-4, 1e-1, 16)
    ds = sweep(64, 64, taus)
    assert emu.last_n_signal is None
    host, all_counts, all_signal, frame0 = [], [], [], 0
    for a, b in ((0, 260), (260, 500)):
        rows, counts = emu.generate_events_batch(fx.frames[a:b], fx.times[a:b], return_device=True)
        n_signal = emu.last_n_signal
        assert n_signal.dtype == np.int64 and n_signal.shape == counts.shape and np.all(n_signal <= counts) and np.all(n_signal >= 0)
        ds.add_run(rows, counts, frame0, n_signal=n_signal)
        host.append(rows.cpu().numpy())
        all_counts.append(np.array(counts))
        all_signal.append(np.array(n_signal))
        frame0 += b - a
    counts, n_signal = np.concatenate(all_counts), np.concatenate(all_signal)
    assert counts[0] == 0 and n_signal[0] == 0  # the clip's first frame
    res = ds.result()
    assert res.n_bad == 0 and res.n_signal + res.n_noise == counts.sum()
    assert res.n_signal == n_signal.sum() and res.n_signal >= 200 and res.n_noise >= 200
    hist, _, _, _ = stcf_serial(np.concatenate(host), 64, 64, taus, labels_from_counts(counts, n_signal))
    assert np.array_equal(res.hist, hist)
    k, tau, tpr, fpr = res.best()
    assert tpr > fpr


def test_denoise_rows_and_callback_feed():
    """denoise_rows against host indexing, and a sweep fed block by block from SyntheticToEvents' callback (500 frames in blocks of
    300: one boundary) against one fed the gathered rows."""
    from v2e_amd import EventEmulator, SyntheticToEvents, denoise_rows, moving_dot
    fx = PhiloxFixture("philox_moving_dot_64x64")
    z = np.load(os.path.join(GOLDEN, "synth_moving_dot_64x64.npz"), allow_pickle=False)
    src = moving_dot(int(z["W"]), int(z["H"]), arg_list=json.loads(str(z["arg_list"])), device="cuda")
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))
    taus = np.geomspace(1e-4, 1e-1, 16)
    fed, keep = sweep(64, 64, taus), (2, 2e-3)
    got = []

    def on_events(ev, cnt, frame0):
        n_signal = emu.last_n_signal
        assert len(n_signal) == len(cnt)
        out = fed.add_run(ev, cnt, frame0, n_signal=n_signal, keep=keep)
        got.append((ev.clone(), np.array(cnt), np.array(n_signal), out["mask"]))
    _, counts, n = SyntheticToEvents(src, emu, block_frames=300).run(on_events, return_device=True)
    assert n == 500 and [len(g[1]) for g in got] == [300, 200]
    rows = torch.cat([g[0] for g in got])
    n_signal = np.concatenate([g[2] for g in got])
    mask = torch.cat([g[3] for g in got])
    assert np.array_equal(np.concatenate([g[1] for g in got]), counts) and rows.shape[0] == counts.sum()
    whole = sweep(64, 64, taus)
    out = whole.add_run(rows, counts, 0, n_signal=n_signal, keep=keep)
    a, b = fed.result(), whole.result()
    assert np.array_equal(a.hist, b.hist) and a.n_signal == n_signal.sum() and a.n_noise == counts.sum() - n_signal.sum()
    assert a.n_noise >= 200 and torch.equal(mask, out["mask"]) and torch.equal(fed.last_t, whole.last_t)

    kept, counts_kept = denoise_rows(rows, counts, mask)
    m = mask.cpu().numpy()
    assert 0 < m.sum() < len(m)
    assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), rows.cpu().numpy()[m])
    frame = np.repeat(np.arange(len(counts)), counts)
    assert counts_kept.dtype == np.int64 and np.array_equal(counts_kept, np.bincount(frame[m], minlength=len(counts)))
    assert denoise_rows(rows, None, mask)[1] is None


def test_degenerate_inputs():
    taus = [1e-3, 1e-2]
    ds = sweep(4, 6, taus)
    for empty in (None, torch.zeros((0, 4), dtype=torch.float32, device="cuda")):
        out = ds.add_run(empty, keep=(1, 1e-3))
        assert (int(out["n"]), int(out["n_bad"])) == (0, 0) and out["mask"].shape == (0,) and out["mask"].dtype == torch.bool
        assert ds.add_run(empty, counts=[0, 0], n_signal=[0, 0])["mask"] is None
    assert not ds.result().hist.any() and ds.passes == 0
    # one row: all eight ages are +inf
    out = ds.add_run(torch.tensor([[0.5, 5.0, 3.0, 1.0]], device="cuda"), keep=(1, 1e9))
    res = ds.result()
    assert (int(out["n"]), int(out["n_bad"]), out["mask"].tolist()) == (1, 0, [False])
    assert res.hist[:, 1, 2].tolist() == [1] * 8 and res.hist.sum() == 8 and ds.last_t[3, 5].item() == 0.5
    assert np.isnan(res.fpr).all() and not res.tpr.any()
    # all rows bad: nothing but n_bad moves
    bad = torch.tensor([[float("nan"), 1, 1, 1], [float("-inf"), 1, 1, 1], [0.1, 6, 1, 1], [0.1, 1, -1, 1], [0.1, 1, 4, 1], [0.1, 0.5, 1, -1]],
                       dtype=torch.float32, device="cuda")
    before = ds.last_t
    out = ds.add_run(bad, labels=torch.zeros(6, dtype=torch.bool), keep=(8, 1.0))
    res2 = ds.result()
    assert (int(out["n"]), int(out["n_bad"]), out["mask"].tolist(), res2.n_bad) == (0, 6, [False] * 6, 6)
    assert np.array_equal(res2.hist, res.hist) and torch.equal(ds.last_t, before)
    # a 1 x 1 sensor has no neighbours: every age is +inf and everything lands in bin T
    one = sweep(1, 1, taus)
    rows = torch.zeros((300, 4), dtype=torch.float32, device="cuda")
    rows[:, 0] = torch.arange(300, device="cuda") * 1e-3
    lab = torch.arange(300) % 3 == 0
    out = one.add_run(rows, labels=lab, keep=(1, 1e9))
    res = one.result()
    assert not out["mask"].any() and res.hist[:, :, :2].sum() == 0
    assert res.hist[:, 1, 2].tolist() == [100] * 8 and res.hist[:, 0, 2].tolist() == [200] * 8
    assert one.last_t.item() == rows[-1, 0].item()
