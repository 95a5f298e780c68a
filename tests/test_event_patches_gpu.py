"""v2e_amd.EventPatches on the MI355X against the numpy definition (tests/patches_ref.py): every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from denoise_ref import BORDER_TAUS, NOISY_DOT_RATE_HZ, border_rows
from fixtures import GOLDEN, PhiloxFixture
from patches_ref import patches_serial

pytestmark = pytest.mark.gpu

H5, W7 = 5, 7
KEEPS = ((1, 2.0 ** -10), (3, 2.0 ** -6))
MODES = (("age", None), ("linear", 2.0 ** -6), ("linear", 0.003))
_ref = {}


def border(r, mode, tau):
    """The shared rows and their reference, computed once per (r, mode, tau): (rows, (features, valid, last_t, last_p))."""
    rows, _ = border_rows(H5, W7, 3000)
    if (r, mode, tau) not in _ref:
        _ref[r, mode, tau] = patches_serial(rows, H5, W7, r, mode, tau)
    return rows, _ref[r, mode, tau]


def patches(H, W, r, mode, tau, **kw):
    from v2e_amd import EventPatches
    return EventPatches(H, W, radius=r, mode=mode, tau=0.1 if tau is None else tau, device="cuda", **kw)


def equal(out, ep, ref):
    """Features, valid, n, n_bad and both maps against (features, valid, last_t, last_p) of the reference; inf compares as a value."""
    feat, valid, last_t, last_p = ref
    assert out["features"].dtype == torch.float32 and out["valid"].dtype == torch.bool and out["features"].is_cuda
    assert out["n"].dim() == 0 and out["n"].dtype == torch.int64 and out["n"].is_cuda and out["n_bad"].dim() == 0
    return (np.array_equal(out["features"].cpu().numpy(), feat) and np.array_equal(out["valid"].cpu().numpy(), valid)
            and (int(out["n"]), int(out["n_bad"])) == (int(valid.sum()), int((~valid).sum()))
            and maps_equal(ep, last_t, last_p))


def maps_equal(ep, last_t, last_p):
    assert ep.last_p.dtype == torch.int8 and ep.last_t.dtype == torch.float32
    return np.array_equal(ep.last_t.cpu().numpy(), last_t) and np.array_equal(ep.last_p.cpu().numpy(), last_p)


@pytest.mark.parametrize("mode,tau", MODES)
@pytest.mark.parametrize("r", [1, 2, 3])
def test_borders_and_ties(r, mode, tau):
    rows, ref = border(r, mode, tau)
    P = 2 * r + 1
    ep = patches(H5, W7, r, mode, tau)
    buf = torch.full((3002, 2, P, P), float("nan"), device="cuda")  # an element the kernel skips shows as NaN
    out = ep.add_run(torch.from_numpy(rows).cuda(), out=buf)
    assert out["features"].shape == (3000, 2, P, P) and out["features"].data_ptr() == buf.data_ptr()
    assert equal(out, ep, ref) and ep.passes == 1
    assert bool(torch.isnan(buf[3000:]).all())                      # and nothing behind the rows is touched
    fresh = patches(H5, W7, r, mode, tau).add_run(torch.from_numpy(rows).cuda())  # without out=: a tensor of its own
    assert torch.equal(fresh["features"], out["features"]) and torch.equal(fresh["valid"], out["valid"])


@pytest.mark.parametrize("mode,tau", MODES[:2])
def test_split_invariance(mode, tau):
    rows, ref = border(3, mode, tau)
    dev_rows = torch.from_numpy(rows).cuda()

    def feed(ep, cuts):
        got = [ep.add_run(dev_rows[a:b]) for a, b in cuts]
        out = {"features": torch.cat([g["features"] for g in got]), "valid": torch.cat([g["valid"] for g in got]),
               "n": sum(g["n"] for g in got), "n_bad": sum(g["n_bad"] for g in got)}
        return equal(out, ep, ref)

    one, three, blocks = patches(H5, W7, 3, mode, tau), patches(H5, W7, 3, mode, tau), patches(H5, W7, 3, mode, tau, max_rows_per_pass=257)
    assert feed(one, [(0, 3000)])
    assert feed(three, [(0, 1), (1, 1777), (1777, 1777), (1777, 3000)])
    assert feed(blocks, [(0, 3000)])
    assert (one.passes, three.passes, blocks.passes) == (1, 3, 12)
    blocks.reset()
    assert bool(torch.isinf(blocks.last_t).all()) and not blocks.last_p.any()
    assert feed(blocks, [(0, 3000)])


def test_long_per_pixel_lists():
    """33x37, 70 000 rows, 40 000 of them on one pixel and its eight neighbours (the rows of test_denoise_gpu.long_case, drawn the
    same way, with random +-1 polarities); r = 3, linear, tau 2^-8: row indices pass 2^16 and the stretches searched are thousands
    long.  About 12 % of the entries lie strictly between 0 and 1."""
    H, W, n = 33, 37, 70000
    rng = np.random.RandomState(21)
    hot = rng.rand(n) < 40000 / n
    x = np.where(hot, 17 + rng.randint(-1, 2, size=n), rng.randint(0, W, size=n))
    y = np.where(hot, 12 + rng.randint(-1, 2, size=n), rng.randint(0, H, size=n))
    t = np.cumsum(rng.randint(0, 3, size=n)) * 2.0 ** -14
    p = np.random.RandomState(22).choice([-1.0, 1.0], size=n)
    rows = np.stack([t, x, y, p], axis=1).astype(np.float32)
    ref = patches_serial(rows, H, W, 3, "linear", 2.0 ** -8)
    between = (ref[0][:, 0] > 0) & (ref[0][:, 0] < 1)
    assert ref[1].all() and 0.08 < between.mean() < 0.16 and (ref[0][:, 1] == 1).any() and (ref[0][:, 1] == -1).any()
    ep = patches(H, W, 3, "linear", 2.0 ** -8)
    assert equal(ep.add_run(torch.from_numpy(rows).cuda()), ep, ref)


def noisy_dot_emulator():
    from v2e_amd import EventEmulator
    fx = PhiloxFixture("philox_moving_dot_64x64")
    return fx, EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))


def test_emulator_rows_end_to_end():
    """philox_moving_dot_64x64 with shot_noise_rate_hz = 5 in two device-resident runs: the patches of each run, the maps carried
    from the first to the second, against the reference on the gathered host rows; and the labels that go with them."""
    from v2e_amd import frame_labels
    fx, emu = noisy_dot_emulator()
    ep = patches(64, 64, 3, "linear", 0.003)
    host, feats, valid, all_counts, all_signal = [], [], [], [], []
    for a, b in ((0, 260), (260, 500)):
        rows, counts = emu.generate_events_batch(fx.frames[a:b], fx.times[a:b], return_device=True)
        out = ep.add_run(rows, counts, a)
        host.append(rows.cpu().numpy())
        feats.append(out["features"])
        valid.append(out["valid"])
        all_counts.append(np.array(counts))
        all_signal.append(np.array(emu.last_n_signal))
    counts, n_signal = np.concatenate(all_counts), np.concatenate(all_signal)
    ref = patches_serial(np.concatenate(host), 64, 64, 3, "linear", 0.003)
    assert ref[1].all() and len(ref[1]) == counts.sum() >= 400
    assert np.array_equal(torch.cat(feats).cpu().numpy(), ref[0]) and bool(torch.cat(valid).all()) and maps_equal(ep, ref[2], ref[3])
    inside = (ref[0][:, 0] > 0) & (ref[0][:, 0] < 1)
    assert inside.any() and (ref[0][:, 1] == 1).any() and (ref[0][:, 1] == -1).any()
    labels = frame_labels(counts, n_signal, device="cuda")
    assert labels.is_cuda and labels.shape == (counts.sum(),) and int(labels.sum()) == n_signal.sum() and 0 < n_signal.sum() < counts.sum()


def test_callback_feed_equals_one_call():
    """The clip through SyntheticToEvents' callback in blocks of 300 frames (500 frames: one boundary) against one call on the
    gathered rows."""
    from v2e_amd import SyntheticToEvents, moving_dot
    fx, emu = noisy_dot_emulator()
    z = np.load(os.path.join(GOLDEN, "synth_moving_dot_64x64.npz"), allow_pickle=False)
    src = moving_dot(int(z["W"]), int(z["H"]), arg_list=json.loads(str(z["arg_list"])), device="cuda")
    fed, got = patches(64, 64, 3, "linear", 0.003), []

    def on_events(ev, cnt, frame0):
        out = fed.add_run(ev, cnt, frame0)
        got.append((ev.clone(), len(cnt), out["features"], out["valid"]))
    _, counts, n = SyntheticToEvents(src, emu, block_frames=300).run(on_events, return_device=True)
    assert n == 500 and [g[1] for g in got] == [300, 200]
    rows = torch.cat([g[0] for g in got])
    whole = patches(64, 64, 3, "linear", 0.003)
    out = whole.add_run(rows)
    assert rows.shape[0] == counts.sum() >= 400 and int(out["n"]) == rows.shape[0]
    assert torch.equal(torch.cat([g[2] for g in got]), out["features"]) and torch.equal(torch.cat([g[3] for g in got]), out["valid"])
    assert torch.equal(fed.last_t, whole.last_t) and torch.equal(fed.last_p, whole.last_p)
    # the same object as the callback itself: the signature is on_events'
    direct = patches(64, 64, 3, "linear", 0.003)
    src = moving_dot(int(z["W"]), int(z["H"]), arg_list=json.loads(str(z["arg_list"])), device="cuda")
    SyntheticToEvents(src, noisy_dot_emulator()[1], block_frames=300).run(direct.add_run, return_device=True)
    assert direct.passes == 2 and torch.equal(direct.last_t, whole.last_t) and torch.equal(direct.last_p, whole.last_p)


def test_cross_module_check_against_denoise_sweep():
    """r = 1, mode "age": the k-th smallest non-centre age against tau is DenoiseSweep's keep mask."""
    from v2e_amd import DenoiseSweep
    rows, _ = border(1, "age", None)
    dev_rows = torch.from_numpy(rows).cuda()
    out = patches(H5, W7, 1, "age", None).add_run(dev_rows)
    ages = out["features"][:, 0].reshape(-1, 9)[:, [0, 1, 2, 3, 5, 6, 7, 8]].sort(dim=1)[0]
    for k, tau in KEEPS:
        mask = DenoiseSweep(H5, W7, BORDER_TAUS, device="cuda").add_run(dev_rows, keep=(k, tau))["mask"]
        assert torch.equal(out["valid"] & (ages[:, k - 1] <= tau), mask) and 0 < int(mask.sum()) < 2902


def test_degenerate_inputs():
    inf = float("inf")
    ep = patches(4, 6, 3, "age", None)
    for empty in (None, torch.zeros((0, 4), dtype=torch.float32, device="cuda")):
        out = ep.add_run(empty, counts=[0, 0], frame0=3)
        assert out["features"].shape == (0, 2, 7, 7) and out["features"].dtype == torch.float32 and out["features"].is_cuda
        assert out["valid"].shape == (0,) and out["valid"].dtype == torch.bool and (int(out["n"]), int(out["n_bad"])) == (0, 0)
    assert ep.passes == 0 and bool(torch.isinf(ep.last_t).all()) and not ep.last_p.any()
    # one row: all entries none
    out = ep.add_run(torch.tensor([[0.5, 5.0, 3.0, -1.0]], device="cuda"))
    assert bool((out["features"][:, 0] == inf).all()) and not out["features"][:, 1].any() and out["valid"].tolist() == [True]
    assert (int(out["n"]), int(out["n_bad"])) == (1, 0) and ep.last_t[3, 5].item() == 0.5 and ep.last_p[3, 5].item() == -1
    assert int(torch.isfinite(ep.last_t).sum()) == 1 and int((ep.last_p != 0).sum()) == 1
    # all rows bad: nothing but n_bad moves
    bad = torch.tensor([[float("nan"), 1, 1, 1], [-inf, 1, 1, 1], [0.1, 6, 1, 1], [0.1, 1, -1, 1], [0.1, 1, 4, 1], [0.1, 0.5, 1, -1]],
                       dtype=torch.float32, device="cuda")
    before_t, before_p = ep.last_t, ep.last_p
    for mode, none0 in (("age", inf), ("linear", 0.0)):
        other = patches(4, 6, 3, mode, 0.1)
        out = other.add_run(bad, out=torch.full((6, 2, 7, 7), float("nan"), device="cuda"))
        assert (int(out["n"]), int(out["n_bad"]), out["valid"].tolist()) == (0, 6, [False] * 6)
        assert bool((out["features"][:, 0] == none0).all()) and bool((out["features"][:, 1] == 0).all())
        assert bool(torch.isinf(other.last_t).all()) and not other.last_p.any()
    out = ep.add_run(bad)
    assert int(out["n_bad"]) == 6 and torch.equal(ep.last_t, before_t) and torch.equal(ep.last_p, before_p)
    # a 1 x 1 sensor: only the centre entry can ever be finite
    rows = torch.zeros((300, 4), dtype=torch.float32, device="cuda")
    rows[:, 0] = torch.arange(300, device="cuda") * 2.0 ** -10
    rows[:, 3] = torch.where(torch.arange(300, device="cuda") % 3 == 0, 1.0, -1.0)
    for r in (1, 3):
        one = patches(1, 1, r, "age", None)
        f = one.add_run(rows)["features"]
        centre = torch.zeros((2 * r + 1, 2 * r + 1), dtype=torch.bool, device="cuda")
        centre[r, r] = True
        assert bool((f[:, 0][:, ~centre] == inf).all()) and not f[:, 1][:, ~centre].any()
        assert f[0, 0, r, r].item() == inf and bool((f[1:, 0, r, r] == 2.0 ** -10).all()) and torch.equal(f[1:, 1, r, r], rows[:-1, 3])
        assert one.last_t.item() == rows[-1, 0].item() and one.last_p.item() == -1
    # a sensor smaller than the patch
    rng = np.random.RandomState(4)
    small = np.stack([np.cumsum(rng.randint(0, 3, size=500)) * 2.0 ** -10, rng.randint(0, 3, size=500), rng.randint(0, 2, size=500),
                      rng.choice([-1.0, 1.0], size=500)], axis=1).astype(np.float32)
    for mode, tau in MODES[:2]:
        ep = patches(2, 3, 3, mode, tau)
        assert equal(ep.add_run(torch.from_numpy(small).cuda()), ep, patches_serial(small, 2, 3, 3, mode, tau))


def test_output_argument_checks(monkeypatch):
    """out= and max_output_bytes: ValueError before anything is allocated or the library is touched."""
    from v2e_amd import EventPatches, _capi

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    rows = torch.zeros((6, 4), device="cuda")
    monkeypatch.setattr(_capi, "lib", touched)
    monkeypatch.setattr(EventPatches, "_dev", touched)
    ep = EventPatches(4, 6, radius=2, device="cuda", max_output_bytes=6 * 2 * 25 * 4 - 1)
    with pytest.raises(ValueError, match="split the call or pass out="):
        ep.add_run(rows)
    for out in (torch.zeros((6, 2, 5, 5)), torch.zeros((5, 2, 5, 5), device="cuda"), torch.zeros((6, 2, 7, 7), device="cuda"),
                torch.zeros((6, 2, 5, 5), device="cuda", dtype=torch.float64), torch.zeros((6, 2, 5, 10), device="cuda")[..., ::2],
                np.zeros((6, 2, 5, 5), np.float32)):
        with pytest.raises(ValueError):
            ep.add_run(rows, out=out)
    with pytest.raises(AssertionError):  # a fitting out= passes every check, whatever max_output_bytes says
        ep.add_run(rows, out=torch.zeros((8, 2, 5, 5), device="cuda"))
