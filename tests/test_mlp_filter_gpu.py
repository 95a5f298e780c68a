"""v2e_amd.MLPFilter on the MI355X against the numpy definition (tests/mlp_filter_ref.py): every comparison is on the float32 bit
patterns, exact."""
import numpy as np
import pytest
import torch

from denoise_ref import NOISY_DOT_RATE_HZ, border_rows, labels_from_counts
from fixtures import PhiloxFixture
from mlp_filter_ref import NAN_BITS, bits, mlp_filter_serial, mlp_scores, random_network
from patches_ref import patches_serial
from tiled_rows import tile_map, tile_rows, wide_width

pytestmark = pytest.mark.gpu

H5, W7 = 5, 7
TAUS = (2.0 ** -6, 0.003)
# what the grid-cap test is sized for (tests/test_mlp_filter.py pins them to v2e_amd/csrc/mlpf.hip)
ROWS_PER_WORKGROUP = 64
MAX_WORKGROUPS = 2048
UNTOUCHED = 0x7FC00123          # a NaN that no kernel writes
_patches = {}


def border_patches(r, tau):
    """The 3000 shared rows and their patches_serial result (features, valid, last_t, last_p), computed once per (r, tau)."""
    rows, _ = border_rows(H5, W7, 3000)
    if (r, tau) not in _patches:
        _patches[r, tau] = patches_serial(rows, H5, W7, r, "linear", tau)
    return rows, _patches[r, tau]


def make(H, W, net, r, tau, **kw):
    from v2e_amd import MLPFilter
    return MLPFilter(H, W, *net, radius=r, tau=tau, device="cuda", **kw)


def dev_bits(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def middle_keep(scores, valid):
    """A keep near the median score: the median of the distinct valid scores, so that at least one row fails and one passes."""
    u = np.unique(scores[valid])
    assert len(u) >= 2
    return float(u[len(u) // 2])


def maps_equal(flt, last_t, last_p):
    assert flt.last_p.dtype == torch.int8 and flt.last_t.dtype == torch.float32
    return np.array_equal(dev_bits(flt.last_t), bits(last_t)) and np.array_equal(flt.last_p.cpu().numpy(), last_p)


def check_types(out, n, mask):
    assert out["scores"].dtype == torch.float32 and out["scores"].is_cuda and out["scores"].shape == (n,)
    assert out["valid"].dtype == torch.bool and out["valid"].shape == (n,)
    assert out["n"].dim() == 0 and out["n"].dtype == torch.int64 and out["n"].is_cuda and out["n_bad"].dim() == 0
    assert (out["mask"] is None) == (not mask) and (not mask or (out["mask"].dtype == torch.bool and out["mask"].shape == (n,)))


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("hidden", [1, 20, 64])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_borders_and_ties(r, hidden, tau):
    rows, (feat, valid, last_t, last_p) = border_patches(r, tau)
    net = random_network(2 * (2 * r + 1) ** 2, hidden, seed=100 * r + hidden)
    scores = mlp_scores(feat, valid, *net)
    keep = middle_keep(scores, valid)
    mask = valid & (scores.astype(np.float64) >= keep)
    flt = make(H5, W7, net, r, tau)
    buf = torch.full((3002,), UNTOUCHED, dtype=torch.int32, device="cuda").view(torch.float32)
    out = flt.add_run(torch.from_numpy(rows).cuda(), keep=keep, out=buf)
    check_types(out, 3000, True)
    assert out["scores"].data_ptr() == buf.data_ptr() and flt.passes == 1
    assert np.array_equal(dev_bits(out["scores"]), bits(scores))
    assert np.array_equal(out["valid"].cpu().numpy(), valid) and np.array_equal(out["mask"].cpu().numpy(), mask)
    assert 0 < mask.sum() < valid.sum() and not mask[~valid].any()            # neither empty nor full
    assert (int(out["n"]), int(out["n_bad"])) == (int(valid.sum()), int((~valid).sum())) == (2902, 98)
    assert (bits(scores[~valid]) == NAN_BITS).all() and maps_equal(flt, last_t, last_p)
    assert (dev_bits(buf[3000:]) == UNTOUCHED).all()                          # nothing behind the rows is touched
    fresh = make(H5, W7, net, r, tau).add_run(torch.from_numpy(rows).cuda())  # without out= and keep=: tensors of its own, no mask
    check_types(fresh, 3000, False)
    assert torch.equal(fresh["scores"].view(torch.int32), out["scores"].view(torch.int32)) and torch.equal(fresh["valid"], out["valid"])


@pytest.mark.parametrize("r", [1, 2, 3])
def test_feature_order_against_event_patches(r):
    """Independent of the reference: a network that passes one input through -- one-hot w1, w2 = 1, no bias -- at a corner, the
    centre and an asymmetric offset of each channel returns the device EventPatches feature at that index where it is positive,
    and 0 elsewhere."""
    from v2e_amd import EventPatches
    rows, _ = border_rows(H5, W7, 3000)
    dev_rows = torch.from_numpy(rows).cuda()
    P = 2 * r + 1
    tau = TAUS[0]
    got = EventPatches(H5, W7, radius=r, mode="linear", tau=tau, device="cuda").add_run(dev_rows)
    feat, valid = got["features"], got["valid"]
    zero, one = np.zeros(1, np.float32), np.ones((1, 1), np.float32)
    for c in (0, 1):
        for dy, dx in ((-r, -r), (0, 0), (r - 1, -r)):
            k = c * P * P + (dy + r) * P + (dx + r)
            w1 = np.zeros((1, 2 * P * P), np.float32)
            w1[0, k] = 1
            out = make(H5, W7, (w1, zero, one, zero), r, tau).add_run(dev_rows)
            f = feat[:, c, dy + r, dx + r]
            want = torch.where(f > 0, f, torch.zeros_like(f))
            assert torch.equal(out["valid"], valid) and int(valid.sum()) == 2902
            assert torch.equal(out["scores"][valid].view(torch.int32), want[valid].view(torch.int32))
            assert bool((dev_bits(out["scores"][~valid]) == NAN_BITS).all())
            assert int((want[valid] > 0).sum()) > 20 and int((want[valid] == 0).sum()) > 20


def test_relu_and_bias_edges():
    """b1 so negative that every h is 0: every valid score is b2.  And exact cancellation, w2 = [+1, -1] on two identical hidden
    units: with tau = 2^-6 and row times that are multiples of 2^-10 every feature is a multiple of 2^-4 in [0, 1]; with weights
    and biases that are multiples of 2^-4 below 2 in size, a_j is a multiple of 2^-8 below 2^8, so h_j is exact in float32, b2 + h
    is exact in float64 and (b2 + h) - h is b2."""
    rows, (feat, valid, last_t, last_p) = border_patches(3, TAUS[0])
    dev_rows = torch.from_numpy(rows).cuda()
    w1, b1, w2, b2 = random_network(98, 20, seed=8)
    dead = make(H5, W7, (w1, np.full(20, -1e6, np.float32), w2, b2), 3, TAUS[0]).add_run(dev_rows)
    assert bool((dev_bits(dead["scores"])[valid] == bits(b2)[0]).all()) and bool((dev_bits(dead["scores"])[~valid] == NAN_BITS).all())
    rng = np.random.RandomState(9)
    unit = rng.randint(-31, 32, size=98).astype(np.float32) / 16
    net = (np.stack([unit, unit]), np.full(2, 0.5, np.float32), np.array([[1.0, -1.0]], np.float32), np.array([0.375], np.float32))
    ref = mlp_scores(feat, valid, *net)
    h = np.maximum(feat.reshape(3000, 98).astype(np.float64) @ unit.astype(np.float64) + 0.5, 0)[valid]
    assert (h > 0).sum() > 500 and (h == 0).sum() > 500 and (ref[valid] == np.float32(0.375)).all()
    flt = make(H5, W7, net, 3, TAUS[0])
    out = flt.add_run(dev_rows, keep=0.375)
    assert np.array_equal(dev_bits(out["scores"]), bits(ref)) and np.array_equal(out["mask"].cpu().numpy(), valid)
    assert maps_equal(flt, last_t, last_p)


def test_tile_edges():
    """1, T - 1, T and T + 1 valid rows, T the rows of a workgroup's tile; and a call whose rows are all bad."""
    from v2e_amd.mlpf import ROWS_PER_WORKGROUP as T
    assert T == ROWS_PER_WORKGROUP
    rows, (_, valid, _, _) = border_patches(3, TAUS[1])
    good = rows[valid]
    net = random_network(98, 20, seed=11)
    for n in (1, T - 1, T, T + 1):
        scores, v, mask, last_t, last_p = mlp_filter_serial(good[:n], H5, W7, 3, TAUS[1], *net, keep=0.0)
        flt = make(H5, W7, net, 3, TAUS[1])
        buf = torch.full((n + 2,), UNTOUCHED, dtype=torch.int32, device="cuda").view(torch.float32)
        out = flt.add_run(torch.from_numpy(good[:n]).cuda(), keep=0.0, out=buf)
        assert v.all() and (int(out["n"]), int(out["n_bad"])) == (n, 0) and bool(out["valid"].all())
        assert np.array_equal(dev_bits(out["scores"]), bits(scores)) and np.array_equal(out["mask"].cpu().numpy(), mask)
        assert (dev_bits(buf[n:]) == UNTOUCHED).all() and maps_equal(flt, last_t, last_p)
    # all rows bad: nothing but n_bad moves
    flt = make(H5, W7, net, 3, TAUS[1])
    flt.add_run(torch.from_numpy(good[:T + 1]).cuda())
    before_t, before_p = flt.last_t, flt.last_p
    bad = torch.from_numpy(np.resize(rows[~valid], (T + 1, 4))).cuda()
    out = flt.add_run(bad, keep=-1e30)
    assert (int(out["n"]), int(out["n_bad"])) == (0, T + 1) and not out["valid"].any() and not out["mask"].any()
    assert bool((dev_bits(out["scores"]) == NAN_BITS).all())
    assert torch.equal(flt.last_t, before_t) and torch.equal(flt.last_p, before_p) and int(torch.isfinite(before_t).sum()) > 10
    # no rows at all
    for empty in (None, torch.zeros((0, 4), dtype=torch.float32, device="cuda")):
        out = flt.add_run(empty, counts=[0, 0], frame0=3, keep=0.0)
        check_types(out, 0, True)
        assert (int(out["n"]), int(out["n_bad"])) == (0, 0) and flt.passes == 2


def test_split_invariance():
    rows, (feat, valid, last_t, last_p) = border_patches(3, TAUS[0])
    net = random_network(98, 20, seed=12)
    scores = mlp_scores(feat, valid, *net)
    dev_rows = torch.from_numpy(rows).cuda()

    def feed(flt, cuts):
        got = [flt.add_run(dev_rows[a:b]) for a, b in cuts]
        assert (sum(int(g["n"]) for g in got), sum(int(g["n_bad"]) for g in got)) == (2902, 98)
        return (np.array_equal(dev_bits(torch.cat([g["scores"] for g in got])), bits(scores))
                and np.array_equal(torch.cat([g["valid"] for g in got]).cpu().numpy(), valid) and maps_equal(flt, last_t, last_p))

    one, three, blocks = make(H5, W7, net, 3, TAUS[0]), make(H5, W7, net, 3, TAUS[0]), make(H5, W7, net, 3, TAUS[0], max_rows_per_pass=257)
    assert feed(one, [(0, 3000)])
    assert feed(three, [(0, 1), (1, 1777), (1777, 1777), (1777, 3000)])
    assert feed(blocks, [(0, 3000)])
    assert (one.passes, three.passes, blocks.passes) == (1, 3, 12)
    blocks.reset()
    assert bool(torch.isinf(blocks.last_t).all()) and not blocks.last_p.any()
    assert feed(blocks, [(0, 3000)])


def test_long_per_pixel_lists():
    """33x37, 70 000 rows, 40 000 of them on one pixel and its eight neighbours: the rows of
    test_event_patches_gpu.test_long_per_pixel_lists, drawn the same way; r = 3, hidden = 20, tau 2^-8.  Row indices pass 2^16."""
    H, W, n = 33, 37, 70000
    rng = np.random.RandomState(21)
    hot = rng.rand(n) < 40000 / n
    x = np.where(hot, 17 + rng.randint(-1, 2, size=n), rng.randint(0, W, size=n))
    y = np.where(hot, 12 + rng.randint(-1, 2, size=n), rng.randint(0, H, size=n))
    t = np.cumsum(rng.randint(0, 3, size=n)) * 2.0 ** -14
    p = np.random.RandomState(22).choice([-1.0, 1.0], size=n)
    rows = np.stack([t, x, y, p], axis=1).astype(np.float32)
    net = random_network(98, 20, seed=13)
    scores, valid, mask, last_t, last_p = mlp_filter_serial(rows, H, W, 3, 2.0 ** -8, *net, keep=0.0)
    assert valid.all() and 0.1 < mask.mean() < 0.9 and len(np.unique(scores)) > 30000
    flt = make(H, W, net, 3, 2.0 ** -8)
    out = flt.add_run(torch.from_numpy(rows).cuda(), keep=0.0)
    assert np.array_equal(dev_bits(out["scores"]), bits(scores)) and np.array_equal(out["mask"].cpu().numpy(), mask)
    assert bool(out["valid"].all()) and maps_equal(flt, last_t, last_p) and flt.passes == 1


def test_second_grid_stride_trip():
    """46 tiles of the border case with 3 guard columns between them, 138 000 rows at 5 x 457 in one pass: more valid rows than
    2048 workgroups of 64 hold, and 45 tiles would not be.  The scores are compared on the device against the base case's, indexed
    by each row's base row."""
    r, tau, K = 3, TAUS[0], 46
    rows, (feat, valid, last_t, last_p) = border_patches(r, tau)
    _, labels = border_rows(H5, W7, 3000)
    net = random_network(98, 20, seed=14)
    scores = mlp_scores(feat, valid, *net)
    keep = middle_keep(scores, valid)
    mask = valid & (scores.astype(np.float64) >= keep)
    wide, _, base_index, _ = tile_rows(rows, labels, W7, K, r)
    Ww = wide_width(W7, K, r)
    n = len(wide)
    assert (n, Ww) == (138000, 457)
    assert (K - 1) * int(valid.sum()) <= MAX_WORKGROUPS * ROWS_PER_WORKGROUP < K * int(valid.sum())
    flt = make(H5, Ww, net, r, tau)
    assert n <= flt.max_rows_per_pass
    out = flt.add_run(torch.from_numpy(wide).cuda(), keep=keep)
    index = torch.from_numpy(base_index).cuda()
    assert flt.passes == 1 and (int(out["n"]), int(out["n_bad"])) == (K * int(valid.sum()), K * int((~valid).sum()))
    assert torch.equal(out["scores"].view(torch.int32), torch.from_numpy(scores).cuda()[index].view(torch.int32))
    assert torch.equal(out["valid"], torch.from_numpy(valid).cuda()[index]) and not valid.all()
    assert torch.equal(out["mask"], torch.from_numpy(mask).cuda()[index]) and 0 < mask.sum() < valid.sum()
    assert np.array_equal(dev_bits(flt.last_t), bits(tile_map(last_t, K, r, -np.inf)))
    assert np.array_equal(flt.last_p.cpu().numpy(), tile_map(last_p, K, r, 0))


def test_emulator_rows_end_to_end():
    """philox_moving_dot_64x64 with shot_noise_rate_hz = 5 in two device-resident runs, each handed to add_run with its counts and
    the emulator's n_signal: scores, mask and the ROC counts of both runs against the reference on the gathered host rows;
    denoise_rows keeps the reference's rows; the final maps are those of an EventPatches fed the same rows."""
    from v2e_amd import EventEmulator, EventPatches, denoise_rows, score_roc
    fx = PhiloxFixture("philox_moving_dot_64x64")
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))
    net = random_network(98, 20, seed=15)
    thresholds = [-4.0, -1.0, 0.0, 0.5, 2.0]
    keep = 0.5
    flt = make(64, 64, net, 3, 0.003, thresholds=thresholds)
    ep = EventPatches(64, 64, radius=3, mode="linear", tau=0.003, device="cuda")
    host, got, kept, kept_counts, all_counts, all_signal = [], [], [], [], [], []
    for a, b in ((0, 260), (260, 500)):
        rows, counts = emu.generate_events_batch(fx.frames[a:b], fx.times[a:b], return_device=True)
        out = flt.add_run(rows, counts, a, n_signal=emu.last_n_signal, keep=keep)
        ep.add_run(rows, counts, a)
        k_rows, k_counts = denoise_rows(rows, counts, out["mask"])
        host.append(rows.cpu().numpy())
        got.append(out)
        kept.append(k_rows.cpu().numpy())
        kept_counts.append(k_counts)
        all_counts.append(np.array(counts))
        all_signal.append(np.array(emu.last_n_signal))
    rows, counts, n_signal = np.concatenate(host), np.concatenate(all_counts), np.concatenate(all_signal)
    scores, valid, mask, last_t, last_p = mlp_filter_serial(rows, 64, 64, 3, 0.003, *net, keep=keep)
    labels = labels_from_counts(counts, n_signal)
    assert valid.all() and len(rows) == counts.sum() >= 400 and 0 < mask.sum() < len(rows) and 0 < labels.sum() < len(rows)
    assert np.array_equal(dev_bits(torch.cat([g["scores"] for g in got])), bits(scores))
    assert np.array_equal(torch.cat([g["mask"] for g in got]).cpu().numpy(), mask)
    assert np.array_equal(bits(np.concatenate(kept)), bits(rows[mask]))
    frame = np.repeat(np.arange(len(counts)), counts)
    assert np.array_equal(np.concatenate(kept_counts), np.bincount(frame[mask], minlength=len(counts)))
    roc = score_roc(torch.from_numpy(scores), torch.from_numpy(labels), thresholds, torch.from_numpy(valid))
    res = flt.result()
    assert res["passed"].dtype == np.int64 and np.array_equal(res["passed"], roc["passed"].numpy())
    assert (res["n_signal"], res["n_noise"]) == (int(labels.sum()), int((~labels).sum()))
    assert np.array_equal(res["tpr"], roc["tpr"].numpy()) and np.array_equal(res["fpr"], roc["fpr"].numpy())
    assert res["passed"][:, 0].sum() > res["passed"][:, -1].sum()
    assert maps_equal(flt, last_t, last_p) and torch.equal(flt.last_t, ep.last_t) and torch.equal(flt.last_p, ep.last_p)
    flt.reset()
    assert not flt.result()["passed"].any() and bool(torch.isinf(flt.last_t).all())


def test_two_instances_on_two_streams():
    rows, (feat, valid, last_t, last_p) = border_patches(3, TAUS[1])
    net = random_network(98, 64, seed=16)
    scores = mlp_scores(feat, valid, *net)
    dev_rows = torch.from_numpy(rows).cuda()
    filters = [make(H5, W7, net, 3, TAUS[1]) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = []
    for flt, s in zip(filters, streams):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            flt.last_t                                                        # (the state is made on the filter's own stream)
            outs.append([flt.add_run(dev_rows[a:b]) for a, b in ((0, 1500), (1500, 3000))])
    for s in streams:
        torch.cuda.current_stream().wait_stream(s)
    a, b = (torch.cat([g["scores"] for g in o]) for o in outs)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(dev_bits(a), bits(scores))
    assert all(maps_equal(f, last_t, last_p) for f in filters)
