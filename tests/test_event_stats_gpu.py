"""v2e_amd.EventStats on the MI355X against the numpy definition (tests/event_stats_ref.py): every integer array, counter, minimum
and map is compared exactly."""
import json
import os

import numpy as np
import pytest
import torch

from denoise_ref import NOISY_DOT_RATE_HZ, labels_from_counts
from event_stats_ref import jsd, pearson, result_dict, same, stats_loop, stats_rows, stats_vectorised
from fixtures import GOLDEN, PhiloxFixture

pytestmark = pytest.mark.gpu

U = 2.0 ** -10
NAN, INF = float("nan"), float("inf")

# ---------------------------------------------------------------------------------------------------------------- crafted rows
W5, H4 = 5, 4
CRAFTED_EDGES = [0.0, 4 * U, 0.25, 1.0]
CRAFTED_BOUNDS = [0.5, 1.0, 1.5, 2.0]
CRAFTED_ROI = ((1, 3), (0, 2))
CRAFTED = np.array([
    [0.25, 1, 1, 1],           # before the first bound; the pixel's first row
    [0.5, 1, 1, -1],           # t on a bound; d = 0.25 exactly on an edge; ON -> OFF
    [0.5, 1, 1, 0],            # the same pixel at an equal t: d = 0; p = 0 is OFF
    [0.5 + 4 * U, 1, 1, 0.5],  # d = 4 U on an edge; p = 0.5 is ON
    [0.375, 1, 1, 1],          # time going backwards
    [NAN, 1, 1, 1], [INF, 2, 2, 1], [-INF, 2, 2, -1],
    [1.0, -1, 1, 1], [1.0, W5, 1, 1], [1.0, 2, 1.5, 1], [1.0, 2, H4, 1],
    [1.0, 0, 0, 1],            # outside the ROI: counted and stamped, nothing else
    [1.25, 0, 0, -1],
    [2.0, 2, 2, 1],            # at the last bound: after
    [2.0 - U, 2, 2, -1],       # the last bin, one unit backwards
    [1.5, 3, 3, 1],            # y outside the ROI
    [1.5, 3, 2, 1],
    [3.0, 3, 2, -1],           # d = 1.5: past every edge
    [-1.0, 2, 0, -1],          # a negative time: t_first
    [1.0, 2, 0, -1],           # d = 2.0 from it
], dtype=np.float32)
CRAFTED_LABELS = np.arange(len(CRAFTED)) % 3 != 1
CRAFTED_COUNTS, CRAFTED_SIGNAL = [5, 0, 6, 10], [2, 0, 0, 10]


def stats(H, W, edges, bounds=None, roi=None, **kw):
    from v2e_amd import EventStats
    return EventStats(H, W, isi_edges=edges, time_bounds=bounds, roi=roi, device="cuda", **kw)


def equal(es, ref):
    """The result and the maps of an EventStats against a reference dict."""
    res = es.result()
    assert res.count.dtype == np.int64 and res.isi_hist.dtype == np.int64 and res.min_isi.dtype == np.float64
    assert es.last_t.dtype == torch.float32 and es.last_p.dtype == torch.int8 and es.last_t.is_cuda
    assert res.n == ref["count"].sum()
    return same(result_dict(res, es.last_t.cpu().numpy(), es.last_p.cpu().numpy()), ref)


def test_crafted_rows():
    rows = torch.from_numpy(CRAFTED).cuda()
    counted = labels_from_counts(CRAFTED_COUNTS, CRAFTED_SIGNAL)
    assert len(counted) == len(CRAFTED) and 0 < counted.sum() < len(counted)
    ref = {key: stats_loop(CRAFTED, H4, W5, CRAFTED_EDGES, CRAFTED_BOUNDS, CRAFTED_ROI, lab)
           for key, lab in (("none", None), ("labels", CRAFTED_LABELS), ("counts", counted))}
    r = ref["labels"]
    assert r["n_bad"] == 7 and r["n_before"] == 3 and r["n_after"] == 2 and r["n_backwards"].sum() == 2 and r["min_isi"].min() == 0
    assert r["t_first"] == -1.0 and r["t_last"] == 3.0 and r["isi_hist"].sum(axis=(0, 1)).tolist() == [2, 1, 1, 1, 2]
    assert r["count"][:, :, 0, 0].sum() == 2 and r["count"][:, :, 3, 3].sum() == 1 and r["count"].sum() == 14

    def run(**kw):
        es = stats(H4, W5, CRAFTED_EDGES, CRAFTED_BOUNDS, CRAFTED_ROI)
        out = es.add_run(rows, **kw)
        assert out["n"].dim() == 0 and out["n"].dtype == torch.int64 and out["n"].is_cuda and out["n_bad"].dim() == 0
        assert (int(out["n"]), int(out["n_bad"])) == (14, 7) and es.passes == 1
        return es
    assert equal(run(), ref["none"])
    assert equal(run(labels=CRAFTED_LABELS), ref["labels"])                                   # host numpy
    assert equal(run(labels=torch.from_numpy(CRAFTED_LABELS)), ref["labels"])                 # host tensor
    assert equal(run(labels=torch.from_numpy(CRAFTED_LABELS).cuda(), counts=[21]), ref["labels"])
    assert equal(run(counts=CRAFTED_COUNTS, frame0=7, n_signal=CRAFTED_SIGNAL), ref["counts"])
    assert equal(run(counts=CRAFTED_COUNTS, frame0=7), ref["none"])                           # counts alone: all signal
    # row by row, the maps carrying everything
    es = stats(H4, W5, CRAFTED_EDGES, CRAFTED_BOUNDS, CRAFTED_ROI)
    for i in range(len(CRAFTED)):
        es.add_run(rows[i:i + 1], labels=CRAFTED_LABELS[i:i + 1])
    assert equal(es, ref["labels"]) and es.passes == len(CRAFTED)


def test_crafted_rows_bad_label_forms_and_empty_runs():
    rows = torch.from_numpy(CRAFTED).cuda()
    es = stats(H4, W5, CRAFTED_EDGES, CRAFTED_BOUNDS, CRAFTED_ROI)
    for kw in (dict(labels=CRAFTED_LABELS, counts=CRAFTED_COUNTS, n_signal=CRAFTED_SIGNAL), dict(n_signal=CRAFTED_SIGNAL),
               dict(counts=[5, 0, 6, 9], n_signal=CRAFTED_SIGNAL), dict(counts=CRAFTED_COUNTS, n_signal=[2, 0, 7, 10]),
               dict(counts=CRAFTED_COUNTS, n_signal=[2, 0, 0]), dict(labels=CRAFTED_LABELS[:-1]),
               dict(labels=CRAFTED_LABELS.astype(np.uint8)), dict(labels=torch.ones((21, 1), dtype=torch.bool, device="cuda"))):
        with pytest.raises(ValueError):
            es.add_run(rows, **kw)
    for empty in (None, rows[:0]):
        out = es.add_run(empty, counts=[0, 0], frame0=3, n_signal=[0, 0])
        assert (int(out["n"]), int(out["n_bad"])) == (0, 0)
    res = es.result()   # nothing was added by any of it
    assert equal(es, stats_loop(CRAFTED[:0], H4, W5, CRAFTED_EDGES, CRAFTED_BOUNDS, CRAFTED_ROI)) and es.passes == 0
    assert (res.n, res.n_bad, res.t_first, res.t_last, res.duration) == (0, 0, None, None, None) and np.isposinf(res.min_isi).all()
    # all rows bad: nothing but n_bad moves
    es.add_run(rows[5:12])
    res = es.result()
    assert (res.n, res.n_bad, res.t_first) == (0, 7, None) and bool(torch.isinf(es.last_t).all()) and not es.last_p.any()
    without = stats(H4, W5, CRAFTED_EDGES, None, CRAFTED_ROI)   # no time bounds: no time histogram
    without.add_run(rows, labels=CRAFTED_LABELS)
    assert without.result().time_hist is None and equal(without, stats_loop(CRAFTED, H4, W5, CRAFTED_EDGES, None, CRAFTED_ROI, CRAFTED_LABELS))


# ----------------------------------------------------------------------------------------------------------------- random rows
RW, RH, RN = 33, 37, 20000
RANDOM_ROI = ((3, 30), (2, 33))
RANDOM_EDGES = {1: [2.0 ** -6], 7: [0.0, U, 3 * U, 2.0 ** -6, 2.0 ** -4, 0.25, 1.0], 256: np.arange(256) * 16 * U}
RANDOM_BOUNDS = {1: [1.0, 20.0], 50: np.arange(51) * 0.5 + 0.25, 1 << 20: np.arange((1 << 20) + 1) * 2.0 ** -15 - 1.0}
_random = {}


def random_case(E, K, seed=11):
    """(rows, labels, reference) of the shared random rows, computed once per table pair."""
    if (E, K, seed) not in _random:
        rows, labels = stats_rows(RH, RW, RN, seed=seed, hot=0.3)
        _random[E, K, seed] = (rows, labels, stats_vectorised(rows, RH, RW, RANDOM_EDGES[E], RANDOM_BOUNDS[K], RANDOM_ROI, labels))
    return _random[E, K, seed]


def test_random_rows_reference_is_the_definition():
    rows, labels, ref = random_case(7, 50)
    assert same(ref, stats_loop(rows, RH, RW, RANDOM_EDGES[7], RANDOM_BOUNDS[50], RANDOM_ROI, labels))
    assert 800 < ref["n_bad"] < 1200 and ref["count"].max() > 100 and ref["n_backwards"].min() > 20
    assert ref["n_after"] > 0 and ref["n_before"] > 0 and (ref["isi_hist"].sum(axis=(0, 1)) > 0).all()


@pytest.mark.parametrize("K", [1, 50, 1 << 20])
@pytest.mark.parametrize("E", [1, 7, 256])
def test_random_rows(E, K):
    rows, labels, ref = random_case(E, K)
    dev_rows, dev_labels = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda()

    def feed(es, cuts):
        for a, b in cuts:
            es.add_run(dev_rows[a:b], labels=dev_labels[a:b])
        return es
    new = lambda **kw: stats(RH, RW, RANDOM_EDGES[E], RANDOM_BOUNDS[K], RANDOM_ROI, **kw)  # noqa: E731
    one, again = feed(new(), [(0, RN)]), feed(new(), [(0, RN)])
    three, blocks = feed(new(), [(0, 1), (1, 7777), (7777, 7777), (7777, RN)]), feed(new(max_rows_per_pass=777), [(0, RN)])
    assert equal(one, ref) and equal(three, ref) and equal(blocks, ref)
    assert (one.passes, three.passes, blocks.passes) == (1, 3, 26)
    assert torch.equal(one._state["acc"], again._state["acc"]) and torch.equal(one.last_t, again.last_t)   # the same call twice: bit-equal
    assert ref["time_hist"].shape == (2, 2, K) and ref["isi_hist"].shape == (2, 4, E + 1)
    # reset, then a second stream: a fresh instance's results
    rows2, labels2, ref2 = random_case(E, K, seed=12)
    blocks.reset()
    assert bool(torch.isinf(blocks.last_t).all()) and not blocks.last_p.any() and blocks.result().n == 0
    blocks.add_run(torch.from_numpy(rows2).cuda(), labels=labels2)
    assert equal(blocks, ref2) and not same(ref, ref2, ("count",))


@pytest.mark.parametrize("K", [300, 8192, 16385])
def test_random_rows_copies_of_the_time_histogram(K):
    """The kernel's workgroups spread their adds over 64, ..., 1 copies of the time histogram, as many as stay within 2^16 cells:
    K = 300 gives 54 copies, 8192 two and 16385 one (K = 1, 50 and 2^20 above: 64, 64 and 1)."""
    from v2e_amd.stats import MAX_TIME_CELLS
    bounds = np.arange(K + 1) * (2.0 ** 15 / K) * U - 1.0
    rows, labels = stats_rows(RH, RW, RN, seed=11, hot=0.3)
    ref = stats_vectorised(rows, RH, RW, RANDOM_EDGES[7], bounds, RANDOM_ROI, labels)
    es = stats(RH, RW, RANDOM_EDGES[7], bounds, RANDOM_ROI)
    assert es._time_replicas() == {300: 54, 8192: 2, 16385: 1}[K] and es._time_replicas() * 4 * K <= max(MAX_TIME_CELLS, 4 * K)
    es.add_run(torch.from_numpy(rows).cuda(), labels=labels)
    assert equal(es, ref) and (ref["time_hist"] > 0).sum() > min(K, 5000)


def test_past_the_rows_kernel_grid_cap():
    """600 000 rows at 97 x 131: more than 2048 workgroups of 256 rows, so the kernel's threads go round their loop again."""
    W, H, n = 97, 131, 600000
    rows, labels = stats_rows(H, W, n, seed=5, unit=2.0 ** -14)
    edges, bounds, roi = RANDOM_EDGES[7], np.arange(51) * 1.0 + 0.5, ((10, 80), (0, 120))
    ref = stats_vectorised(rows, H, W, edges, bounds, roi, labels)
    assert ref["count"].sum() > 2048 * 256 and ref["n_after"] > 0 and (ref["time_hist"].sum(axis=2) > 0).all()
    es = stats(H, W, edges, bounds, roi)
    es.add_run(torch.from_numpy(rows).cuda(), labels=torch.from_numpy(labels).cuda())
    assert equal(es, ref) and es.passes == 1


def test_one_hot_pixel():
    """100 000 rows on a single pixel: one long stretch of the sorted keys and one contended counter per (label, polarity)."""
    n = 100000
    rng = np.random.RandomState(9)
    t = np.cumsum(rng.randint(0, 3, size=n)).astype(np.float64)
    late = rng.rand(n) < 0.02
    t[late] -= rng.randint(1, 9, size=int(late.sum()))
    rows = np.stack([t * 2.0 ** -12, np.full(n, 17), np.full(n, 12), rng.choice([-1.0, 1.0], size=n)], axis=1).astype(np.float32)
    labels = rng.rand(n) < 0.5
    edges, bounds = np.arange(8) * 2.0 ** -12, np.arange(51) * 0.5
    ref = stats_vectorised(rows, RH, RW, edges, bounds, None, labels)
    assert ref["count"].sum() == n == ref["count"][:, :, 12, 17].sum() and ref["n_first"].sum() == 1 and ref["isi_hist"].sum() == n - 1
    es = stats(RH, RW, edges, bounds)
    es.add_run(torch.from_numpy(rows).cuda(), labels=labels)
    assert equal(es, ref)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_golden_time_bins_on_the_device():
    """The reference's histogram_events_in_time_bins(select_events_in_roi(rows)) for polarity 1 and -1, from the device."""
    from v2e_amd import EventStats
    z = np.load(os.path.join(GOLDEN, "event_stats_time_bins.npz"), allow_pickle=False)
    roi = (tuple(int(v) for v in z["roi_x"]), tuple(int(v) for v in z["roi_y"]))
    es = stats(260, 346, [1.0], EventStats.time_bins(float(z["start"]), float(z["stop"]), float(z["time_bin_ms"]) * 0.001), roi)
    es.add_run(torch.from_numpy(z["rows"]).cuda())
    res = es.result()
    assert np.array_equal(res.time_series(1), z["ts_on"]) and np.array_equal(res.time_series(-1), z["ts_off"])
    inside = (z["rows"][:, 1] >= roi[0][0]) & (z["rows"][:, 1] <= roi[0][1]) & (z["rows"][:, 2] >= roi[1][0]) & (z["rows"][:, 2] <= roi[1][1])
    assert res.on_off_counts() == (int((z["rows"][inside, 3] > 0).sum()), int((z["rows"][inside, 3] < 0).sum()))


def noisy_dot(seed_offset=0):
    from v2e_amd import EventEmulator, moving_dot
    fx = PhiloxFixture("philox_moving_dot_64x64")
    z = np.load(os.path.join(GOLDEN, "synth_moving_dot_64x64.npz"), allow_pickle=False)
    src = moving_dot(int(z["W"]), int(z["H"]), arg_list=json.loads(str(z["arg_list"])), device="cuda")
    emu = EventEmulator(device="cuda", seed=fx.seed + seed_offset, rng_mode="philox", **dict(fx.kw, shot_noise_rate_hz=NOISY_DOT_RATE_HZ))
    return src, emu


EMU_EDGES = np.geomspace(1e-5, 10.0, 61)
EMU_BOUNDS = np.arange(0, 0.052, 0.002)
EMU_ROI = ((8, 55), (8, 55))


def emulator_run(block_frames, seed_offset=0):
    """The noisy moving dot through SyntheticToEvents with on_events feeding an EventStats: (the EventStats, rows, counts, n_signal)."""
    from v2e_amd import SyntheticToEvents
    src, emu = noisy_dot(seed_offset)
    es, got = stats(64, 64, EMU_EDGES, EMU_BOUNDS, EMU_ROI), []

    def on_events(ev, cnt, frame0):
        n_signal = emu.last_n_signal
        es.add_run(ev, cnt, frame0, n_signal=n_signal)
        got.append((ev.clone(), np.array(n_signal)))
    _, counts, n = SyntheticToEvents(src, emu, block_frames=block_frames).run(on_events, return_device=True)
    assert n == 500 and len(got) == -(-500 // block_frames)
    return es, torch.cat([g[0] for g in got]), np.asarray(counts), np.concatenate([g[1] for g in got])


def test_emulator_round_trip():
    results = []
    for block_frames in (300, 128):
        es, rows, counts, n_signal = emulator_run(block_frames)
        host = rows.cpu().numpy()
        ref = stats_vectorised(host, 64, 64, EMU_EDGES, EMU_BOUNDS, EMU_ROI, labels_from_counts(counts, n_signal))
        assert equal(es, ref)
        res = es.result()
        assert res.n_bad == 0 and res.n == counts.sum() == rows.shape[0] >= 400
        assert res.count[:, 1].sum() == int(torch.count_nonzero(rows[:, 3] > 0)) and res.count[1].sum() == n_signal.sum()
        assert 0 < n_signal.sum() < counts.sum() and res.isi_hist[0].sum() > 0 and res.isi_hist[1].sum() > 0
        results.append((res, ref))
    assert same(results[0][1], results[1][1])                       # the block size changes nothing
    # another seed's run beside it
    es2, rows2, counts2, n_signal2 = emulator_run(300, seed_offset=1)
    other, (res, ref) = es2.result(), results[0]
    ref2 = stats_vectorised(rows2.cpu().numpy(), 64, 64, EMU_EDGES, EMU_BOUNDS, EMU_ROI, labels_from_counts(counts2, n_signal2))
    assert equal(es2, ref2) and not same(ref, ref2, ("count",))
    got = res.compare(other)
    (x0, x1), (y0, y1) = EMU_ROI
    for pol in (0, 1):
        assert got["time_corr"][pol] == pearson(ref["time_hist"][:, pol].sum(axis=0), ref2["time_hist"][:, pol].sum(axis=0))
        assert got["map_corr"][pol] == pearson(ref["count"][:, pol, y0:y1 + 1, x0:x1 + 1].sum(axis=0),
                                               ref2["count"][:, pol, y0:y1 + 1, x0:x1 + 1].sum(axis=0))
        assert 0 < got["time_corr"][pol] <= 1 and 0 < got["map_corr"][pol] <= 1   # the same dot on the same path
    # (the sum of the divergence's terms is taken in another order than the loop's: a few ulps of float64)
    assert got["isi_jsd"] == pytest.approx(jsd(ref["isi_hist"].sum(axis=(0, 1)), ref2["isi_hist"].sum(axis=(0, 1))), rel=1e-12)
    assert 0 <= got["isi_jsd"] < 0.5
