"""CPU-only: the two numpy statements of EventStats' definition agree (tests/event_stats_ref.py), the shared rows reach every branch
of it, the golden time bins of the reference come out of the definition, and the host side of v2e_amd/stats.py: argument checks
(all raised before the library or a device is touched), time_bins, EventStatsResult and its compare, and the ctypes table."""
import math
import os

import numpy as np
import pytest
import torch

from event_stats_ref import jsd, pearson, same, stats_loop, stats_rows, stats_vectorised
from fixtures import GOLDEN

U = 2.0 ** -10
EDGES = [0.0, U, 3 * U, 2.0 ** -6, 2.0 ** -4]
BOUNDS = np.arange(-8, 3000, 64) * U


def host_result(ref, H, W, edges, bounds=None, roi=None):
    from v2e_amd import EventStatsResult
    return EventStatsResult(H, W, ((0, W - 1), (0, H - 1)) if roi is None else roi, edges, bounds, ref["count"], ref["isi_hist"],
                            ref["time_hist"], ref["n_first"], ref["n_backwards"], ref["n_before"], ref["n_after"], ref["min_isi"],
                            ref["t_first"], ref["t_last"], ref["n_bad"])


@pytest.mark.parametrize("roi", [None, ((1, 5), (0, 3))])
@pytest.mark.parametrize("bounds", [None, BOUNDS])
def test_loop_equals_vectorised(roi, bounds):
    rows, labels = stats_rows(5, 7, 3000)
    for lab in (None, labels):
        assert same(stats_loop(rows, 5, 7, EDGES, bounds, roi, lab), stats_vectorised(rows, 5, 7, EDGES, bounds, roi, lab))
    # with carried maps: the second part of a stream equals the whole, in both statements
    whole = stats_loop(rows, 5, 7, EDGES, bounds, roi, labels)
    a = stats_loop(rows[:1234], 5, 7, EDGES, bounds, roi, labels[:1234])
    for f in (stats_loop, stats_vectorised):
        b = f(rows[1234:], 5, 7, EDGES, bounds, roi, labels[1234:], last_t=a["last_t"], last_p=a["last_p"])
        assert same(b, whole, ("last_t", "last_p"))
        for k in ("count", "isi_hist", "n_first", "n_backwards", "n_bad") + (() if bounds is None else ("time_hist", "n_before", "n_after")):
            assert np.array_equal(np.asarray(a[k]) + np.asarray(b[k]), whole[k]), k
        assert np.array_equal(np.minimum(a["min_isi"], b["min_isi"]), whole["min_isi"])
        assert (min(a["t_first"], b["t_first"]), max(a["t_last"], b["t_last"])) == (whole["t_first"], whole["t_last"])


def test_shared_rows_reach_every_branch():
    """What tests/test_event_stats_gpu.py relies on, counted on the loop."""
    rows, labels = stats_rows(5, 7, 3000)
    r = stats_loop(rows, 5, 7, EDGES, BOUNDS, ((1, 5), (0, 3)), labels)
    assert r["n_bad"] > 100 and r["count"].sum() == 3000 - r["n_bad"] and (r["count"].sum(axis=(2, 3)) > 0).all()
    assert (r["isi_hist"].sum(axis=2) > 0).all() and (r["isi_hist"].sum(axis=(0, 1)) > 0).all()   # every transition, every bin (0: d < 0)
    assert (r["n_backwards"] > 0).all() and r["isi_hist"][:, :, 0].sum() == r["n_backwards"].sum()
    assert (r["min_isi"] == 0).sum() >= 4 and np.isfinite(r["min_isi"]).all() and (r["min_isi"] > 0).any()   # equal times at one pixel
    assert r["n_first"].sum() == 5 * 4 and r["n_before"] > 0 and r["n_after"] > 0 and (r["time_hist"].sum(axis=2) > 0).all()
    inside = r["count"][:, :, 0:4, 1:6].sum()
    assert inside == r["n_first"].sum() + r["isi_hist"].sum() == r["n_before"] + r["n_after"] + r["time_hist"].sum() < r["count"].sum()
    assert r["t_first"] < 0 < r["t_last"] or r["t_first"] == 0


def test_golden_time_bins_of_the_reference():
    """histogram_events_in_time_bins(select_events_in_roi(rows)) of the reference, polarity 1 and -1, equals time_series exactly."""
    from v2e_amd import EventStats
    z = np.load(os.path.join(GOLDEN, "event_stats_time_bins.npz"), allow_pickle=False)
    roi = (tuple(int(v) for v in z["roi_x"]), tuple(int(v) for v in z["roi_y"]))
    bounds = EventStats.time_bins(float(z["start"]), float(z["stop"]), float(z["time_bin_ms"]) * 0.001)
    assert z["rows"].shape == (4000, 4) and z["ts_on"].shape == (len(bounds) - 1, 2) and z["ts_on"].dtype == np.float64
    for f in (stats_loop, stats_vectorised):
        res = host_result(f(z["rows"], 260, 346, [1.0], bounds, roi), 260, 346, [1.0], bounds, roi)
        assert np.array_equal(res.time_series(1), z["ts_on"]) and np.array_equal(res.time_series(-1), z["ts_off"])
        assert np.array_equal(res.time_series(None)[:, 1], z["ts_on"][:, 1] + z["ts_off"][:, 1])
        assert res.n_before > 0 and res.n_after > 0 and z["ts_on"][:, 1].sum() > 500 and res.n == 4000
        assert res.on_off_counts() == (res.count[:, 1, 25:200, 40:301].sum(), res.count[:, 0, 25:200, 40:301].sum())


def test_time_bins():
    from v2e_amd import EventStats
    assert np.array_equal(EventStats.time_bins(0, 3.5, 0.05), np.arange(0, 3.5, 0.05))
    b = EventStats.time_bins(0.25, 1.0, 0.03125)
    assert b.dtype == np.float64 and len(b) == 24 and b[0] == 0.25 and b[-1] == 0.96875
    assert EventStats(4, 6, time_bounds=b).time_bounds is not b
    for bad in ((0, 0.05, 0.05), (1, 0, 0.1)):
        with pytest.raises(ValueError):
            EventStats.time_bins(*bad)


def test_argument_checks(monkeypatch):
    from v2e_amd import EventStats, _capi

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)
    monkeypatch.setattr(EventStats, "_dev", touched)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(isi_edges=[]), dict(isi_edges=np.arange(257.0)), dict(isi_edges=[-1.0, 1.0]), dict(isi_edges=[1.0, 1.0]),
                dict(isi_edges=[2.0, 1.0]), dict(isi_edges=[1.0, inf]), dict(isi_edges=[nan]), dict(time_bounds=[1.0]),
                dict(time_bounds=[]), dict(time_bounds=[0.0, 0.0]), dict(time_bounds=[1.0, 0.5]), dict(time_bounds=[0.0, inf]),
                dict(time_bounds=[nan, 1.0]), dict(time_bounds=np.arange((1 << 20) + 2.0)), dict(roi=((0, 6), (0, 3))),
                dict(roi=((2, 1), (0, 3))), dict(roi=((0, 5), (-1, 3))), dict(roi=((0, 5), (0, 4))), dict(roi=(0, 5)), dict(roi="ab"),
                dict(height=0), dict(width=0), dict(max_rows_per_pass=0), dict(max_rows_per_pass=(1 << 30) + 1)):
        kw = dict(height=4, width=6)
        kw.update(bad)
        with pytest.raises(ValueError):
            EventStats(**kw)
    es = EventStats(4, 6)
    assert (es.height, es.width, es.roi, es.time_bounds, es.passes, es.max_rows_per_pass) == (4, 6, ((0, 5), (0, 3)), None, 0, 1 << 25)
    assert np.array_equal(es.isi_edges, np.geomspace(1e-5, 10.0, 61))
    assert len(EventStats(4, 6, isi_edges=np.arange(256.0), time_bounds=np.arange((1 << 20) + 1.0), roi=((5, 5), (3, 3))).isi_edges) == 256
    assert EventStats(4, 6, isi_edges=[0.0], time_bounds=[-1.0, 0.0]).time_bounds.tolist() == [-1.0, 0.0]
    for r in (torch.zeros((6, 4)), torch.zeros((6, 3)), torch.zeros((6, 4), dtype=torch.float64), np.zeros((6, 4), np.float32), [[0, 0, 0, 0]]):
        with pytest.raises(ValueError):  # host rows, wrong shape, wrong type
            es.add_run(r)
    # the label forms that cannot be (the checks that need device rows: tests/test_event_stats_gpu.py)
    for kw in (dict(labels=np.zeros(0, bool), n_signal=[], counts=[]), dict(n_signal=[0]), dict(counts=[2], n_signal=[3]),
               dict(counts=[2, 1], n_signal=[1]), dict(counts=[1], n_signal=[1]), dict(labels=np.zeros(1, bool)),
               dict(labels=np.zeros(0, np.uint8)), dict(labels=torch.zeros((0, 1), dtype=torch.bool))):
        with pytest.raises(ValueError):
            es.add_run(None, **kw)


def test_result_on_the_host():
    rows, labels = stats_rows(5, 7, 3000)
    roi = ((1, 5), (0, 3))
    ref = stats_loop(rows, 5, 7, EDGES, BOUNDS, roi, labels)
    res = host_result(ref, 5, 7, EDGES, BOUNDS, roi)
    assert res.n == ref["count"].sum() and res.n_bad == ref["n_bad"] and res.count.dtype == np.int64 and res.min_isi.dtype == np.float64
    assert res.duration == float(np.float64(np.float32(ref["t_last"])) - np.float64(np.float32(ref["t_first"]))) > 0
    assert np.array_equal(res.rate_hz(), ref["count"] / res.duration) and np.array_equal(res.rate_hz(2.0), ref["count"] / 2.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            res.rate_hz(bad)
    c = ref["count"]
    assert res.on_off_counts() == (c[:, 1, 0:4, 1:6].sum(), c[:, 0, 0:4, 1:6].sum())
    assert res.on_off_counts(roi=((0, 6), (0, 4))) == (c[:, 1].sum(), c[:, 0].sum())
    assert res.on_off_counts(roi=((2, 2), (3, 3)), label=1) == (c[1, 1, 3, 2], c[1, 0, 3, 2])
    assert res.on_off_counts(label=0) == (c[0, 1, 0:4, 1:6].sum(), c[0, 0, 0:4, 1:6].sum())
    with pytest.raises(ValueError):
        res.on_off_counts(roi=((0, 7), (0, 4)))
    with pytest.raises(ValueError):
        res.on_off_counts(label=2)
    centres = (BOUNDS[:-1] + BOUNDS[1:]) / 2
    for pol, p in ((1, 1), (-1, 0), (0, 0)):
        assert np.array_equal(res.time_series(pol), np.stack([centres, ref["time_hist"][:, p].sum(axis=0).astype(np.float64)], axis=1))
        assert np.array_equal(res.time_series(pol, label=1)[:, 1], ref["time_hist"][1, p])
    assert res.time_series(None).shape == (len(BOUNDS) - 1, 2) and res.time_series(None)[:, 1].sum() == ref["time_hist"].sum()
    with pytest.raises(ValueError):
        res.time_series(2)
    without = host_result(stats_loop(rows, 5, 7, EDGES, None, roi, labels), 5, 7, EDGES, None, roi)
    assert without.time_hist is None and without.time_bounds is None
    with pytest.raises(ValueError):
        without.time_series(1)
    empty = host_result(stats_loop(rows[:0], 5, 7, EDGES), 5, 7, EDGES)
    assert (empty.n, empty.t_first, empty.t_last, empty.duration) == (0, None, None, None) and np.isposinf(empty.min_isi).all()
    with pytest.raises(ValueError):
        empty.rate_hz()


def test_compare_against_the_formulas_written_out():
    roi = ((1, 5), (0, 3))
    rows_a, lab_a = stats_rows(5, 7, 3000, seed=11)
    rows_b, _ = stats_rows(5, 7, 2500, seed=12, unit=2.0 ** -9)
    ra, rb = stats_loop(rows_a, 5, 7, EDGES, BOUNDS, roi, lab_a), stats_loop(rows_b, 5, 7, EDGES, BOUNDS, roi)
    a, b = host_result(ra, 5, 7, EDGES, BOUNDS, roi), host_result(rb, 5, 7, EDGES, BOUNDS, roi)
    got = a.compare(b)
    for pol in (0, 1):
        assert got["time_corr"][pol] == pearson(ra["time_hist"][:, pol].sum(axis=0), rb["time_hist"][:, pol].sum(axis=0))
        assert got["map_corr"][pol] == pearson(ra["count"][:, pol, 0:4, 1:6].sum(axis=0), rb["count"][:, pol, 0:4, 1:6].sum(axis=0))
        assert -1 <= got["time_corr"][pol] <= 1 and -1 <= got["map_corr"][pol] <= 1
    # (the sum of the divergence's terms is taken in another order: a few ulps)
    assert got["isi_jsd"] == pytest.approx(jsd(ra["isi_hist"].sum(axis=(0, 1)), rb["isi_hist"].sum(axis=(0, 1))), rel=1e-12)
    assert 0 < got["isi_jsd"] < 1
    same_stream = a.compare(a)
    assert same_stream["isi_jsd"] == 0 and same_stream["time_corr"] == pytest.approx([1, 1]) and same_stream["map_corr"] == pytest.approx([1, 1])
    # a constant side, and no interval at all: NaN
    one = np.zeros((1, 4), np.float32)
    flat = host_result(stats_loop(one, 5, 7, EDGES, BOUNDS, roi), 5, 7, EDGES, BOUNDS, roi)   # (x = 0: outside the ROI)
    c = a.compare(flat)
    assert all(math.isnan(v) for v in c["time_corr"] + c["map_corr"]) and math.isnan(c["isi_jsd"])
    assert host_result(stats_loop(rows_a, 5, 7, EDGES, None, roi), 5, 7, EDGES, None, roi).compare(
        host_result(stats_loop(rows_b, 5, 7, EDGES, None, roi), 5, 7, EDGES, None, roi))["time_corr"] is None
    for other in (host_result(stats_loop(rows_b, 5, 7, EDGES, BOUNDS), 5, 7, EDGES, BOUNDS),                       # another ROI
                  host_result(stats_loop(rows_b, 5, 7, EDGES[1:], BOUNDS, roi), 5, 7, EDGES[1:], BOUNDS, roi),    # other edges
                  host_result(stats_loop(rows_b, 5, 7, EDGES, BOUNDS[1:], roi), 5, 7, EDGES, BOUNDS[1:], roi),    # other bounds
                  host_result(stats_loop(rows_b, 5, 7, EDGES, None, roi), 5, 7, EDGES, None, roi),                # no bounds
                  host_result(stats_loop(rows_b, 6, 7, EDGES, BOUNDS, roi), 6, 7, EDGES, BOUNDS, roi)):           # another sensor
        with pytest.raises(ValueError):
            a.compare(other)
    with pytest.raises(TypeError):
        a.compare(ra)


def test_ctypes_table_lists_the_entry_points():
    from v2e_amd import _capi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "v2e_amd.h")).read()
    for name, n_args in (("v2e_stats_rows", 27), ("v2e_stats_map_update", 8)):
        assert name in _capi.SIGNATURES and ("int %s(" % name) in header
        assert len(_capi.SIGNATURES[name][1]) == n_args
        assert hasattr(_capi.lib(), name)
