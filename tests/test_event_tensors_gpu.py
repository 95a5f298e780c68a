"""v2e_amd.EventTensorizer on the MI355X against the numpy definition (tests/event_tensors_ref.py): count images, voxel grids
and time surfaces, every comparison exact -- the kernels use integer atomics only, so there is nothing to tolerate."""
import numpy as np
import pytest
import torch

from event_tensors_ref import Q, event_tensors, uniform_bounds

pytestmark = pytest.mark.gpu

REPS = ("count", "voxel", "time_surface")
F32 = np.float32


def _explicit_bounds(n_bounds, seed=5):
    """Ascending, unevenly spaced, from -0.25 to 0.75, with one zero-width window when there is room for it."""
    if n_bounds == 2:
        return np.array([-0.25, 0.75])
    rng = np.random.default_rng(seed)
    b = np.sort(np.concatenate(([-0.25, 0.75], rng.uniform(-0.25, 0.75, n_bounds - 2))))
    b[11] = b[10]
    return b


def _make_rows(n, H, W, bounds, seed):
    """n hand-made rows: for a few bounds the float32 value nearest the bound (the bound itself where float32 holds it) and its
    float32 neighbours below and above; random times in two windows out of three (the third stays empty), some before the first
    and after the last bound, negative ones among them; random pixels and polarities; shuffled."""
    rng = np.random.default_rng(seed)
    K = len(bounds) - 1
    special = []
    for k in sorted({0, 1, K // 2, K - 1, K} & set(range(K + 1))):
        f = F32(bounds[k])
        special += [np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))]
    special = np.array(special, F32)[rng.permutation(len(special))][:n]
    m = n - len(special)
    ks = rng.integers(0, K, m)
    ks = np.where(ks % 3 == 1, (ks + 1) % K, ks) if K >= 3 else ks
    t = bounds[ks] + rng.random(m) * (bounds[ks + 1] - bounds[ks])
    out = rng.random(m) < 0.1
    t = np.where(out, np.where(rng.random(m) < 0.5, bounds[0] - 0.05 * rng.random(m), bounds[-1] + 0.05 * rng.random(m)), t)
    rows = np.empty((n, 4), F32)
    rows[:, 0] = np.concatenate((special, t.astype(F32)))
    rows[:, 1] = rng.integers(0, W, n)
    rows[:, 2] = rng.integers(0, H, n)
    rows[:, 3] = rng.integers(0, 2, n) * 2 - 1
    return rows[rng.permutation(n)]


def _mode(mode):
    """-> (constructor arguments, t_end of the clip, n_windows or None)"""
    if mode == "uniform_300":      # bounds that float32 does not hold
        return dict(window_s=1 / 300.0, t_start=-0.25), -0.25 + 299.5 * (1 / 300.0)
    if mode == "uniform_256":      # bounds that float32 holds: a t exactly on a bound
        return dict(window_s=1 / 256.0, t_start=-0.25), -0.25 + 40.5 / 256.0
    if mode == "explicit_2":
        return dict(bounds=_explicit_bounds(2)), 0.75
    return dict(bounds=_explicit_bounds(300)), 0.75


def _clip_bounds(kw, n_windows):
    return uniform_bounds(kw["t_start"], kw["window_s"], n_windows) if "window_s" in kw else np.asarray(kw["bounds"], np.float64)


def _tensorize(kw, H, W, runs, bins=5, reps=REPS, **more):
    """runs: [(rows (numpy), t_end or None), ...] -> (tensorizer, {rep: numpy [K, ...]}, K): every run's output and flush's, joined."""
    from v2e_amd import EventTensorizer
    tz = EventTensorizer(H, W, representations=reps, voxel_bins=bins, **kw, **more)
    parts, nxt = [], 0
    for rows, t_end in runs:
        res = tz.add_run(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), t_end=t_end)
        assert res["windows"][0] == nxt
        nxt += res["windows"][1]
        parts.append(res)
    res = tz.flush()
    assert res["windows"][0] == nxt and res["windows"][1] in (0, 1)
    nxt += res["windows"][1]
    parts.append(res)
    got = {}
    for rep in reps:
        assert all(p[rep].is_cuda and p[rep].shape[0] == p["windows"][1] for p in parts)
        got[rep] = torch.cat([p[rep] for p in parts]).cpu().numpy()
    return tz, got, nxt


def _assert_equal(got, ref, reps=REPS):
    for rep in reps:
        assert got[rep].dtype == ref[rep].dtype and got[rep].shape == ref[rep].shape, rep
        assert np.array_equal(got[rep].view(np.uint32), ref[rep].view(np.uint32)), rep


@pytest.fixture(scope="module")
def big():
    """5000 shuffled rows at 33x37 over 299 uniform windows, and the definition of their tensors (shared, never modified)."""
    kw, t_end = _mode("uniform_300")
    rows = _make_rows(5000, 33, 37, uniform_bounds(kw["t_start"], kw["window_s"], 300), seed=77)
    ref = event_tensors(rows, uniform_bounds(kw["t_start"], kw["window_s"], 300), 33, 37, bins=5)
    return kw, t_end, rows, ref


@pytest.mark.parametrize("bins", [1, 2, 5])
@pytest.mark.parametrize("mode", ["uniform_300", "uniform_256", "explicit_2", "explicit_300"])
@pytest.mark.parametrize("n", [0, 1, 63, 257, 5000])
@pytest.mark.parametrize("hw", [(5, 7), (33, 37)])
def test_hand_made_rows(hw, n, mode, bins):
    H, W = hw
    kw, t_end = _mode(mode)
    n_ref = {"uniform_300": 300, "uniform_256": 41, "explicit_2": 1, "explicit_300": 299}[mode]
    bounds = _clip_bounds(kw, n_ref)
    rows = _make_rows(n, H, W, bounds, seed=n + 7 * bins + H)
    tz, got, K = _tensorize(kw, H, W, [(rows, t_end)], bins=bins)
    assert K == n_ref
    ref = event_tensors(rows, bounds, H, W, bins=bins)
    _assert_equal(got, ref)
    c = tz.check()
    assert c == {"n_bad": 0, "n_before": ref["n_before"], "n_after": ref["n_after"]}
    if n >= 63:
        assert ref["n_before"] > 0 and ref["n_after"] > 0 and ref["count"].sum() > 0
    if n >= 257 and n_ref >= 3:
        assert (ref["count"].reshape(n_ref, -1).sum(1) == 0).any()  # there are empty windows
    assert tz.host_syncs == 1  # check()'s


@pytest.mark.parametrize("mode", ["uniform_300", "explicit_300"])
def test_contention_on_one_pixel(mode):
    """5000 rows on one pixel, one polarity, one window."""
    H, W = 5, 7
    kw, t_end = _mode(mode)
    n_ref = 300 if mode == "uniform_300" else 299
    bounds = _clip_bounds(kw, n_ref)
    rng = np.random.default_rng(3)
    rows = np.empty((5000, 4), F32)
    rows[:, 0] = (bounds[17] + rng.random(5000) * (bounds[18] - bounds[17]) * 0.999).astype(F32)
    rows[:, 1], rows[:, 2], rows[:, 3] = 6, 4, -1
    ref = event_tensors(rows, bounds, H, W)
    assert ref["count"][17, 0, 4, 6] + ref["count"][18, 0, 4, 6] == 5000 and ref["count"][17, 0, 4, 6] >= 4990
    _, got, K = _tensorize(kw, H, W, [(rows, t_end)])
    assert K == n_ref
    _assert_equal(got, ref)


def test_voxel_bins_sum_to_the_polarity_difference(big):
    """Per window and pixel the int64 bin sums are 2^24 * (ON - OFF).  On the device's float32 output that reads: the float64 sum
    of the bins equals ON - OFF wherever float32 holds every bin of the pixel exactly -- a bin that several events share can carry
    more than 24 significant bits (2^24 - q1 of one event plus q1' of another) and is then rounded once, by the finish kernel;
    every pixel with a single event, and most of the others, are exact.  The rounded bins are pinned bit for bit by the definition,
    whose int64 sums are checked here as they stand."""
    kw, t_end, rows, ref = big
    tz, got, K = _tensorize(kw, 33, 37, [(rows, t_end)])
    _assert_equal(got, ref)
    diff = got["count"][:, 1].astype(np.int64) - got["count"][:, 0]
    n_ev = got["count"].astype(np.int64).sum(1)
    assert got["count"].max() < Q and np.abs(diff).sum() > 0 and (n_ev > 1).sum() > 20
    assert np.array_equal(ref["voxel_acc"].sum(1), Q * diff)
    back = np.rint(got["voxel"].astype(np.float64) * Q).astype(np.int64)  # the bins the float32 output holds
    exact = (back == ref["voxel_acc"]).all(1)
    assert exact[n_ev <= 1].all() and exact[n_ev > 1].any() and exact.mean() > 0.99
    assert np.array_equal(got["voxel"].astype(np.float64).sum(1)[exact], diff.astype(np.float64)[exact])
    # and the device's own int64 sums, before any rounding: all rows in one open window, many events per pixel
    from v2e_amd import EventTensorizer
    one = EventTensorizer(33, 37, representations=("count", "voxel"), bounds=[-0.25, 0.76], voxel_bins=5)
    assert one.add_run(torch.from_numpy(rows).cuda(), t_end=0.75)["windows"] == (0, 0)
    w = one.open_window()
    cnt, acc = w["count"].cpu().numpy().astype(np.int64), w["voxel_acc"].cpu().numpy()
    whole = event_tensors(rows, np.array([-0.25, 0.76]), 33, 37)
    assert acc.dtype == np.int64 and cnt.sum() == 5000 - whole["n_before"] - whole["n_after"] > 4000 and cnt.max() >= 4
    assert np.array_equal(acc.sum(0), Q * (cnt[1] - cnt[0]))
    assert np.array_equal(acc, whole["voxel_acc"][0]) and np.array_equal(cnt, whole["count"][0])


@pytest.mark.parametrize("mode", ["uniform_300", "explicit_300"])
def test_split_runs_agree_with_one_run(mode):
    """The clip in one add_run and cut into 3 runs at rows inside a window; every run's end time is read from its last row."""
    H, W = 33, 37
    kw, _ = _mode(mode)
    bounds = _clip_bounds(kw, 300 if mode == "uniform_300" else 299)
    rows = _make_rows(5000, H, W, bounds, seed=11)
    rows = rows[(rows[:, 0] >= bounds[0]) & (rows[:, 0] < bounds[200])]
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    cuts = []
    for c in (len(rows) // 3, 2 * len(rows) // 3):
        while not (np.searchsorted(bounds, rows[c - 1, 0], "right") == np.searchsorted(bounds, rows[c, 0], "right")):
            c += 1  # rows c - 1 and c lie in the same window
        cuts.append(c)
    one_tz, one, K1 = _tensorize(kw, H, W, [(rows, None)])
    parts = [(rows[:cuts[0]], None), (rows[cuts[0]:cuts[1]], None), (rows[cuts[1]:], None)]
    three_tz, three, K3 = _tensorize(kw, H, W, parts)
    assert K1 == K3 and (one_tz.host_syncs, three_tz.host_syncs) == (1, 3)
    _assert_equal(three, one)
    assert torch.equal(one_tz.surface_state().view(torch.int32), three_tz.surface_state().view(torch.int32))
    ref = event_tensors(rows, bounds[:K1 + 1], H, W)
    _assert_equal(one, ref)
    assert np.array_equal(one_tz.surface_state().cpu().numpy().view(np.uint32), ref["time_surface"][-1].view(np.uint32))
    assert one_tz.check() == three_tz.check() == {"n_bad": 0, "n_before": 0, "n_after": 0}


def test_tiny_scratch_budget_cuts_the_voxel_windows_into_blocks(big):
    from v2e_amd.tensors import plan_windows
    kw, t_end, rows, ref = big
    plane = 8 * 5 * 33 * 37
    budget = 120 * plane + 5
    blocks = plan_windows(t_end, 0, voxel_plane_bytes=plane, max_scratch_bytes=budget, **kw)[2]
    assert len(blocks) == 3
    tz, got, _ = _tensorize(kw, 33, 37, [(rows, t_end)], max_scratch_bytes=budget)
    assert tz.scatter_launches == 3
    whole_tz, whole, _ = _tensorize(kw, 33, 37, [(rows, t_end)])
    assert whole_tz.scatter_launches == 1
    _assert_equal(got, whole)
    _assert_equal(got, ref)
    assert tz.check() == whole_tz.check()  # the re-reads of the rows count nothing twice


@pytest.mark.parametrize("hw,guard", [((5, 7), 3), ((32, 36), 4), ((32, 36), 1)])
def test_bad_rows_are_counted_and_write_nothing(hw, guard):
    """Rows with x = W, y = -1, p = 0 (and worse) among good ones: outputs as without them, n_bad exact, check() raises, and the
    guard elements around caller-supplied outputs stay intact (guard 4: the 16-byte path, 1 and 3: outputs off the 16-byte grid)."""
    from v2e_amd import EventTensorizer
    from v2e_amd.tensors import plan_windows
    H, W = hw
    kw, t_end = _mode("uniform_256")
    bounds = _clip_bounds(kw, 41)
    good = _make_rows(2000, H, W, bounds, seed=21)
    bad = _make_rows(40, H, W, bounds, seed=22)
    bad[0:8, 1] = W
    bad[8:16, 2] = -1
    bad[16:24, 3] = 0
    bad[24:28, 1] = 1e9
    bad[28:32, 2] = -np.inf
    bad[32:34, 1] = np.nan
    bad[34:36, 3] = 2
    bad[36:38, 1] = 0.5
    bad[38:40, 0] = np.nan
    rows = np.concatenate((good, bad))[np.random.default_rng(1).permutation(2040)]
    ref = event_tensors(good, bounds, H, W)
    assert event_tensors(rows, bounds, H, W)["n_bad"] == 40
    nc = plan_windows(t_end, 0, **kw)[0]
    assert nc == 40
    tz = EventTensorizer(H, W, representations=REPS, **kw)
    flat, out = {}, {}
    for rep, ch, dt, fill in (("count", 2, torch.int32, 0x5A5A5A5A), ("voxel", 5, torch.float32, 1234.5), ("time_surface", 2, torch.float32, 1234.5)):
        flat[rep] = torch.full((guard + nc * ch * H * W + guard,), fill, dtype=dt, device="cuda")
        out[rep] = flat[rep][guard:guard + nc * ch * H * W].view(nc, ch, H, W)
    res = tz.add_run(torch.from_numpy(rows).cuda(), t_end=t_end, out=out)
    last = tz.flush()
    assert res["windows"] == (0, nc) and last["windows"] == (nc, 1)
    for rep in REPS:
        assert res[rep].data_ptr() == out[rep].data_ptr()
        g = torch.cat((flat[rep][:guard], flat[rep][-guard:])).cpu()
        assert torch.equal(g, torch.full_like(g, 0x5A5A5A5A if rep == "count" else 1234.5)), rep
    got = {rep: torch.cat((res[rep], last[rep])).cpu().numpy() for rep in REPS}
    _assert_equal(got, ref)
    assert tz.counters() == {"n_bad": 40, "n_before": ref["n_before"], "n_after": ref["n_after"]}
    with pytest.raises(ValueError, match="40 malformed"):
        tz.check()


def test_real_rows_of_a_device_resident_run():
    """The smoke clip (64x96, 6 frames) straight from generate_events_batch(return_device=True) through add_run with frame_times:
    no read-back, and all three representations as the definition gives them for the host copy of the rows."""
    from v2e_amd import EventEmulator, EventTensorizer
    from v2e_amd.synth import int_gradient_frames
    kw = dict(pos_thres=.2, neg_thres=.2, sigma_thres=.03, cutoff_hz=300, leak_rate_hz=.1, shot_noise_rate_hz=2.0, refractory_period_s=.0005)
    frames = int_gradient_frames(6, 64, 96, seed=3, noise=8, as_array=True)
    times = [i / 300 for i in range(6)]
    emu = EventEmulator(device="cuda:0", seed=11, rng_mode="philox", **kw)
    ev, counts = emu.generate_events_batch(frames, times, return_device=True)
    assert ev.is_cuda and ev.shape[0] == int(np.sum(counts)) > 1000
    tz = EventTensorizer(64, 96, representations=REPS, window_s=1 / 600.0, frame_times=times)
    res = tz.add_run(ev, counts)
    last = tz.flush()
    assert tz.host_syncs == 0 and res["windows"] == (0, 10) and last["windows"] == (10, 1)
    got = {rep: torch.cat((res[rep], last[rep])).cpu().numpy() for rep in REPS}
    ref = event_tensors(ev.cpu().numpy(), uniform_bounds(0.0, 1 / 600.0, 11), 64, 96)
    assert ref["count"].sum() == ev.shape[0] - ref["n_after"] and ref["n_before"] == 0
    _assert_equal(got, ref)
    assert tz.check() == {"n_bad": 0, "n_before": 0, "n_after": ref["n_after"]}


def test_two_runs_of_the_same_input_are_bit_equal(big):
    kw, t_end, rows, ref = big
    _, a, _ = _tensorize(kw, 33, 37, [(rows, t_end)])
    _, b, _ = _tensorize(kw, 33, 37, [(rows, t_end)])
    _, c, _ = _tensorize(kw, 33, 37, [(rows[::-1], t_end)])  # and in another order
    _assert_equal(b, a)
    _assert_equal(c, a)
    _assert_equal(a, ref)


def test_add_run_takes_device_rows_only():
    from v2e_amd import EventTensorizer
    tz = EventTensorizer(5, 7, window_s=0.01)
    with pytest.raises(TypeError):
        tz.add_run(np.zeros((3, 4), np.float32), t_end=0.0)
    with pytest.raises(TypeError):
        tz.add_run(torch.zeros((3, 4)), t_end=0.0)
    res = tz.add_run(None, t_end=0.025)  # a run without events still completes windows
    assert res["windows"] == (0, 2) and int(res["count"].sum()) == 0
