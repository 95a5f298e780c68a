"""v2e_amd.ThresholdSweep on the MI355X: its counts against the CPU oracle run once per threshold (the contract, literally) and
against this project's own emulator column by column, the ROI's edges, the refractory rule's two paths, repeatability and stream
ordering.  Every comparison is exact equality of int64 arrays.  The clip's own conditions (columns non-zero, distinct, on both
sides of the rule) are pinned by tests/test_threshold_sweep.py."""
import numpy as np
import pytest
import torch

import threshold_sweep_ref as tsr
from v2e_amd import EventEmulator, ThresholdSweep
from v2e_amd.sweep import count_rows_in_roi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _sweep(name, roi=tsr.ROI, thresholds=tsr.THRESHOLDS, **kw):
    model, neg = tsr.CONFIGS[name]
    return ThresholdSweep(37, 33, thresholds, neg, roi=roi, seed=tsr.SEED, device=DEV, **model, **kw)


@pytest.fixture(scope="module")
def clip_dev():
    frames, times = tsr.clip()
    return torch.from_numpy(np.array(frames)).to(DEV), times


def _assert_equal(res, ref):
    assert res.on.dtype == np.int64 and res.off.dtype == np.int64 and res.rule_on.dtype == bool
    print("on  ", res.on.tolist(), "\nref ", ref["on"].tolist(), "\noff ", res.off.tolist(), "\nref ", ref["off"].tolist())
    assert np.array_equal(res.on, ref["on"]) and np.array_equal(res.off, ref["off"])


# 1. against the oracle: T = 11 is no multiple of the column chunk, 37 x 33 = 1221 pixels of neither 64 nor 256
@pytest.mark.parametrize("name", ["defaults", "scalar_f32", "cutoff_f64", "no_jitter", "neg_differs"])
def test_sweep_equals_one_oracle_run_per_threshold(clip_dev, name):
    frames, times = clip_dev
    res = _sweep(name).run(frames, times)
    _assert_equal(res, tsr.reference(name))
    assert not res.rule_on.any()


@pytest.mark.parametrize("cols", [4, 8, 16])
@pytest.mark.parametrize("name", ["defaults", "cutoff_f64"])
def test_every_column_chunk_size_gives_the_same_counts(clip_dev, name, cols):
    frames, times = clip_dev
    _assert_equal(_sweep(name, cols_per_thread=cols).run(frames, times), tsr.reference(name))


# 2. against this project's emulator, column by column, at a size with several workgroups per column chunk
def _emulator_counts(frames, times, pos, neg, roi, **model):
    on, off = [], []
    for p, n in zip(pos, neg):
        emu = EventEmulator(pos_thres=float(p), neg_thres=float(n), rng_mode="philox", seed=tsr.SEED, shot_noise_rate_hz=0.0,
                            device=DEV, **model)
        ev, _ = emu.generate_events_batch(frames, list(times), return_device=True)
        a, b = count_rows_in_roi(ev, roi).cpu().tolist()
        emu.cleanup()
        on.append(a)
        off.append(b)
    return dict(on=np.array(on, np.int64), off=np.array(off, np.int64))


@pytest.mark.parametrize("T", [1, 19])
def test_sweep_equals_the_emulator_column_by_column(T):
    H, W = 97, 131
    frames, times = tsr.make_clip(H, W)
    frames = torch.from_numpy(frames).to(DEV)
    thr = [0.2] if T == 1 else list(np.round(np.linspace(0.14, 0.86, 19), 3))
    roi = ((10, 120), (7, 90))
    model = dict(cutoff_hz=100.0) if T == 19 else {}
    res = ThresholdSweep(H, W, thr, roi=roi, seed=tsr.SEED, device=DEV, **model).run(frames, times)
    ref = _emulator_counts(frames, times, thr, thr, roi, **model)
    assert res.on.shape == (T,) and np.all(res.on > 0) and np.all(res.off > 0)
    _assert_equal(res, ref)


# 3. ROI edges
@pytest.mark.parametrize("roi", [((0, 32), (0, 36)), ((16, 16), (9, 9)), ((0, 32), (20, 20)), ((17, 32), (30, 36)), ((0, 0), (0, 36))],
                         ids=["whole", "pixel", "row", "to_the_corner", "first_column"])
def test_roi_edges(clip_dev, roi):
    frames, times = clip_dev
    res = _sweep("defaults", roi=roi).run(frames, times)
    ref = tsr.reference("defaults", roi)
    _assert_equal(res, ref)
    assert ref["on"].sum() > 0 and ref["off"].sum() > 0


def test_whole_sensor_is_the_default_roi(clip_dev):
    frames, times = clip_dev
    _assert_equal(_sweep("defaults", roi=None).run(frames, times), tsr.reference("defaults", ((0, 32), (0, 36))))


# 4. the refractory rule: speculative columns and recomputed ones
def test_refractory_columns_take_the_path_the_oracle_says(clip_dev):
    frames, times = clip_dev
    sw = _sweep("refractory")
    res = sw.run(frames, times)
    ref = tsr.reference("refractory")
    print("rule_on", res.rule_on.tolist())
    assert np.array_equal(res.rule_on, ref["rule_on"])
    assert res.rule_on.tolist() == [True, True] + [False] * 9 and sw.recomputed_columns == 2
    _assert_equal(res, ref)


def test_refractory_with_scalar_thresholds_never_switches_on(clip_dev):
    frames, times = clip_dev
    res = _sweep("refractory_scalar").run(frames, times)
    assert not res.rule_on.any()
    _assert_equal(res, tsr.reference("refractory_scalar"))


# 5. repeatability and stream ordering
def test_two_runs_are_identical_and_a_run_orders_behind_the_frames_producer():
    frames_h, times = tsr.clip()
    ref = tsr.reference("defaults")
    sw = _sweep("defaults")
    frames = torch.from_numpy(np.array(frames_h)).to(DEV)
    a = sw.run(frames, times)
    b = sw.run(frames, times)
    assert np.array_equal(a.on, b.on) and np.array_equal(a.off, b.off) and np.array_equal(a.rule_on, b.rule_on)
    _assert_equal(a, ref)
    # the frames are produced by kernels on a side stream (a long-running fill first, so that the sweep would read stale bytes if it
    # did not queue up behind them), the sweep is enqueued right behind them with no synchronisation in between
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    src = torch.from_numpy(np.array(frames_h)).to(DEV).to(torch.int16)
    ballast = torch.zeros((64 << 20,), dtype=torch.float32, device=DEV)
    made = torch.zeros(src.shape, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            ballast.add_(1.0)
        made.copy_((src + 7 - 7).to(torch.uint8))
        c = sw.run(made, times)
    _assert_equal(c, ref)
    assert np.array_equal(made.cpu().numpy(), frames_h)


# 6. the arms of k_sweep the smooth clip never reaches (the inputs are pinned by tests/test_threshold_sweep.py)
def _run(frames, times, thresholds, roi, height=37, width=33, neg=None, **kw):
    sw = ThresholdSweep(height, width, thresholds, neg, roi=roi, seed=tsr.SEED, device=DEV, **kw)
    return sw, sw.run(torch.from_numpy(np.array(frames)).to(DEV), times)


AIMED_CASES = [(i, 0) for i in sorted(tsr.INSTANTIATIONS)] + [(i, c) for i in ("f32_pixel", "f64_scalar") for c in (4, 8, 16)]


@pytest.mark.parametrize("instantiation,cols", AIMED_CASES)
def test_aimed_clip_both_fixup_arms_of_the_floor_division(instantiation, cols):
    """`mag -= r0 < 0` and `mag += r0 >= bt` (with r0 == bt) of k_sweep<float|double, *, SCALAR|per-pixel>."""
    inst = tsr.INSTANTIATIONS[instantiation]
    model = inst["model"]
    # sweep.hip: f64 = cutoff_hz > 0, scalar = !(sigma_thres > 0)
    assert (model["cutoff_hz"] > 0) == (inst["state"] == np.float64) and (not model["sigma_thres"] > 0) == inst["scalar"]
    frames, times, thetas = tsr.aimed_clip(instantiation)
    _, res = _run(frames, times, thetas, tsr.WHOLE, refractory_period_s=0.0, cols_per_thread=cols, **model)
    _assert_equal(res, tsr.aimed_reference(instantiation))
    assert not res.rule_on.any()


@pytest.mark.parametrize("t0", [tsr.LEVELS_T0, 0.0], ids=["late_start", "start_at_0"])
@pytest.mark.parametrize("name", ["defaults", "cutoff_f64"])
def test_every_grey_level_at_uneven_intervals_and_a_late_first_frame(name, t0):
    """Levels 0, 20, 21, 255 (the linear branch of lin-log, the ends of the scale), a dt per frame, and t[0] > 0: a non-zero
    dt_over_tau in entry 0 of the frame table, frame 1's interval from time 0 (the t[0] == 0 twin has another reference)."""
    frames, times = tsr.levels_clip(t0)
    _, res = _run(frames, times, tsr.THRESHOLDS, tsr.ROI, **tsr.CONFIGS[name][0])
    _assert_equal(res, tsr.levels_reference(name, t0))


@pytest.mark.parametrize("leak", [True, False], ids=["leak", "no_leak"])
def test_low_pass_clamp_on_some_pixels_of_every_frame(leak):
    """`if (eps > 1.0) eps = 1.0` taken and not taken within one frame."""
    frames, times = tsr.clamp_clip()
    _, res = _run(frames, times, tsr.THRESHOLDS, tsr.ROI, cutoff_hz=tsr.CLAMP_CUTOFF_HZ, **({} if leak else dict(leak_rate_hz=0.0)))
    _assert_equal(res, tsr.clamp_reference(leak))


def test_per_pixel_thresholds_clamped_to_a_hundredth(clip_dev):
    """`tp < 0.01f ? 0.01f : tp` on a third of the pixels."""
    frames, times = clip_dev
    n = tsr.THRES_CLAMP["frames"]
    sw = ThresholdSweep(37, 33, tsr.THRES_CLAMP["thresholds"], roi=tsr.ROI, seed=tsr.SEED, device=DEV, **tsr.THRES_CLAMP["model"])
    _assert_equal(sw.run(frames[:n], times[:n]), tsr.thres_clamp_reference())


@pytest.mark.parametrize("one_pixel", [False, True], ids=["whole", "pixel"])
@pytest.mark.parametrize("hw", tsr.SMALL_SENSORS, ids=lambda hw: "%dx%d" % hw)
def test_sensors_smaller_than_a_wave(hw, one_pixel):
    """`valid` false on most lanes of the only workgroup (1x70 and 67x1: of the last wave that has pixels)."""
    frames, times, roi, ref = tsr.small_sensor_case(hw[0], hw[1], one_pixel)
    _, res = _run(frames, times, tsr.SMALL_THRESHOLDS, roi, height=hw[0], width=hw[1])
    _assert_equal(res, ref)
    assert ref["on"].sum() + ref["off"].sum() > 0


@pytest.mark.parametrize("T,cols", [(16, 16), (17, 16), (4, 4), (5, 4)])
def test_column_count_at_the_chunk_boundary(clip_dev, T, cols):
    """blockIdx.y's last chunk full (T == cols_per_thread) and holding one column (T == cols_per_thread + 1: the other lanes of the
    chunk repeat the last column and add nothing)."""
    frames, times = clip_dev
    idx = [j % len(tsr.THRESHOLDS) for j in range(T)]
    res = _sweep("defaults", thresholds=[tsr.THRESHOLDS[j] for j in idx], cols_per_thread=cols).run(frames, times)
    ref = tsr.reference("defaults")
    _assert_equal(res, dict(on=ref["on"][idx], off=ref["off"][idx]))


@pytest.mark.parametrize("F", [2, 3])
def test_shortest_clips(clip_dev, F):
    """The frame loop run once (no prefetch of a next frame) and twice."""
    frames, times = clip_dev
    _assert_equal(_sweep("defaults").run(frames[:F], times[:F]), tsr.prefix_reference("defaults", F))


def test_refractory_flag_raised_only_by_a_pixel_outside_the_roi():
    """`flags |= 1u << c` by a pixel with in_roi false: the rule depends on the whole frame's M."""
    frames, times = tsr.lone_pixel_clip()
    ref = tsr.lone_pixel_reference()
    sw, res = _run(frames, times, tsr.THRESHOLDS, tsr.ROI, **tsr.CONFIGS["refractory"][0])
    assert np.array_equal(res.rule_on, ref["rule_on"]) and sw.recomputed_columns == int(ref["rule_on"].sum()) == 2
    _assert_equal(res, ref)


def test_recompute_whose_last_block_is_a_single_frame(clip_dev):
    """_recompute_column with F = 33: a block of 32 frames and one of 1."""
    frames, times = clip_dev
    sw = _sweep("refractory")
    res = sw.run(frames[:33], times[:33])
    ref = tsr.prefix_reference("refractory", 33)
    assert np.array_equal(res.rule_on, ref["rule_on"]) and sw.recomputed_columns == int(ref["rule_on"].sum()) == 2
    _assert_equal(res, ref)


@pytest.mark.parametrize("name", sorted(tsr.GENERIC))
def test_quotients_beyond_qmax_take_the_generic_division(name):
    """`!(q0 <= QMAX)`: div_floor on one pixel whose count per frame is 5.8e6 (float32 state) or 1.49e9 (float64 state)."""
    R, theta, model = tsr.GENERIC[name]
    frames, times = tsr.alternating_clip(37, 33, 3)
    roi = ((16, 16), (9, 9))
    _, res = _run(frames, times, [theta], roi, **model)
    _assert_equal(res, tsr.model_sweep(frames, times, [theta], [theta], roi, R))
    assert not res.rule_on.any()


def test_a_waves_total_beyond_32_bits():
    """The per-wave sum of 64 pixels' counts: 4 462 414 848 ON events in the one wave of an 8 x 8 sensor."""
    n, (on, off), _ = tsr.wave_sum_frames()
    frames, times = tsr.alternating_clip(8, 8, n)
    roi = ((0, 7), (0, 7))
    _, res = _run(frames, times, [tsr.WAVE_SUM_THETA], roi, height=8, width=8, **tsr.GENERIC["f32"][2])
    assert (on, off) == tsr.column_model(frames, times, tsr.WAVE_SUM_THETA, tsr.WAVE_SUM_THETA, roi) and on > 2 ** 32
    _assert_equal(res, dict(on=np.array([on]), off=np.array([off])))


def test_calls_on_two_streams_share_the_scratch_and_a_long_clip_regrows_it():
    """g_scratch through the C API: two calls enqueued back to back on two streams (the second one waits for the first one's
    stream before it overwrites the frame table and the thresholds), a third whose 300 frames need more than the 4096 bytes the
    scratch starts with; nothing is read back before all three are enqueued."""
    import ctypes as C
    from v2e_amd import _capi
    H, W = 5, 7
    roi = ((0, W - 1), (0, H - 1))
    lib = _capi.lib()
    calls = [(12, (0.13, 0.2, 0.31)), (20, (0.15, 0.17, 0.25, 0.38, 0.45)), (300, (0.14, 0.6))]
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    P = _capi.SweepParams()
    P.sigma_thres, P.cutoff_hz, P.leak_rate_hz, P.leak_jitter_fraction, P.noise_rate_cov_decades = 0.03, 0.0, 0.1, 0.1, 0.1
    P.refractory_period_s, P.seed, P.cols_per_thread = 0.0, tsr.SEED, 0
    ballast = torch.zeros((64 << 20,), dtype=torch.float32, device=DEV)
    held, refs = [], []
    for F, thr in calls:
        frames, times = tsr.make_clip(H, W, F)
        refs.append(tsr.oracle_sweep(frames, times, thr, thr, roi))
        held.append((torch.from_numpy(frames).to(DEV), np.ascontiguousarray(times), np.array(thr, np.float64),
                     torch.empty((len(thr), 2), dtype=torch.int64, device=DEV), torch.empty((len(thr),), dtype=torch.int32, device=DEV)))
    torch.cuda.synchronize()
    with torch.cuda.device(DEV):
        with torch.cuda.stream(streams[0]):  # the first call queues up behind a long fill: it is still in flight when the second comes
            for _ in range(8):
                ballast.add_(1.0)
        for k, (frames, times, thr, counts, rule) in enumerate(held):
            s = streams[k % 2]
            dp = C.POINTER(C.c_double)
            _capi.check(lib.v2e_thres_sweep(C.c_void_p(frames.data_ptr()), _capi.DT_U8, frames.shape[0], H, W, times.ctypes.data_as(dp),
                                            C.byref(P), thr.ctypes.data_as(dp), thr.ctypes.data_as(dp), len(thr),
                                            (C.c_int * 4)(0, W - 1, 0, H - 1), C.c_void_p(counts.data_ptr()), C.c_void_p(rule.data_ptr()),
                                            C.c_void_p(s.cuda_stream)), "v2e_thres_sweep")
    torch.cuda.synchronize()
    for (frames, times, thr, counts, rule), ref in zip(held, refs):
        c = counts.cpu().numpy()
        print(c.tolist(), ref["on"].tolist(), ref["off"].tolist())
        assert np.array_equal(c[:, 0], ref["on"]) and np.array_equal(c[:, 1], ref["off"]) and not rule.cpu().numpy().any()
        assert ref["on"].sum() > 0 and ref["off"].sum() > 0
