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
