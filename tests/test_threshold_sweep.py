"""v2e_amd.ThresholdSweep without a GPU: the threshold estimate against the reference's loop, argument validation (before the
library or the device is needed), and -- with the CPU oracle alone -- the conditions of the test clip that the GPU tests
(tests/test_threshold_sweep_gpu.py) rely on, so that they are not vacuous."""
import numpy as np
import pytest
import torch

import threshold_sweep_ref as tsr
from v2e_amd import EventEmulator, ThresholdSweep, estimate_thresholds
from v2e_amd.sweep import SweepResult


# ------------------------------------------------------------------------------------------------ estimate_thresholds
def _reference_estimate(thresholds, on_counts, off_counts, dvs_on, dvs_off):
    """The threshold loop of dataset_scripts/ddd/ddd_find_thresholds.py:106-158 with the per-threshold counts given: starting
    values -1 and inf, numpy absolute differences, strict `<` for both polarities, the difference arrays filled in step."""
    pos_thres, neg_thres = -1.0, -1.0
    on_diffs = np.full(len(thresholds), np.nan)
    off_diffs = np.full(len(thresholds), np.nan)
    best_pos = best_neg = np.inf
    for k, threshold in enumerate(thresholds):
        d_pos = np.abs(dvs_on - on_counts[k])
        d_neg = np.abs(dvs_off - off_counts[k])
        if d_pos < best_pos:
            best_pos, pos_thres = d_pos, threshold
        if d_neg < best_neg:
            best_neg, neg_thres = d_neg, threshold
        on_diffs[k], off_diffs[k] = d_pos, d_neg
    return pos_thres, neg_thres, on_diffs, off_diffs


ESTIMATE_TABLES = {
    # thresholds, ON counts, OFF counts, recording's ON, OFF
    "interior": ([1.0, 0.8, 0.6, 0.4, 0.2], [10, 40, 90, 200, 900], [12, 35, 100, 260, 1000], 100, 240),
    "tie_first_wins": ([0.5, 0.4, 0.3, 0.2], [80, 120, 120, 80], [90, 110, 95, 105], 100, 100),
    "minimum_at_start": ([1.0, 0.5, 0.25], [500, 900, 2000], [450, 800, 1500], 10, 460),
    "minimum_at_end": ([1.0, 0.5, 0.25], [5, 9, 20], [4, 8, 15], 1000, 14),
    "ascending_order_given": ([0.1, 0.2, 0.3], [300, 200, 100], [310, 190, 120], 200, 150),
    "all_equal": ([0.3, 0.2, 0.1], [7, 7, 7], [7, 7, 7], 7, 9),
    "single": ([0.2], [3], [4], 100, 0),
}


@pytest.mark.parametrize("name", sorted(ESTIMATE_TABLES))
def test_estimate_thresholds_is_the_references_loop(name):
    thr, on, off, dvs_on, dvs_off = ESTIMATE_TABLES[name]
    res = SweepResult(np.array(on, np.int64), np.array(off, np.int64), np.zeros(len(thr), bool))
    pos, neg, on_d, off_d = estimate_thresholds(res, thr, dvs_on, dvs_off)
    rpos, rneg, ron_d, roff_d = _reference_estimate(thr, on, off, dvs_on, dvs_off)
    assert (pos, neg) == (rpos, rneg)
    assert on_d.dtype == np.int64 and off_d.dtype == np.int64
    assert np.array_equal(on_d, ron_d) and np.array_equal(off_d, roff_d)


def test_estimate_thresholds_hand_checked():
    thr, on, off, dvs_on, dvs_off = ESTIMATE_TABLES["tie_first_wins"]
    res = SweepResult(np.array(on, np.int64), np.array(off, np.int64), np.zeros(4, bool))
    pos, neg, on_d, off_d = estimate_thresholds(res, thr, dvs_on, dvs_off)
    assert (pos, neg) == (0.5, 0.3)  # ON: 20, 20, 20, 20 -> the first; OFF: 10, 10, 5, 5 -> the first 5
    assert on_d.tolist() == [20, 20, 20, 20] and off_d.tolist() == [10, 10, 5, 5]
    with pytest.raises(ValueError):
        estimate_thresholds(res, thr[:3], dvs_on, dvs_off)


# ------------------------------------------------------------------------------------------------ argument validation
def test_constructor_validation():
    ThresholdSweep(37, 33, [0.2, 0.3], roi=((3, 28), (5, 30)))
    sw = ThresholdSweep(37, 33, [0.2, 0.3])
    assert sw.roi == ((0, 32), (0, 36)) and np.array_equal(sw.neg_thresholds, sw.thresholds)
    for bad in ([0.2, 0.0], [0.2, -0.1], [float("nan")], [float("inf")], []):
        with pytest.raises(ValueError):
            ThresholdSweep(37, 33, bad)
        with pytest.raises(ValueError):
            ThresholdSweep(37, 33, [0.2] * max(len(bad), 1), bad)
    with pytest.raises(ValueError):  # mismatched lengths
        ThresholdSweep(37, 33, [0.2, 0.3], [0.2])
    for roi in (((0, 33), (0, 36)), ((0, 32), (0, 37)), ((-1, 5), (0, 5)), ((5, 4), (0, 5)), ((0, 5), (9, 8)), (0, 5)):
        with pytest.raises(ValueError):  # outside the sensor, empty, malformed
            ThresholdSweep(37, 33, [0.2], roi=roi)
    with pytest.raises(ValueError):
        ThresholdSweep(37, 33, [0.2], cols_per_thread=5)


def test_run_refuses_host_tensors_and_other_dtypes():
    sw = ThresholdSweep(8, 6, [0.2, 0.3])
    t = [0.0, 1e-3, 2e-3]
    with pytest.raises(ValueError):  # a host tensor
        sw.run(torch.zeros((3, 8, 6), dtype=torch.uint8), t)
    with pytest.raises(ValueError):  # a host array
        sw.run(np.zeros((3, 8, 6), np.uint8), t)
    with pytest.raises(ValueError):  # (dtype is checked after residence: still a ValueError on a host without a GPU)
        sw.run(torch.zeros((3, 8, 6), dtype=torch.float32), t)
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            sw.run(torch.zeros((3, 8, 6), dtype=torch.float32, device="cuda"), t)
        ok = torch.zeros((3, 8, 6), dtype=torch.uint8, device="cuda")
        for bad_t in ([0.0, 1e-3], [0.0, 2e-3, 1e-3], [0.0, 1e-3, 1e-3], [-1e-3, 0.0, 1e-3]):
            with pytest.raises(ValueError):
                sw.run(ok, bad_t)
        with pytest.raises(ValueError):
            sw.run(ok[:1], [0.0])
        with pytest.raises(ValueError):
            sw.run(torch.zeros((3, 6, 8), dtype=torch.uint8, device="cuda"), t)


def test_from_emulator_copies_the_model_and_refuses_what_is_out_of_scope(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    emu = EventEmulator(pos_thres=0.3, neg_thres=0.4, sigma_thres=0.02, cutoff_hz=50.0, leak_rate_hz=0.2, refractory_period_s=1e-3,
                        leak_jitter_fraction=0.05, noise_rate_cov_decades=0.2, seed=9, output_width=33, output_height=37,
                        rng_mode="philox")
    sw = ThresholdSweep.from_emulator(emu, [0.2, 0.3], roi=((1, 2), (3, 4)))
    assert (sw.height, sw.width, sw.roi) == (37, 33, ((1, 2), (3, 4)))
    assert (sw.sigma_thres, sw.cutoff_hz, sw.leak_rate_hz, sw.refractory_period_s, sw.leak_jitter_fraction,
            sw.noise_rate_cov_decades, sw.seed) == (0.02, 50.0, 0.2, 1e-3, 0.05, 0.2, 9)
    assert sw.thresholds.tolist() == [0.2, 0.3]
    sw = ThresholdSweep.from_emulator(EventEmulator(rng_mode="philox"), [0.2], height=8, width=6)
    assert (sw.height, sw.width) == (8, 6)
    with pytest.raises(ValueError):  # no size anywhere
        ThresholdSweep.from_emulator(EventEmulator(rng_mode="philox"), [0.2])
    out_of_scope = [dict(shot_noise_rate_hz=1.0), dict(hdr=True), dict(scidvs=True), dict(cs_lambda_pixels=2.0, cs_tau_p_ms=2.0),
                    dict(cs_lambda_pixels=2.0), dict(photoreceptor_noise=True, shot_noise_rate_hz=1.0, cutoff_hz=10.0)]
    for kw in out_of_scope:
        with pytest.raises(ValueError):
            ThresholdSweep.from_emulator(EventEmulator(rng_mode="philox", **kw), [0.2], height=8, width=6)


def test_sweep_params_layout_matches_the_header():
    import ctypes as C
    import os
    import re
    from v2e_amd._capi import SweepParams
    assert C.sizeof(SweepParams) == 6 * 8 + 8 + 4 + 4 and SweepParams.seed.offset == 48 and SweepParams.cols_per_thread.offset == 56
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "v2e_amd.h")).read()
    body = re.search(r"typedef struct v2e_sweep_params \{(.*?)\} v2e_sweep_params;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [name for name, _ in SweepParams._fields_]


# ------------------------------------------------------------------------------------------------ the test clip, by the oracle alone
def test_clip_is_the_documented_one():
    frames, times = tsr.clip()
    assert frames.shape == (40, 37, 33) and frames.dtype == np.uint8 and times[3] == 3e-3
    assert 37 * 33 % 64 != 0 and len(tsr.THRESHOLDS) % 4 != 0 and len(tsr.THRESHOLDS) % 8 != 0  # no multiple of wave, workgroup, chunk
    ref = tsr.reference("defaults")
    j06, j013 = tsr.THRESHOLDS.index(0.6), tsr.THRESHOLDS.index(0.13)
    assert (ref["on"][j06], ref["off"][j06]) == (352, 410)
    assert (ref["on"][j013], ref["off"][j013]) == (4888, 4885)


@pytest.mark.parametrize("name", sorted(tsr.CONFIGS))
def test_clip_conditions_the_gpu_tests_rely_on(name):
    ref = tsr.reference(name)
    on, off = ref["on"], ref["off"]
    assert np.all(on > 0) and np.all(off > 0), "a column without events checks nothing"
    cols = {(int(a), int(b)) for a, b in zip(on, off)}
    assert len(cols) == len(on), "two columns with the same counts could be swapped unnoticed"
    # FrameCtl's tables cover iteration counts up to 32: the emulator the sweep is compared with stays in its ordinary range
    assert ref["max_m"].max() <= 32
    if name in ("defaults", "scalar_f32", "cutoff_f64", "no_jitter"):
        assert np.all(np.diff(on) < 0) and np.all(np.diff(off) < 0)  # counts fall strictly as the threshold rises
    if "refractory" not in name:
        assert not ref["rule_on"].any()


def test_refractory_clip_has_columns_on_both_sides_of_the_rule():
    ref = tsr.reference("refractory")
    assert ref["rule_on"].tolist() == [True, True] + [False] * 9  # 0.13 and 0.15; never from 0.17 up
    assert ref["rule_on"].sum() >= 2 and (~ref["rule_on"]).sum() >= 2
    assert ref["max_m"][:2].max() <= 32
    assert not tsr.reference("refractory_scalar")["rule_on"].any()
    # the rule changes what a rule-on column emits: the recomputed columns are compared with something the speculation would miss
    plain = tsr.reference("defaults")
    # (at 0.13 the rule filters events: 4838 / 4838 with it, 4888 / 4885 without; at 0.15 it is on for a frame and filters nothing)
    assert (ref["on"][0], ref["off"][0]) == (4838, 4838) and (plain["on"][0], plain["off"][0]) == (4888, 4885)
    assert all((ref["on"][j], ref["off"][j]) == (plain["on"][j], plain["off"][j]) for j in range(2, 11))
