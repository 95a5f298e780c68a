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


# ------------------------------------------------------------------------------------------------ the aimed inputs, by the oracle alone
import chain_dtypes as cd  # noqa: E402


def _aimed_stats(instantiation):
    """Over all columns and frames of aimed_clip, from the oracle's planes around each frame (one oracle run per column): the
    pixel-frame-columns whose reciprocal estimate is one too large, one too small, one too small on an exact multiple (r0 == bt),
    and the ON / OFF split of all of them."""
    from oracle import oracle as orc
    inst = tsr.INSTANTIATIONS[instantiation]
    R = inst["state"]
    frames, times, thetas = tsr.aimed_clip(instantiation)
    tot = dict(n=0, fires=0, large=0, small=0, small_exact=0, on=0, off=0)
    for th in thetas:
        def watch(k, before, ora):
            # the divisors as the instantiation holds them: the Python double (in float32 state: rounded to it), or the float32 plane
            pt, nt = (th, th) if inst["scalar"] else (ora.pos_thres_arr, ora.neg_thres_arr)
            leak = tsr.aimed_leak(inst["model"], times, k, np.broadcast_to(np.float32(pt), before.shape))
            am, t, pos = cd.frame_quotients(before, ora.lp_log_frame, pt, nt, R, leak=leak)
            off = cd.estimate_off_by_one(am, t, R)
            zero = cd.remainder_zero(am, t, R)
            # the predicate's floor is the oracle's count
            assert np.array_equal(cd.estimate(am, t, R) - off, np.where(pos, ora.last["pos_cnt"], ora.last["neg_cnt"]))
            tot["n"] += am.size
            tot["fires"] += int((am >= t).sum())
            tot["large"] += int((off == 1).sum())
            tot["small"] += int((off == -1).sum())
            tot["small_exact"] += int(((off == -1) & zero).sum())
            tot["on"] += int(((off != 0) & pos).sum())
            tot["off"] += int(((off != 0) & ~pos).sum())

        kw = dict(pos_thres=th, neg_thres=th, shot_noise_rate_hz=0.0, refractory_period_s=0.0, **inst["model"])
        out = cd.oracle_run(orc, kw, frames, list(times), seed=tsr.SEED, watch=watch)
        assert out["state"] == R
        if not inst["scalar"]:  # sigma_thres selects the per-pixel kernel and leaves every threshold at the aimed value
            pt = orc.OracleEmulator(seed=tsr.SEED, rng_mode="philox", **kw)
            pt.generate_events(frames[0], float(times[0]))
            assert np.all(pt.pos_thres_arr == np.float32(th)) and np.all(pt.neg_thres_arr == np.float32(th))
    return tot


# measured at 33 x 37, 8 frames, 12 columns = 102 564 pixel-frame-columns per instantiation (asked of each: at least 20):
#                 fire     too large   too small   too small, r0 == bt   ON / OFF of those
#   f32_scalar    69 433   2 745       13 591      13 591                8 716 / 7 620
#   f32_pixel     69 433   2 745       13 591      13 591                8 716 / 7 620
#   f64_scalar    75 783   1 436       19 300      19 300                10 888 / 9 848
#   f64_pixel     82 670   258         13 224      13 224                6 133 / 7 349      (with AIM_LEAK; 0 too large without)
AIMED_FLOOR = 20


@pytest.mark.parametrize("instantiation", sorted(tsr.INSTANTIATIONS))
def test_aimed_clip_reaches_both_fixup_arms(instantiation):
    """The table above.  Every estimate that is too small sits on an exact multiple: theta = d / n was chosen so.

    k_sweep<double, *, false> (float32 thresholds, float64 state) needs a device of its own for `mag -= r0 < 0`: the estimate
    fl(am * fl(1 / theta)) is one too large only if am lies below a multiple m theta by less than about m theta 2^-52.  Without a
    leak am is a sum of float32 values (lin-log levels and steps fl32(count * theta), all of magnitude 0.05 .. 5.6) and m theta a
    small multiple of a float32 value, so both are multiples of 2^-28 and differ by 0 or by at least 2^-28 > 5.6 * 2^-52: the arm
    cannot be reached (measured: 0).  AIM_LEAK moves the base by about one unit in its last place per frame, which is that close;
    the predicate then takes the frame's leak step off the base, and its floor still is the oracle's count."""
    inst = tsr.INSTANTIATIONS[instantiation]
    frames, times, thetas = tsr.aimed_clip(instantiation)
    assert frames.shape == (tsr.AIM_FRAMES, 37, 33) and frames.dtype == np.uint8 and len(thetas) <= 12 and times[0] > 0
    assert len(set(thetas)) == len(thetas) and min(thetas) >= 0.05 and max(thetas) <= 1.0
    assert (inst["model"]["cutoff_hz"] > 0) == (inst["state"] == np.float64) and (inst["model"]["sigma_thres"] > 0) == (not inst["scalar"])
    if inst["state"] == np.float64:  # eps clamps at every level, in every frame
        assert tsr.clamp_eps(np.zeros((len(times), 1, 1), np.uint8), times, inst["model"]["cutoff_hz"]).min() > 2.0
    tot = _aimed_stats(instantiation)
    print(instantiation, tot)
    assert tot["small"] >= AIMED_FLOOR and tot["small_exact"] >= AIMED_FLOOR
    assert tot["on"] >= AIMED_FLOOR and tot["off"] >= AIMED_FLOOR
    assert tot["large"] >= AIMED_FLOOR
    ref = tsr.aimed_reference(instantiation)
    assert np.all(ref["on"] > 0) and np.all(ref["off"] > 0) and not ref["rule_on"].any()
    assert len({(int(a), int(b)) for a, b in zip(ref["on"], ref["off"])}) == len(thetas)


def test_column_model_is_the_oracle_where_both_can_run():
    """column_model (float32 state) on the existing clip's scalar_f32 configuration, all 11 columns, and on the scalar float32
    aimed clip; its float64 form on the scalar float64 aimed clip (eps clamped: lp == L).  It may then stand in for the oracle."""
    frames, times = tsr.clip()
    ref = tsr.reference("scalar_f32")
    got = tsr.model_sweep(frames, times, tsr.THRESHOLDS, tsr.THRESHOLDS, tsr.ROI)
    assert np.array_equal(got["on"], ref["on"]) and np.array_equal(got["off"], ref["off"])
    for instantiation, R in (("f32_scalar", np.float32), ("f64_scalar", np.float64)):
        frames, times, thetas = tsr.aimed_clip(instantiation)
        ref = tsr.aimed_reference(instantiation)
        got = tsr.model_sweep(frames, times, thetas, thetas, tsr.WHOLE, R)
        assert np.array_equal(got["on"], ref["on"]) and np.array_equal(got["off"], ref["off"])


def test_generic_division_and_wave_sum_inputs():
    """One pixel's per-frame count on the alternating clip is beyond QMAX of its state type (5 810 436 > 1e6 at 2^-20 in float32
    state, 1 487 471 616 > 1e9 at 2^-28 in float64 state) and fits an int; the 8 x 8 sensor passes 2^32 ON events at 24 frames
    (4 462 414 848 ON, 4 090 546 944 OFF) while a pixel's own total is 69 725 232."""
    for name, qmax in (("f32", 1e6), ("f64", 1e9)):
        R, theta, model = tsr.GENERIC[name]
        frames, times = tsr.alternating_clip(37, 33, 3)
        on, off = tsr.column_model(frames, times, theta, theta, ((16, 16), (9, 9)), R)
        print(name, on, off)
        assert qmax < on < 2 ** 31 and qmax < off < 2 ** 31
        assert (model["cutoff_hz"] > 0) == (R == np.float64)
        if R == np.float64:
            assert tsr.clamp_eps(frames * 0, times, model["cutoff_hz"]).min() > 2.0
    n, (on, off), one = tsr.wave_sum_frames()
    print(n, on, off, one)
    assert n <= 40 and max(on, off) > 2 ** 32 and one < 2 ** 32
    assert (on % 2 ** 32, off % 2 ** 32) != (on, off)  # a 32-bit wave sum gives another number


def test_levels_clip_holds_every_grey_level_and_starts_late():
    frames, times = tsr.levels_clip()
    late, early = tsr.levels_clip(), tsr.levels_clip(0.0)
    assert times[0] > 0 and early[1][0] == 0 and np.array_equal(late[0], early[0])
    assert np.allclose(np.diff(late[1]), np.diff(early[1]), rtol=0, atol=1e-15)
    d = np.diff(times)
    assert d.min() >= 0.0004 and d.max() <= 0.006 and len(set(np.round(d, 9))) == len(d)
    for f in frames:
        assert len(np.unique(f)) == 256
    steps = {(int(a), int(b)) for k in range(len(frames) - 1) for a, b in zip(frames[k].ravel()[:8], frames[k + 1].ravel()[:8])}
    assert {(0, 20), (20, 21), (21, 255), (255, 21), (21, 20), (20, 0), (0, 255), (255, 20), (0, 21), (255, 0)} <= steps
    # frame 0's eps is neither 0 nor clamped on some pixels (cutoff 100 Hz): (1 - eps) L + eps L is a rounded expression
    e0 = tsr.clamp_eps(frames, times)[0]
    assert ((e0 > 0) & (e0 < 1)).sum() > 100
    # the start time is visible in the counts: a sweep that took frame 1's interval from t[0] would give the other reference
    for name in ("defaults", "cutoff_f64"):
        a, b = tsr.levels_reference(name), tsr.levels_reference(name, 0.0)
        print(name, (a["on"] - b["on"]).tolist(), (a["off"] - b["off"]).tolist())
        assert not (np.array_equal(a["on"], b["on"]) and np.array_equal(a["off"], b["off"]))
        assert np.all(a["on"] > 0) and np.all(a["off"] > 0) and not a["rule_on"].any()


def test_clamp_clip_has_eps_on_both_sides_of_one_in_every_frame():
    frames, times = tsr.clamp_clip()
    eps = tsr.clamp_eps(frames, times)
    print([(int((e > 1).sum()), int((e < 1).sum())) for e in eps])
    for e in eps[1:]:
        assert (e > 1).sum() >= 100 and (e < 1).sum() >= 100
    for leak in (True, False):
        ref = tsr.clamp_reference(leak)
        assert np.all(ref["on"] > 0) and np.all(ref["off"] > 0)
    assert not np.array_equal(tsr.clamp_reference(True)["on"], tsr.clamp_reference(False)["on"])


def test_threshold_clamp_case_clamps_a_share_of_the_pixels():
    pos, neg = tsr.thres_clamp_fraction()
    print(pos, neg)  # 0.344, 0.399
    assert 0.1 <= pos <= 0.9 and 0.1 <= neg <= 0.9
    ref = tsr.thres_clamp_reference()
    assert np.all(ref["on"] > 0) and np.all(ref["off"] > 0) and not ref["rule_on"].any()
    assert tsr.THRES_CLAMP["model"]["refractory_period_s"] == 0


def test_lone_pixel_outside_the_roi_switches_the_rule_on():
    (x0, x1), (y0, y1) = tsr.ROI
    x, y = tsr.LONE_PIXEL
    assert not (x0 <= x <= x1 and y0 <= y <= y1)
    with_lone, without = tsr.lone_pixel_clip(True)[0], tsr.lone_pixel_clip(False)[0]
    assert (with_lone != without).any(axis=0).sum() == 1 and (with_lone != without)[:, y, x].any()
    ref, plain = tsr.lone_pixel_reference(True), tsr.lone_pixel_reference(False)
    print(ref["rule_on"].tolist(), ref["max_m"].tolist(), plain["max_m"].tolist())
    assert ref["rule_on"].tolist() == [True, True] + [False] * 9
    # refr_on_n = 3 (REFRACTORY_S, 1 ms frames): without the lone pixel no pixel of the sensor, inside the ROI or not, gets there
    assert not plain["rule_on"].any() and plain["max_m"].max() < 3 and ref["max_m"][:2].min() >= 3
    assert ref["max_m_roi"].max() < 3 and ref["max_m"].max() <= 32
    assert ref["on"][:5].min() > 0
