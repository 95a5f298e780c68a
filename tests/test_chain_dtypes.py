"""What keeps tests/test_chain_dtypes_gpu.py from going blind, checked with the oracle alone (no GPU): the clips of
tests/chain_dtypes.py hold the values they promise, make events, stay below max_iters, and the frames built for frame_body's
reciprocal floor division really put the estimate one off, in both directions, and the remainder on zero."""
from fractions import Fraction

import numpy as np
import pytest

import chain_dtypes as cd

H, W = 33, 37


def test_all_on_is_the_record_tests_parameter_set():
    import test_record8_gpu
    assert cd.ALL_ON == test_record8_gpu.ALL_ON


def _fixup_stats(orc, kw, frames, times, seed):
    """Per built frame, from the oracle's planes around it: (pixels, hit: off by one or remainder 0, estimate too small, too large,
    remainder 0, remainder 0 under an estimate that is too small: r0 == bt in the kernel), and the pos / neg event pixels."""
    rows = []

    def watch(k, before, ora):
        am, th, pos = cd.frame_quotients(before, ora.lp_log_frame, ora.pos_thres_arr, ora.neg_thres_arr, np.float32)
        fires = am >= th
        off = cd.estimate_off_by_one(am, th, np.float32)
        zero = cd.remainder_zero(am, th, np.float32)
        # the predicate's floor is the oracle's count (c10::div_floor_floating on the same operands)
        cnt = np.where(pos, ora.last["pos_cnt"], ora.last["neg_cnt"])
        assert np.array_equal(cd.estimate(am, th, np.float32) - off, cnt)
        rows.append(dict(n=am.size, hit=int(((off != 0) | zero).sum()), small=int((off == -1).sum()), large=int((off == 1).sum()),
                         zero=int(zero.sum()), zero_small=int((zero & (off == -1)).sum()), on=int((fires & pos).sum()),
                         off=int((fires & ~pos).sum())))

    out = cd.oracle_run(orc, kw, frames, times, seed=seed, watch=watch)
    assert out["state"] == np.float32 and out["events"].shape[0] > 0 and out["max_count"] < cd.MAX_ITERS
    return rows


def test_reciprocal_of_the_default_scalar_thresholds_never_underestimates():
    """Thresholds 0.2 / 0.15 in float32 state: the estimate floor(fl(am * fl(1 / theta))) is never BELOW the true floor, so the
    `r0 >= bt` arm of frame_body's fix-up cannot be reached with them.  Proof: fl(1 / theta) >= 1 / theta for both (checked in
    rationals), so am * fl(1 / theta) >= am / theta >= n, and rounding to nearest is monotone: fl(.) >= n.  Checked by brute force
    too, and the counts are asserted: of all 2^23 float32 values of am in [1, 2), 0 estimates are too small and 3 (theta 0.2) and
    4 (0.15) too large -- the few values just below a multiple of theta; of every 7th value in [2, 4) (1 198 373 values), 0 too
    small, 3 and 2 too large.  FIXUP_KW_DOWN's thresholds round the other way: in [1, 2), 1 (55 / 256) and 2 (355 / 2048)
    estimates too small, 0 too large.  So random inputs all but never reach either arm: fixup_frames has to aim."""
    def count(t, am):
        d = cd.estimate_off_by_one(am, np.full(am.shape, t), np.float32)
        return int((d == -1).sum()), int((d == 1).sum()), d.size

    binade = np.arange(0x3F800000, 0x40000000, dtype=np.int32).view(np.float32)  # [1, 2)
    sparse = np.arange(0x40000000, 0x40800000, 7, dtype=np.int32).view(np.float32)  # [2, 4)
    for th, large, large_sparse in ((0.2, 3, 3), (0.15, 4, 2)):
        t = np.float32(th)
        rbt = np.float32(1) / t
        assert Fraction(float(rbt)) >= 1 / Fraction(float(t))
        print("theta", th, "(too small, too large, of) in [1, 2):", count(t, binade), "every 7th of [2, 4):", count(t, sparse))
        assert count(t, binade) == (0, large, 1 << 23)
        assert count(t, sparse) == (0, large_sparse, 1198373)
    for th, small in ((cd.FIXUP_KW_DOWN["pos_thres"], 1), (cd.FIXUP_KW_DOWN["neg_thres"], 2)):
        t = np.float32(th)
        assert float(t) == th, "a float32 value"
        rbt = np.float32(1) / t
        assert Fraction(float(rbt)) < 1 / Fraction(float(t)) and np.float32(t * rbt) < 1  # am = theta: q0 = 0, r0 == theta
        print("theta", th, "(too small, too large, of) in [1, 2):", count(t, binade))
        assert count(t, binade) == (small, 0, 1 << 23)


def test_fixup_frames_reach_both_arms_of_the_fixup(oracle_lib):
    """fixup_frames at 33x37 (1 221 pixels per frame), seed 3, measured here (hit = estimate off by one or remainder 0):
      FIXUP_KW (0.2 / 0.15)       frame 1: 720 hits (59 %), 572 too large, 148 remainder 0;  frame 2: 1 221 (100 %), 671, 550;
                                  frame 3: 898 (74 %), 444, 454;  never too small (see the test above)
      FIXUP_KW_DOWN (55/256, 355/2048)  frame 1: 1 095 hits (90 %), 1 000 too small;  frame 2: 1 221 (100 %), 1 215;
                                  frame 3: 1 183 (97 %), 1 172;  every one of the too-small estimates on an exact multiple (r0 == bt)
    Asked: at least 25 % of the pixels of every built frame hit; at least 20 pixels too small and 20 too large over the built
    frames of the two parameter sets together (float32 state reaches each direction with ONE threshold value only on one side);
    ON and OFF quotients both occur."""
    small = large = zero_small = 0
    for name, kw in (("up", cd.FIXUP_KW), ("down", cd.FIXUP_KW_DOWN)):
        frames, times, hits = cd.fixup_frames(oracle_lib, kw, H, W, 3)
        assert frames.dtype == np.float32 and frames.shape == (1 + len(cd.FIXUP_BUILT), H, W)
        assert frames.min() > 0 and frames.max() < 20
        rows = _fixup_stats(oracle_lib, kw, frames, times, 3)
        for k, r in zip(cd.FIXUP_BUILT, rows):
            print(name, "frame", k, r)
            assert 4 * r["hit"] >= r["n"], "frame %d of %s: fewer than 25 %% of the pixels hit" % (k, name)
            # what the builder meant to hit is what the oracle's planes show
            assert r["hit"] >= int((hits[k - 1] != 0).sum())
        assert sum(r["on"] for r in rows) >= 20 and sum(r["off"] for r in rows) >= 20
        small += sum(r["small"] for r in rows)
        large += sum(r["large"] for r in rows)
        zero_small += sum(r["zero_small"] for r in rows)
        if name == "up":
            assert sum(r["zero"] for r in rows) >= 20  # remainder 0 under a right estimate: the boundary of `r0 < 0`
    assert small >= 20 and large >= 20
    assert zero_small >= 20  # the equality in `r0 >= bt`


def test_fixup_frames_u8_keep_hits(oracle_lib):
    """uint8 frames with hits (estimate off by one or remainder 0), FIXUP_KW, 33x37, seed 3, counted from the oracle's planes:
      fixup_frames_rounded (the float frames rounded to bytes)   8 of 3 663 pixel-frames keep a hit, by chance (all 8
                                                                 remainders 0); the float frames have 2 839.  Asked: some
      fixup_frames_u8 (a search among the grey levels, 6 frames) 131 of 7 326 (88 too large, 43 remainders 0).  Asked: at least 20
    None too small in either: thresholds 0.2 / 0.15 cannot."""
    frames, times = cd.fixup_frames_rounded(oracle_lib, cd.FIXUP_KW, H, W, 3)
    assert frames.dtype == np.uint8
    rows = _fixup_stats(oracle_lib, cd.FIXUP_KW, frames, times, 3)
    print("rounded:", rows)
    assert sum(r["hit"] for r in rows) >= 1
    frames, times, hits = cd.fixup_frames_u8(oracle_lib, cd.FIXUP_KW, H, W, 3)
    assert frames.dtype == np.uint8
    rows = _fixup_stats(oracle_lib, cd.FIXUP_KW, frames, times, 3)
    print("searched:", rows)
    assert sum(r["hit"] for r in rows) >= 20 and sum(r["large"] for r in rows) >= 1
    assert sum(r["hit"] for r in rows) >= int((hits != 0).sum())


def test_exact_multiple_clip_has_zero_remainders(oracle_lib):
    """exact_multiple_clip at 33x37, 40 frames, leak and shot noise off in frames 1-19 and on from frame 20 (as the device test
    feeds it): measured here 15 699 pixel-frames with an event whose quotient is an exact integer (r0 == 0) in float64 state, of
    the 19 944 with an event in frames 1-19; no estimate off by one.  Asked: at least 10 000."""
    frames, times = cd.exact_multiple_clip(40, H, W, 5)
    assert frames.dtype == np.float32 and np.array_equal(frames * 8, np.rint(frames * 8)) and frames.max() <= 5.5
    tot = dict(zero=0, ev=0, off=0)

    def watch(k, before, ora):
        if ora.leak_rate_hz > 0:
            return  # (the leak moves the base before the division: the ordinary quotients)
        am, th, pos = cd.frame_quotients(before, ora.lp_log_frame, cd.EXACT_KW["pos_thres"], cd.EXACT_KW["neg_thres"], np.float64)
        fires = am >= th
        assert np.array_equal(np.where(pos, ora.last["pos_cnt"], ora.last["neg_cnt"]), cd.estimate(am, th, np.float64))
        tot["ev"] += int(fires.sum())
        tot["zero"] += int((fires & cd.remainder_zero(am, th, np.float64)).sum())
        tot["off"] += int((cd.estimate_off_by_one(am, th, np.float64) != 0).sum())

    noisy = {k: cd.EXACT_KW_NOISY[k] for k in ("leak_rate_hz", "shot_noise_rate_hz")}
    out = cd.oracle_run(oracle_lib, cd.EXACT_KW_NOISY, frames, times, phases=[(1, {k: 0.0 for k in noisy}), (20, noisy)], watch=watch)
    print(tot, out["counters"], out["max_count"])
    assert out["state"] == np.float64
    assert tot["zero"] >= 10000
    assert out["events"].shape[0] > 0 and out["max_count"] < cd.MAX_ITERS


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_float_clips_hold_every_edge_value_in_every_frame(dtype, oracle_lib):
    """Every column value of EDGE_VALUES in every frame, the alternating column, fractional (float64: not float32) values elsewhere;
    and with cutoff_hz = 300 the oracle's eps = min((x + 20) / 275 * dt_over_tau, 1) is at the clamp on some pixel-frames
    and below it on others.  The oracle's own eps is observed through its lp_log_frame: at the clamp it IS the frame's lin-log value
    L, below it it equals (1 - eps) lp + eps L bit for bit and differs from L wherever the pixel moved.  Measured here at 33x37,
    20 frames, all pixel-frames: 19 435 at the clamp, 3 764 below it, 2 387 of those moved (float32 frames; float64 frames 19 284,
    3 915 and 2 231)."""
    frames, times = cd.clip(dtype, 20, H, W, 21)
    edges = cd.edge_values(dtype, False)
    assert frames.dtype == dtype and frames.shape == (20, H, W)
    assert set(cd.EDGE_VALUES) <= set(edges) and {0.0, 20.0, 255.0, 300.0, 1000.0} <= set(edges)
    assert float(np.float32(edges[2])) == edges[2] < 20.0 < edges[3] == float(np.float32(edges[3]))
    for f in frames:
        for c, v in enumerate(edges):
            assert np.all(f[:, c] == v)
    alt = frames[:, :, len(edges)]
    assert np.all(alt[0::2] == 0.0) and np.all(alt[1::2] == 255.0)
    body = frames[:, :, len(edges) + 1:]
    assert body.min() >= 0 and body.max() <= 255 and np.mean(body != np.rint(body)) > 0.95
    if dtype == np.float64:
        assert np.mean(body != body.astype(np.float32)) > 0.95
        assert np.all(frames[:, :, 7:9] != frames[:, :, 7:9].astype(np.float32))  # the float64 neighbours of 20.0
    dts = np.diff(times)
    assert dts.min() >= 0.0004 and dts.max() <= 0.006 and len(set(np.round(dts, 9))) == len(dts)
    # eps at and below its clamp: the oracle's lp_log_frame is (1 - eps) lp + eps L with this eps, bit for bit, on every pixel
    kw = cd.case_kw("f64state_f32frames", "scalar_thres", leak_rate_hz=0.0, shot_noise_rate_hz=0.0)
    n = dict(at=0, below=0, below_moved=0)
    prev = {}

    def watch(k, before, ora):
        x = frames[k].astype(np.float64)
        tau = 1.0 / (np.pi * 2 * kw["cutoff_hz"])
        eps = (x + 20.0) / 275.0 * ((times[k] - times[k - 1]) / tau)
        at = eps >= 1.0
        L = cd._oracle_lin_log(oracle_lib, frames[k]).astype(np.float64)
        lp = ora.lp_log_frame
        assert np.array_equal(lp[at], L[at])
        if "lp" in prev:
            want = (1.0 - eps) * prev["lp"] + eps * L
            assert np.array_equal(lp[~at], want[~at])
            moved = ~at & (prev["lp"] != L)
            assert np.all(lp[moved] != L[moved])  # below the clamp the low-pass lags behind
            n["below_moved"] += int(moved.sum())
        prev["lp"] = lp.copy()
        n["at"] += int(at.sum())
        n["below"] += int((~at).sum())

    out = cd.oracle_run(oracle_lib, kw, frames, times, watch=watch)
    print(n)
    assert n["at"] > 1000 and n["below"] > 1000 and n["below_moved"] > 1000 and out["events"].shape[0] > 0


def test_hdr_clip_is_log_valued():
    frames, times = cd.clip(np.float32, 20, H, W, 22, hdr=True)
    assert frames.dtype == np.float32 and frames.min() == 0.0 and frames.max() == np.float32(cd.HDR_MAX)
    assert np.all(frames[:, :, 0] == 0) and np.all(frames[:, :, 1] == np.float32(cd.HDR_MAX))
    assert np.all(frames[0::2, :, 2] == 0) and np.all(frames[1::2, :, 2] == np.float32(cd.HDR_MAX))


CLIPS = [(row, shape, variant) for row in cd.ROWS for shape in cd.SHAPES for variant in cd.VARIANTS]


@pytest.mark.parametrize("row,shape,variant", CLIPS, ids=["-".join(c) for c in CLIPS])
def test_every_clip_makes_events_below_max_iters(row, shape, variant, oracle_lib):
    """Every (row, shape, variant) the device tests run: more than zero events through the oracle, ON and OFF, the largest
    per-pixel count below max_iters, and the state type the row names.  The alternating column fires some 30 events per pixel on
    every frame, so with the refractory periods of ALL_ON and `refractory_heavy` the rule (refractory_period_s > dt / M) is on in
    every frame: every launch of the chain is redone.  `refractory_mixed` has it on in some frames and off in others."""
    kw = cd.case_kw(row, variant)
    frames, times = cd.case_clip(row, shape)
    assert frames.dtype == cd.ROWS[row]["frames"]
    rule = []
    out = cd.oracle_run(oracle_lib, kw, frames, times,
                        watch=lambda k, before, ora: rule.append(kw["refractory_period_s"] > (times[k] - times[k - 1]) / max(ora.last_M, 1)))
    assert out["state"] == cd.ROWS[row]["state"]
    assert out["counters"][1] > 0 and out["counters"][2] > 0
    assert 0 < out["max_count"] < cd.MAX_ITERS
    assert any(rule)
    if variant == "refractory_heavy":
        assert np.mean(rule) > 0.5
    if variant == "refractory_mixed":
        print(row, shape, "rule on in %d of %d frames" % (sum(rule), len(rule)))
        assert 0.15 < np.mean(rule) < 0.85


@pytest.mark.parametrize("row", ["f64state_f32frames", "f64state_f64frames"])
def test_ring_wrap_clips_make_events(row, oracle_lib):
    frames, times = cd.case_clip(row, "33x37", n=cd.N_WRAP)
    out = cd.oracle_run(oracle_lib, cd.case_kw(row), frames, times)
    assert out["events"].shape[0] > 0 and out["max_count"] < cd.MAX_ITERS


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32frames", "f64frames"])
@pytest.mark.parametrize("cutoff_hz", [300, 0], ids=["f64state", "f32state"])
def test_multi_clip_clips_make_events_below_max_iters(cutoff_hz, dtype, oracle_lib):
    clips, times, kw = cd.multi_clip_case(dtype, cutoff_hz)
    for c, frames in enumerate(clips):
        assert frames.dtype == dtype
        out = cd.oracle_run(oracle_lib, kw, frames, [0.0] + list(times[1:, c]), seed=cd.MULTI_SEED, clip=c)
        assert out["counters"][1] > 0 and out["counters"][2] > 0 and 0 < out["max_count"] < cd.MAX_ITERS


def test_fallback_clip_makes_events_below_max_iters(oracle_lib):
    frames, times, kw = cd.fallback_case()
    assert frames.dtype == np.float64 and np.mean(frames != frames.astype(np.float32)) > 0.9
    out = cd.oracle_run(oracle_lib, kw, frames, times)
    assert out["state"] == np.float64 and out["counters"][1] > 0 and out["counters"][2] > 0 and 0 < out["max_count"] < cd.MAX_ITERS
