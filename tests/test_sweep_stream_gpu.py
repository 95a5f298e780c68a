"""v2e_amd.ThresholdSweep fed chunk by chunk (add_run / result / reset) on the MI355X, and the `on_frames` hooks that feed it from
VideoToEvents.run_stream and SyntheticToEvents.run.  The references are those of tests/threshold_sweep_ref.py: one oracle emulator
per column over the whole clip, independent of how the clip is cut.  Every comparison is exact equality of integer arrays.  That
the boundary cases cut where they claim is pinned by tests/test_sweep_stream.py with the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import threshold_sweep_ref as tsr
from v2e_amd import EventEmulator, ThresholdSweep, _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CUTS = [(40,), (1, 39), (7, 8, 25), (13, 1, 1, 25), (1,) * 40]
CUT_IDS = ["40", "1+39", "7+8+25", "13+1+1+25", "40x1"]


def _sweep(name, roi=tsr.ROI, thresholds=tsr.THRESHOLDS, height=37, width=33, **kw):
    model, neg = tsr.CONFIGS[name]
    return ThresholdSweep(height, width, thresholds, neg, roi=roi, seed=tsr.SEED, device=DEV, **model, **kw)


def _dev(frames):
    return torch.from_numpy(np.array(frames)).to(DEV)


def _feed(sw, frames, times, cut, give_frame0=True):
    """The clip through add_run in chunks of the sizes `cut`; returns the frame0 of every chunk."""
    assert sum(cut) == len(times)
    starts, a = [], 0
    for n in cut:
        sw.add_run(frames[a:a + n], times[a:a + n], a if give_frame0 else None)
        starts.append(a)
        a += n
    assert sw.frames_seen == len(times)
    return starts


def _assert_equal(res, ref, what=""):
    assert res.on.dtype == np.int64 and res.off.dtype == np.int64 and res.rule_on.dtype == bool and res.rule_on_from.dtype == np.int64
    print(what, "\non  ", res.on.tolist(), "\nref ", ref["on"].tolist(), "\noff ", res.off.tolist(), "\nref ", ref["off"].tolist(),
          "\nrule_on", res.rule_on.tolist(), "from", res.rule_on_from.tolist())
    assert np.array_equal(res.on, ref["on"]) and np.array_equal(res.off, ref["off"])
    if "rule_on" in ref:
        assert np.array_equal(res.rule_on, ref["rule_on"])
    assert np.array_equal(res.rule_on_from >= 0, res.rule_on)


@pytest.fixture(scope="module")
def clip_dev():
    frames, times = tsr.clip()
    return _dev(frames), times


# 1. chunked equals the oracle, however the clip is cut
@pytest.mark.parametrize("cut", CUTS, ids=CUT_IDS)
@pytest.mark.parametrize("name", list(tsr.CONFIGS))
def test_chunked_sweep_equals_one_oracle_run_per_threshold(clip_dev, name, cut):
    frames, times = clip_dev
    sw = _sweep(name)
    _feed(sw, frames, times, cut, give_frame0=len(cut) != 4)
    refr = tsr.CONFIGS[name][0].get("refractory_period_s", 0.0) > 0
    assert sw.host_syncs == (len(cut) if refr else 0)
    _assert_equal(sw.result(), tsr.reference(name), "%s %r" % (name, cut))


@pytest.mark.parametrize("name", list(tsr.CONFIGS))
def test_result_between_chunks_is_the_prefix(clip_dev, name):
    frames, times = clip_dev
    sw = _sweep(name)
    a = 0
    for n in (7, 8, 25):
        sw.add_run(frames[a:a + n], times[a:a + n], a)
        a += n
        _assert_equal(sw.result(), tsr.prefix_reference(name, a), "%s, first %d frames" % (name, a))


# 2. every instantiation of the kernel through the carry path, on the clip aimed at the floor division's fix-ups
@pytest.mark.parametrize("cut", [(3, 5), (1, 1, 6)], ids=["3+5", "1+1+6"])
@pytest.mark.parametrize("inst", list(tsr.INSTANTIATIONS))
def test_every_instantiation_carries_its_state(inst, cut):
    frames, times, thetas = tsr.aimed_clip(inst)
    sw = ThresholdSweep(37, 33, thetas, roi=tsr.WHOLE, seed=tsr.SEED, device=DEV, refractory_period_s=0.0,
                        **tsr.INSTANTIATIONS[inst]["model"])
    _feed(sw, _dev(frames), times, cut)
    assert sw.host_syncs == 0
    res = sw.result()
    _assert_equal(res, tsr.aimed_reference(inst), "%s %r" % (inst, cut))
    assert not res.rule_on.any()


@pytest.mark.parametrize("cols", [4, 16])
@pytest.mark.parametrize("name", ["defaults", "cutoff_f64"])
def test_other_column_chunk_sizes_carry_too(clip_dev, name, cols):
    frames, times = clip_dev
    sw = _sweep(name, cols_per_thread=cols)
    _feed(sw, frames, times, (7, 8, 25))
    _assert_equal(sw.result(), tsr.reference(name))


# 3. a column leaves the kernel at a chunk boundary
@pytest.mark.parametrize("cut", [(5, 7), (6, 6), (3, 4, 5)], ids=["first_of_chunk", "last_of_chunk", "inside_chunk"])
def test_a_column_leaves_the_kernel_in_the_chunk_that_holds_the_lone_frame(cut):
    frames, times = tsr.lone_pixel_clip(True)
    ref = tsr.lone_pixel_reference(True)
    sw = _sweep("refractory")
    starts = _feed(sw, _dev(frames), times, cut)
    assert sw.host_syncs == len(cut)
    res = sw.result()
    _assert_equal(res, ref, repr(cut))
    chunk0 = max(s for s in starts if s <= tsr.LONE_FRAME)  # (0 for the cut (6, 6): a fresh emulator that goes on into the next chunk)
    assert np.array_equal(res.rule_on_from, np.where(ref["rule_on"], chunk0, -1))


def test_no_column_is_flagged_without_the_lone_pixel():
    frames, times = tsr.lone_pixel_clip(False)
    sw = _sweep("refractory")
    _feed(sw, _dev(frames), times, (5, 7))
    assert sw.host_syncs == 2
    res = sw.result()
    _assert_equal(res, tsr.lone_pixel_reference(False))
    assert not res.rule_on.any() and np.all(res.rule_on_from == -1)


def test_a_flag_in_the_first_chunk_is_a_fresh_emulator(clip_dev):
    frames, times = clip_dev
    sw = _sweep("refractory")
    _feed(sw, frames, times, (40,))
    res = sw.result()
    ref = tsr.reference("refractory")
    _assert_equal(res, ref)
    assert np.array_equal(res.rule_on_from, np.where(ref["rule_on"], 0, -1))


# 4. reset
def test_two_clips_through_one_instance(clip_dev):
    frames, times = clip_dev
    lone_f, lone_t = tsr.lone_pixel_clip(True)
    sw = _sweep("refractory")
    _feed(sw, _dev(lone_f), lone_t, (6, 6))
    _assert_equal(sw.result(), tsr.lone_pixel_reference(True), "lone pixel clip")
    with pytest.raises(ValueError):  # the next clip does not continue this one
        sw.add_run(frames[:7], times[:7], 0)
    sw.reset()
    assert sw.frames_seen == 0 and sw.host_syncs == 0
    _feed(sw, frames, times, (7, 8, 25))
    _assert_equal(sw.result(), tsr.reference("refractory"), "test clip after reset")
    sw.reset()
    _feed(sw, _dev(lone_f), lone_t, (5, 7))
    res = sw.result()
    _assert_equal(res, tsr.lone_pixel_reference(True), "lone pixel clip again")
    assert np.array_equal(res.rule_on_from, np.where(res.rule_on, 5, -1))


# 5. run is what it was
def _recorded_parent_info():
    """{(f64_state, scalar_thres): (vgprs, workgroups_per_cu)} of the default instantiations on the parent commit, as recorded in
    profiles/r18_sweep_stream.txt."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r18_sweep_stream.txt")
    out = {}
    for m in re.finditer(r"^parent commit: k_sweep f64_state=(\d) scalar_thres=(\d) cols_per_thread=8: VGPRs (\d+), workgroups/CU (\d+)$",
                         open(path).read(), re.M):
        out[(int(m.group(1)), int(m.group(2)))] = (int(m.group(3)), int(m.group(4)))
    return out


def test_run_is_unchanged(clip_dev):
    frames, times = clip_dev
    for name in ("defaults", "cutoff_f64", "refractory"):
        sw = _sweep(name)
        _assert_equal(sw.run(frames, times), tsr.reference(name), name)
        assert sw.frames_seen == 0  # run() is no part of a streamed clip
    recorded = _recorded_parent_info()
    assert sorted(recorded) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    lib = _capi.lib()
    for (f64, scalar), want in recorded.items():
        cols, vg, occ = C.c_int(0), C.c_int(0), C.c_int(0)
        _capi.check(lib.v2e_thres_sweep_info(f64, scalar, 0, C.byref(cols), C.byref(vg), C.byref(occ)), "v2e_thres_sweep_info")
        print("k_sweep f64_state=%d scalar_thres=%d cols %d: VGPRs %d, workgroups/CU %d; parent %r" % (f64, scalar, cols.value, vg.value,
                                                                                                     occ.value, want))
        assert cols.value == 8 and (vg.value, occ.value) == want


# 6. small sensors
@pytest.mark.parametrize("one_pixel", [False, True], ids=["whole", "pixel"])
@pytest.mark.parametrize("hw", tsr.SMALL_SENSORS, ids=["%dx%d" % hw for hw in tsr.SMALL_SENSORS])
def test_small_sensors(hw, one_pixel):
    frames, times, roi, ref = tsr.small_sensor_case(hw[0], hw[1], one_pixel)
    sw = ThresholdSweep(hw[0], hw[1], tsr.SMALL_THRESHOLDS, roi=roi, seed=tsr.SEED, device=DEV)
    _feed(sw, _dev(frames), times, (5, 7))
    _assert_equal(sw.result(), ref, "%r %r" % (hw, roi))


# 7. the hooks
HOOK_THRESHOLDS = (0.2, 0.4, 0.8)


class _Hook:
    """on_frames for a sweep: keeps a host copy of what it was given, then hands it on."""

    def __init__(self, sw):
        self.sw, self.frames, self.times, self.frame0 = sw, [], [], []

    def __call__(self, frames, times, frame0):
        assert torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and len(times) == frames.shape[0]
        self.frames.append(frames.cpu().numpy())
        self.times.append(np.asarray(times, np.float64))
        self.frame0.append(int(frame0))
        self.sw.add_run(frames, times, frame0)

    def check(self, n_frames, roi, **model):
        """The callbacks came in order and without gaps, and the sweep equals the oracle on the frames they were given."""
        lens = [len(f) for f in self.frames]
        assert self.frame0 == [int(v) for v in np.concatenate(([0], np.cumsum(lens)[:-1]))] and sum(lens) == n_frames
        frames, times = np.concatenate(self.frames), np.concatenate(self.times)
        ref = tsr.oracle_sweep(frames, times, HOOK_THRESHOLDS, HOOK_THRESHOLDS, roi, seed=tsr.SEED, **model)
        res = self.sw.result()
        _assert_equal(res, ref, "hook, chunks %r" % (lens,))
        assert ref["on"].sum() > 0 and ref["off"].sum() > 0
        return frames, times


def _rows(ev):
    return np.zeros((0, 4), np.float32) if ev is None else (ev.cpu().numpy() if torch.is_tensor(ev) else ev)


def test_synthetic_source_feeds_the_sweep():
    from v2e_amd.synthetic import SyntheticToEvents, moving_dot
    args = ['--t_total', '0.003', '--radius', '20']
    kw = dict(pos_thres=0.2, neg_thres=0.2, seed=tsr.SEED, rng_mode="philox", shot_noise_rate_hz=0.0, device=DEV)
    roi = ((8, 55), (4, 59))
    emu = EventEmulator(**kw)
    sw = ThresholdSweep.from_emulator(emu, HOOK_THRESHOLDS, roi=roi, height=64, width=64)
    hook = _Hook(sw)
    src = moving_dot(64, 64, arg_list=args, device=DEV)
    ev, counts, n = SyntheticToEvents(src, emu, block_frames=8).run(on_frames=hook, return_device=True)
    assert n == 30 and [len(f) for f in hook.frames] == [8, 8, 8, 6] and sw.host_syncs == 0
    frames, times = hook.check(n, roi)
    # the frames the hook was given are the source's own
    own, own_t = moving_dot(64, 64, arg_list=args, device=DEV).frames_block(0, n)
    assert np.array_equal(own.cpu().numpy(), frames) and np.array_equal(np.asarray(own_t, np.float64), times)
    # the run's events are those of a run without the hook
    ev0, counts0, n0 = SyntheticToEvents(moving_dot(64, 64, arg_list=args, device=DEV), EventEmulator(**kw), block_frames=8).run(
        return_device=True)
    assert n0 == n and np.array_equal(counts, counts0) and counts0.sum() > 0
    assert np.array_equal(_rows(ev).view(np.int32), _rows(ev0).view(np.int32))


def test_run_stream_feeds_the_sweep():
    from v2e_amd.pipeline import VideoToEvents
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import int_gradient_frames, portable_unet_state_dict
    H, W, U, BS = 32, 64, 2, 8
    sd_f, sd_i = portable_unet_state_dict(2, 4, 401), portable_unet_state_dict(12, 5, 402)
    eng = SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()}, {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda")
    kw = dict(pos_thres=0.15, neg_thres=0.15, sigma_thres=0.03, cutoff_hz=200.0, leak_rate_hz=0.1, shot_noise_rate_hz=0.0,
              refractory_period_s=0.0, device="cuda", seed=tsr.SEED, rng_mode="philox")
    model = dict(sigma_thres=0.03, cutoff_hz=200.0, leak_rate_hz=0.1)
    src = torch.from_numpy(int_gradient_frames(70, H, W, seed=3, noise=10, as_array=True)).cuda()  # 69 pairs: chunks of 64 and 5
    roi = ((5, 60), (3, 28))
    pipe = VideoToEvents(eng, EventEmulator(**kw), U, batch_size=BS)
    sw = ThresholdSweep.from_emulator(pipe.emu, HOOK_THRESHOLDS, roi=roi, height=H, width=W)
    hook = _Hook(sw)
    ev, counts, n = pipe.run_stream(src, 1 / 30.0, chunk_pairs=64, on_frames=hook, return_device=True)
    assert n == 69 * U and [len(f) for f in hook.frames] == [64 * U, 5 * U] and sw.host_syncs == 0
    hook.check(n, roi, **model)
    pipe0 = VideoToEvents(eng, EventEmulator(**kw), U, batch_size=BS)
    ev0, counts0, n0 = pipe0.run_stream(src, 1 / 30.0, chunk_pairs=64, return_device=True)
    assert n0 == n and np.array_equal(counts, counts0) and counts0.sum() > 0
    assert np.array_equal(_rows(ev).view(np.int32), _rows(ev0).view(np.int32))
