"""CPU-only: the host side of VideoToEvents(auto_upsample=True) -- the per-batch factor rule from the squared-speed bits the
device reduces, the ragged frame times, and the new entry points of the C ABI."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("v2e_slomo_max_speed2_seg", "v2e_slomo_prep_tab", "v2e_slomo_fuse_tab", "v2e_f32_to_u8_trunc_tab")


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def test_factor_is_the_ceil_of_the_float32_sqrt():
    from v2e_amd.pipeline import auto_upsampling_factor
    assert auto_upsampling_factor(_bits(16.0), None) == 4
    assert auto_upsampling_factor(_bits(16.5), None) == 5
    assert auto_upsampling_factor(_bits(144.0), None) == 12
    # the float32 just above 25: its float32 sqrt rounds to 5.0 (the reference takes torch.sqrt in float32), a float64 sqrt does not
    v = np.nextafter(np.float32(25.0), np.float32(30.0))
    assert int(np.ceil(np.sqrt(np.float64(v)))) == 6 and float(np.sqrt(v)) == 5.0
    assert auto_upsampling_factor(_bits(v), None) == 5


def test_factor_floors_at_the_minimum_and_at_two():
    from v2e_amd.pipeline import auto_upsampling_factor
    assert auto_upsampling_factor(0, None) == 2            # no motion at all
    assert auto_upsampling_factor(_bits(0.25), None) == 2  # speed 0.5 -> 1 -> 2
    assert auto_upsampling_factor(_bits(0.25), 3) == 3
    assert auto_upsampling_factor(_bits(49.0), 3) == 7     # the minimum does not cap
    assert auto_upsampling_factor(_bits(4.0), 1) == 2
    assert auto_upsampling_factor(_bits(4.0), None) == 2


def test_nan_flow_raises():
    from v2e_amd.pipeline import auto_upsampling_factor
    with pytest.raises(ValueError):
        auto_upsampling_factor(0xFFFFFFFF, 3)
    with pytest.raises(ValueError):
        auto_upsampling_factor(-1, None)  # the same bits read back as a signed int32


def _reference_times(n_src, factors, bs, dt):
    """slomo.py:388-400 (interframeTimes per batch, concatenated) and v2e.py:786-797 (stretched to the processed duration)."""
    npairs = n_src - 1
    interpTimes, inputFrameCounter = None, 0
    for bi, b0 in enumerate(range(0, npairs, bs)):
        num_batch_frames = min(bs, npairs - b0)
        upsampling_factor = factors[bi]
        numOutputFramesThisBatch = upsampling_factor * num_batch_frames
        interframeTime = 1 / upsampling_factor
        interframeTimes = inputFrameCounter + np.array(range(numOutputFramesThisBatch)) * interframeTime
        interframeTimes = interframeTimes.squeeze()
        interpTimes = interframeTimes if interpTimes is None else np.concatenate((interpTimes, interframeTimes))
        inputFrameCounter += num_batch_frames
    srcVideoRealProcessedDuration = npairs * dt
    f = srcVideoRealProcessedDuration / (np.max(interpTimes) - np.min(interpTimes))
    return interpTimes, f * interpTimes


@pytest.mark.parametrize("n_src,bs,factors", [(8, 3, [2, 5, 3]), (23, 8, [7, 4, 12]), (12, 4, [3, 3, 9]), (3, 8, [6])])
def test_ragged_frame_times_follow_slomo_and_v2e(n_src, bs, factors):
    from v2e_amd.pipeline import interp_frame_times, interp_times
    dt = 1 / 30.0
    raw, t = _reference_times(n_src, factors, bs, dt)
    got_raw = interp_times(n_src, None, bs, factors)
    got = interp_frame_times(n_src, None, dt, bs, factors=factors)
    assert got_raw.shape == raw.shape and np.array_equal(got_raw, raw)
    assert got.shape == t.shape and np.array_equal(got, t)


def _times_before_auto_upsample(n_src, U, src_frame_interval_s, batch_size=None):
    """interp_frame_times as it was before the per-batch factors (fixed U)."""
    npairs = n_src - 1
    bs = npairs if not batch_size else int(batch_size)
    parts = []
    for b0 in range(0, npairs, bs):
        nb = min(bs, npairs - b0)
        parts.append(b0 + np.array(range(U * nb)) * (1 / U))
    interp = np.concatenate(parts)
    duration = npairs * float(src_frame_interval_s)
    f = duration / (np.max(interp) - np.min(interp))
    return f * interp


@pytest.mark.parametrize("n_src,U,bs", [(11, 10, 8), (150, 3, 8), (7, 7, None), (40, 6, 5)])
def test_equal_factors_give_the_fixed_u_times_bit_for_bit(n_src, U, bs):
    from v2e_amd.pipeline import interp_frame_times
    dt = 1 / 25.0
    old = _times_before_auto_upsample(n_src, U, dt, bs)
    nb = len(range(0, n_src - 1, bs or (n_src - 1)))
    assert np.array_equal(interp_frame_times(n_src, U, dt, bs), old)
    assert np.array_equal(interp_frame_times(n_src, None, dt, bs, factors=[U] * nb), old)
    with pytest.raises(ValueError):
        interp_frame_times(n_src, None, dt, bs, factors=[U] * (nb + 1))


def test_new_entry_points_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "v2e_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(v2e_[a-z0-9_]+)\s*\(", src))
    from v2e_amd import _capi
    lib = _capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _capi.SIGNATURES
        assert hasattr(lib, name)


def test_sample_table_is_v2e_frame_order():
    """Batches U_b = 2, 5, 3 of 3, 3 and 2 pairs: sample s of the chunk is frame s, frame = batch offset + U_b * pair + k
    (slomo.py:441), with the time row of (k + 0.5) / U_b."""
    from v2e_amd.pipeline import auto_sample_table
    ts, tab, cuts = auto_sample_table([2, 5, 3], 8, 3)
    assert cuts == [0, 6, 21, 27] and len(tab) == 27
    assert [f for _, _, f in tab] == list(range(27))
    off, expect = 0, []
    for j, (u, nb) in enumerate(zip([2, 5, 3], [3, 3, 2])):
        for b in range(nb):
            for k in range(u):
                expect.append((3 * j + b, off + u * b + k, (k + 0.5) / u))
        off += u * nb
    assert [(p, f, ts[r]) for p, r, f in tab] == expect
    with pytest.raises(ValueError):
        auto_sample_table([2, 5], 8, 3)


def test_group_and_chunk_pairs_are_refused_with_auto_upsample():
    """The sharded paths derive every rank's frame count from (pairs, world size): not so with per-batch factors."""
    from v2e_amd.pipeline import VideoToEvents
    pipe = VideoToEvents(None, None, None, batch_size=2, auto_upsample=True)
    frames = np.zeros((5, 40, 70), dtype=np.uint8)
    with pytest.raises(NotImplementedError):
        pipe.run(frames, 1 / 30, group=object())
    with pytest.raises(NotImplementedError):
        pipe.run(frames, 1 / 30, chunk_pairs=4)
    with pytest.raises(NotImplementedError):
        pipe.upsample_sharded(frames, group=object())
