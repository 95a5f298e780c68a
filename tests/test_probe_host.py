"""CPU: the host side of single-pixel probes in device-resident runs -- the C ABI entry and its constants, the pure helper that
appends a run's block to the recorder's series (against a plain per-frame loop written as emulator.py:985-1009 is), and the
validation of probed pixels."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_probe_entry_is_declared_bound_and_exported():
    from v2e_amd import _capi
    src = open(os.path.join(ROOT, "include", "v2e_amd.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define V2E_(PROBE_[A-Z_]+) (\d+)\b", src, flags=re.M)}
    assert consts == {"PROBE_FIELDS": 9, "PROBE_MAX": 64} == {"PROBE_FIELDS": _capi.PROBE_FIELDS, "PROBE_MAX": _capi.PROBE_MAX}
    assert re.search(r"^int v2e_emu_set_probes\(v2e_emu \*h, const int32_t \*pixel_index, int n, double \*out_dev\);", src, flags=re.M)
    res, args = _capi.SIGNATURES["v2e_emu_set_probes"]
    assert len(args) == 4
    assert len(_capi.PROBE_FIELD_NAMES) == _capi.PROBE_FIELDS
    for i, name in enumerate(_capi.PROBE_FIELD_NAMES):  # the header documents the order the binding relies on
        assert re.search(r"^ \*\s+(?:\d [a-z_]+, )?%d %s\b" % (i, name), src, flags=re.M), (i, name)
    if os.path.isfile(_capi.LIB_PATH):
        assert hasattr(_capi.lib(), "v2e_emu_set_probes")
    from v2e_amd.emulator import PIXEL_STATE_SERIES, EventEmulator
    e = EventEmulator(record_single_pixel_states=(1, 2))
    assert tuple(e.single_pixel_states) == PIXEL_STATE_SERIES  # the reference's ten series, in its order
    e.record_single_pixel_states = None


def _per_frame_loop(max_samples, runs, scalar):
    """emulator.py:985-1009 frame after frame: what the series hold after the frames of `runs` [(times, block)], and whether and
    when the recording stopped."""
    from v2e_amd._capi import PROBE_FIELD_NAMES
    st = {k: np.full(max_samples, np.nan) for k in ("time",) + PROBE_FIELD_NAMES}
    count, stopped_in = 0, None
    for r, (times, block) in enumerate(runs):
        for t, row in zip(times, block):
            if stopped_in is not None:
                continue
            if count < max_samples:
                st["time"][count] = t
                for i, name in enumerate(PROBE_FIELD_NAMES):
                    st[name][count] = row[i]
                if scalar is not None:
                    st["pos_thres"][count], st["neg_thres"][count] = scalar
                count += 1
            else:
                stopped_in = r
    return st, count, stopped_in


@pytest.mark.parametrize("scalar", [None, (0.2, 0.25)])
@pytest.mark.parametrize("max_samples,lengths", [(1000, [1, 5, 13]), (19, [1, 5, 13]), (12, [4, 8, 3]), (7, [5, 5, 5]), (6, [9])])
def test_append_pixel_states_equals_the_per_frame_loop(max_samples, lengths, scalar, caplog):
    """Runs of several lengths against a cap that is never reached, reached exactly at the end of the clip, exactly at the end of
    a run, inside a run, and inside the first run: the same series, count and stopping run as the frame-by-frame rule gives; the
    very first frame of the clip is not among a run's frames, so no sample is made for it."""
    import logging
    from v2e_amd._capi import PROBE_FIELD_NAMES, PROBE_FIELDS
    from v2e_amd.emulator import append_pixel_states
    rng = np.random.default_rng(len(lengths) * 100 + max_samples)
    runs, t = [], 0.0
    for n in lengths:
        times = t + 0.001 * (1 + np.arange(n))
        t = times[-1]
        runs.append((times, rng.standard_normal((n, PROBE_FIELDS))))
    ref, ref_count, ref_stop = _per_frame_loop(max_samples, runs, scalar)
    st = {k: np.full(max_samples, np.nan) for k in ("time",) + PROBE_FIELD_NAMES}
    count, stopped_in = 0, None
    with caplog.at_level(logging.INFO, logger="v2e_amd.emulator"):
        for r, (times, block) in enumerate(runs):
            if stopped_in is None:
                count, stop = append_pixel_states(st, count, max_samples, times, block, *(scalar or (None, None)))
                if stop:
                    stopped_in = r
    assert count == ref_count and stopped_in == ref_stop
    for k in ref:
        assert np.array_equal(st[k], ref[k], equal_nan=True), k
    # emulator.py:987-988: a log line at samples 0, 250, 500, ...
    logged = [rec.getMessage() for rec in caplog.records if "single pixel states" in rec.getMessage()]
    assert logged == ["recorded %d single pixel states" % k for k in range(0, count, 250)]


def test_probe_pixel_validation():
    from v2e_amd.emulator import probe_pixel_indices
    H, W = 97, 131
    assert probe_pixel_indices([(0, 0), (H - 1, W - 1), (2, 3), (2, 3), (np.int64(1), np.int32(0))], H, W) == [0, H * W - 1, 2 * W + 3, 2 * W + 3, W]
    assert probe_pixel_indices([], H, W) == []
    assert len(probe_pixel_indices([(0, k % W) for k in range(64)], H, W)) == 64
    with pytest.raises(ValueError, match="at most 64"):
        probe_pixel_indices([(0, k) for k in range(65)], H, W)
    for bad in [(H, 0), (0, W), (-1, 0), (0, -1), (0.0, 1), (1,), (1, 2, 3), "ab", 5]:
        with pytest.raises(ValueError):
            probe_pixel_indices([bad], H, W)


def test_batch_refuses_what_it_cannot_record_before_touching_the_device():
    """show_dvs_model_state still needs the host per frame; record_single_pixel_states no longer raises for being set (without a GPU
    the call gets as far as the engine, which raises V2EAmdError: there is no CPU path)."""
    from v2e_amd import EventEmulator, V2EAmdError
    frames, times = np.zeros((3, 8, 8), np.uint8), [0.0, 0.1, 0.2]
    e = EventEmulator(show_dvs_model_state=["lp_log_frame"], rng_mode="philox")
    with pytest.raises(ValueError, match="show_dvs_model_state / save_dvs_model_state"):
        e.generate_events_batch(frames, times)
    e = EventEmulator(record_single_pixel_states=(9, 1), rng_mode="philox")
    with pytest.raises(ValueError, match="outside the 8 x 8"):
        e.generate_events_batch(frames, times)
    e.record_single_pixel_states = None
    e = EventEmulator(record_single_pixel_states=(1, 1), rng_mode="philox")
    with pytest.raises(ValueError, match="beside record_single_pixel_states"):
        e.generate_events_batch(frames, times, probe_pixels=[(0, 0)] * 64)
    e.record_single_pixel_states = None
    e = EventEmulator(rng_mode="philox")
    with pytest.raises(ValueError, match="at most 64"):
        e.generate_events_batch(frames, times, probe_pixels=[(0, 0)] * 65)
    import torch
    if not torch.cuda.is_available():
        e = EventEmulator(record_single_pixel_states=(1, 1), rng_mode="philox")
        with pytest.raises(V2EAmdError):
            e.generate_events_batch(frames, times)
        e.record_single_pixel_states = None
