"""The streamed ThresholdSweep without a GPU: the continuation check of `add_run`, the new C entry's declaration and binding, and
-- with the oracle alone -- that the clips tests/test_sweep_stream_gpu.py cuts at a chunk boundary switch the refractory rule on
where those cuts assume."""
import os
import re

import numpy as np
import pytest

import threshold_sweep_ref as tsr
from v2e_amd.sweep import SweepResult, ThresholdSweep, check_continuation


# ------------------------------------------------------------------------------------------------ the continuation check
def test_first_chunk_begins_the_clip():
    assert check_continuation(0, None, [0.0, 1e-3]) == 0
    assert check_continuation(0, None, [0.5], frame0=0) == 0
    with pytest.raises(ValueError, match="a gap"):
        check_continuation(0, None, [0.0, 1e-3], frame0=3)


def test_later_chunks_continue_where_the_last_one_ended():
    assert check_continuation(7, 6e-3, [7e-3, 8e-3]) == 7
    assert check_continuation(7, 6e-3, [7e-3], frame0=7) == 7
    with pytest.raises(ValueError, match="a gap"):
        check_continuation(7, 6e-3, [7e-3, 8e-3], frame0=8)
    with pytest.raises(ValueError, match="an overlap"):
        check_continuation(7, 6e-3, [7e-3, 8e-3], frame0=6)
    with pytest.raises(ValueError, match="an overlap"):
        check_continuation(7, 6e-3, [7e-3, 8e-3], frame0=0)


@pytest.mark.parametrize("t", [[6e-3, 7e-3], [5e-3, 7e-3]], ids=["equal", "earlier"])
def test_a_chunk_must_begin_after_the_last_frame_swept(t):
    with pytest.raises(ValueError, match="not after the last frame"):
        check_continuation(7, 6e-3, t)


@pytest.mark.parametrize("t", [[], [1e-3, 1e-3], [2e-3, 1e-3], [1e-3, float("nan")], [float("inf")], [-1e-3, 0.0]],
                         ids=["empty", "equal", "decreasing", "nan", "inf", "negative"])
def test_times_inside_a_chunk(t):
    with pytest.raises(ValueError):
        check_continuation(0, None, t)


def test_add_run_checks_before_it_touches_the_device():
    """The checks of add_run come before anything needs a GPU: a host tensor, and a chunk that does not continue."""
    import torch
    sw = ThresholdSweep(4, 5, [0.2, 0.3])
    assert sw.frames_seen == 0 and sw.host_syncs == 0
    with pytest.raises(ValueError, match="add_run: frames are on the host"):
        sw.add_run(torch.zeros((2, 4, 5), dtype=torch.uint8), [0.0, 1e-3])
    with pytest.raises(ValueError, match="add_run: frames must be a device tensor"):
        sw.add_run(np.zeros((2, 4, 5), np.uint8), [0.0, 1e-3])
    res = sw.result()  # nothing swept: zeros, and no read-back to count
    assert isinstance(res, SweepResult) and res.on.tolist() == [0, 0] and res.off.tolist() == [0, 0]
    assert res.rule_on.tolist() == [False, False] and res.rule_on_from.tolist() == [-1, -1] and sw.host_syncs == 0
    sw.reset()
    assert sw.frames_seen == 0


def test_run_results_carry_rule_on_from():
    res = SweepResult(np.array([1, 2]), np.array([3, 4]), np.array([False, True]))
    assert res.rule_on_from.tolist() == [-1, 0] and res.rule_on_from.dtype == np.int64


# --------------------------------------------------------------------------------------------------------- the C entry
def test_chunk_entry_is_declared_and_bound():
    from v2e_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "v2e_amd.h")).read()
    for name in ("v2e_thres_sweep_chunk", "v2e_thres_sweep_chunk_info"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, src)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(_capi.SIGNATURES[name][1]) == n_args, (name, n_args)
    # the entries the one-shot sweep had keep their declarations
    assert re.search(r"\bint v2e_thres_sweep\(const void \*frames, int frame_dtype, int F, int H, int W, const double \*t_frames, "
                     r"const v2e_sweep_params \*p,", src)
    assert "int v2e_thres_sweep_info(int f64_state, int scalar_thres, int cols_per_thread, int *cols_out, int *vgprs, " \
           "int *workgroups_per_cu);" in src


# ------------------------------------------------------------------------------ the cuts cut where the GPU tests claim
def test_lone_pixel_switches_the_rule_on_in_its_frame_and_not_before():
    """tests/test_sweep_stream_gpu.py puts LONE_FRAME first in, last in and inside a chunk.  That is a boundary case only if the
    rule first comes on in that very frame -- in some columns, so that the others stay with the kernel."""
    ref = tsr.lone_pixel_reference(True)
    assert ref["rule_on"].any() and not ref["rule_on"].all()
    frames, times = tsr.lone_pixel_clip(True)
    model, _ = tsr.CONFIGS["refractory"]
    before = tsr.oracle_sweep(frames[:tsr.LONE_FRAME], times[:tsr.LONE_FRAME], tsr.THRESHOLDS, tsr.THRESHOLDS, tsr.ROI, **model)
    upto = tsr.oracle_sweep(frames[:tsr.LONE_FRAME + 1], times[:tsr.LONE_FRAME + 1], tsr.THRESHOLDS, tsr.THRESHOLDS, tsr.ROI, **model)
    assert not before["rule_on"].any()
    assert np.array_equal(upto["rule_on"], ref["rule_on"])
    assert not tsr.lone_pixel_reference(False)["rule_on"].any()
    # the cuts of the GPU test: LONE_FRAME first in, last in, inside a chunk
    for cut, where in (((5, 7), "first"), ((6, 6), "last"), ((3, 4, 5), "inside")):
        assert sum(cut) == len(frames)
        starts = np.concatenate(([0], np.cumsum(cut)))
        c = int(np.searchsorted(starts, tsr.LONE_FRAME, side="right")) - 1
        lo, hi = starts[c], starts[c + 1] - 1
        assert {"first": tsr.LONE_FRAME == lo and hi > lo, "last": tsr.LONE_FRAME == hi and lo < hi,
                "inside": lo < tsr.LONE_FRAME < hi}[where], (cut, where)


def test_the_clip_cuts_cover_odd_and_even_starts_and_one_frame_chunks():
    frames, _ = tsr.clip()
    cuts = [(40,), (1, 39), (7, 8, 25), (13, 1, 1, 25), (1,) * 40]
    starts = set()
    for cut in cuts:
        assert sum(cut) == len(frames)
        starts.update(int(s) for s in np.cumsum(cut)[:-1])
    assert any(s % 2 for s in starts) and any(s % 2 == 0 for s in starts) and 1 in starts
    assert cuts[1][0] == 1 and 1 in cuts[3][1:-1]
    # in the refractory configuration the rule comes on in the first chunk of some cuts and in a later chunk of others
    ref = tsr.reference("refractory")
    assert ref["rule_on"].any() and not ref["rule_on"].all()
    first_on = min(n for n in (7, 13, 15, 40) if tsr.prefix_reference("refractory", n)["rule_on"].any())
    print("the rule is first on within the first %d frames" % first_on)
