"""CPU-only: the numpy definition of the event tensors against a case worked by hand, the host arithmetic of
v2e_amd.tensors.plan_windows, and EventTensorizer's argument validation (which comes before anything touches a GPU)."""
import math

import numpy as np
import pytest

from event_tensors_ref import Q, event_tensors, uniform_bounds

NINF = -np.inf


def test_definition_against_a_hand_worked_case():
    """6 rows, 2 windows [0,1) and [1,2), 3 voxel bins, a 2x2 sensor.  By hand (tau = 2 * (t - B_k)):
      (0.00, x0, y0, +1)  k0, tau 0.0 -> bin0 += 1
      (0.25, x0, y0, -1)  k0, tau 0.5 -> bin0 -= 1/2, bin1 -= 1/2
      (0.75, x1, y0, +1)  k0, tau 1.5 -> bin1 += 1/2, bin2 += 1/2
      (1.00, x0, y0, +1)  on the bound: k1, tau 0.0 -> bin0 += 1
      (1.50, x1, y1, -1)  k1, tau 1.0 -> bin1 -= 1 (frac 0: nothing for bin2)
      (2.00, x0, y0, +1)  at the last bound: skipped, n_after"""
    rows = np.array([[0.0, 0, 0, 1], [0.25, 0, 0, -1], [0.75, 1, 0, 1], [1.0, 0, 0, 1], [1.5, 1, 1, -1], [2.0, 0, 0, 1]], np.float32)
    r = event_tensors(rows, uniform_bounds(0.0, 1.0, 2), 2, 2, bins=3)
    count = np.zeros((2, 2, 2, 2), np.int32)  # [k, c, y, x]
    count[0, 1, 0, 0] = count[0, 0, 0, 0] = count[0, 1, 0, 1] = 1
    count[1, 1, 0, 0] = count[1, 0, 1, 1] = 1
    assert np.array_equal(r["count"], count)
    voxel = np.zeros((2, 3, 2, 2), np.float32)
    voxel[0, 0, 0, 0], voxel[0, 1, 0, 0] = 0.5, -0.5
    voxel[0, 1, 0, 1], voxel[0, 2, 0, 1] = 0.5, 0.5
    voxel[1, 0, 0, 0], voxel[1, 1, 1, 1] = 1.0, -1.0
    assert np.array_equal(r["voxel"], voxel)
    assert r["voxel_acc"][0, 0, 0, 0] == Q // 2 and r["voxel_acc"][1, 1, 1, 1] == -Q
    surf = np.full((2, 2, 2, 2), NINF, np.float32)
    surf[0, 1, 0, 0], surf[0, 0, 0, 0], surf[0, 1, 0, 1] = 0.0, 0.25, 0.75
    surf[1] = surf[0]
    surf[1, 1, 0, 0], surf[1, 0, 1, 1] = 1.0, 1.5
    assert np.array_equal(r["time_surface"], surf)
    assert (r["n_bad"], r["n_before"], r["n_after"]) == (0, 0, 1)
    # the voxel invariant: the bins of a window and pixel sum to ON - OFF
    assert np.array_equal(r["voxel_acc"].sum(1), Q * (r["count"][:, 1].astype(np.int64) - r["count"][:, 0]))


def test_definition_counts_malformed_and_early_rows():
    rows = np.array([[0.5, 2, 0, 1], [0.5, 0, -1, 1], [0.5, 0, 0, 0], [0.5, 0.5, 0, 1], [np.nan, 0, 0, 1], [-0.5, 0, 0, 1], [0.5, 1, 1, -1]],
                    np.float32)
    r = event_tensors(rows, np.array([0.0, 1.0]), 2, 2, bins=1)
    assert (r["n_bad"], r["n_before"], r["n_after"]) == (5, 1, 0)
    assert r["count"].sum() == 1 and r["count"][0, 0, 1, 1] == 1 and r["voxel"][0, 0, 1, 1] == -1.0


def test_plan_windows_on_bounds_that_are_not_representable():
    """B_k = k * window_s is rarely the real k * window_s: a t_end exactly on B_k completes window k - 1, its float64 neighbour
    below does not -- for every k, whatever the quotient's floor says."""
    from v2e_amd.tensors import plan_windows
    assert 3 * 0.1 > 0.3  # the bound that is not 0.3
    assert plan_windows(0.3, window_s=0.1)[0] == 2
    assert plan_windows(3 * 0.1, window_s=0.1)[0] == 3
    for ws, t0 in ((1 / 300.0, 0.0), (0.1, 0.0), (1e-3, 0.25), (1 / 3.0, -7.0)):
        for k in range(1, 1500):
            bk = t0 + float(k) * ws
            assert plan_windows(bk, window_s=ws, t_start=t0)[0] == k, (ws, t0, k)
            assert plan_windows(math.nextafter(bk, -math.inf), window_s=ws, t_start=t0)[0] == k - 1, (ws, t0, k)
    # windows already handed out are not counted again; a t_end before the open window completes nothing
    assert plan_windows(1.0, k_open=4, window_s=0.1)[:2] == (6, True)
    assert plan_windows(0.2, k_open=4, window_s=0.1)[:2] == (0, True)
    assert plan_windows(-5.0, window_s=0.1, t_start=-1.0)[:2] == (0, True)


def test_plan_windows_explicit_bounds():
    from v2e_amd.tensors import plan_windows
    b = [0.0, 0.1, 0.25, 1.0]
    assert plan_windows(0.25, bounds=b)[:2] == (2, True)   # exactly on a bound: the window before it is complete
    assert plan_windows(math.nextafter(0.25, 0), bounds=b)[:2] == (1, True)
    assert plan_windows(1.0, bounds=b)[:2] == (3, False)   # the table is used up: no open window
    assert plan_windows(7.0, k_open=1, bounds=b)[:2] == (2, False)
    assert plan_windows(7.0, k_open=3, bounds=b) == (0, False, [])
    assert plan_windows(-1.0, bounds=b)[:2] == (0, True)


def test_plan_windows_cuts_voxel_blocks_under_a_scratch_budget():
    from v2e_amd.tensors import plan_windows
    plane = 8 * 5 * 7 * 5
    n, has_open, blocks = plan_windows(1.0, window_s=0.1, voxel_plane_bytes=plane, max_scratch_bytes=3 * plane + 1)
    assert (n, has_open) == (10, True) and blocks == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert plan_windows(1.0, window_s=0.1, voxel_plane_bytes=plane, max_scratch_bytes=1)[2] == [(k, k + 1) for k in range(10)]
    assert plan_windows(1.0, window_s=0.1, voxel_plane_bytes=plane)[2] == [(0, 10)]
    assert plan_windows(1.0, window_s=0.1)[2] == [(0, 10)]          # no voxel grid: one block
    assert plan_windows(0.05, window_s=0.1, voxel_plane_bytes=plane)[2] == []


def test_plan_windows_refuses_a_run_of_too_many_windows():
    from v2e_amd.tensors import MAX_RUN_WINDOWS, plan_windows
    assert MAX_RUN_WINDOWS == 1 << 22
    assert plan_windows(float(MAX_RUN_WINDOWS - 1), window_s=1.0)[0] == MAX_RUN_WINDOWS - 1  # with the open one: exactly the limit
    with pytest.raises(ValueError, match="windows"):
        plan_windows(float(MAX_RUN_WINDOWS), window_s=1.0)
    with pytest.raises(ValueError, match="windows"):
        plan_windows(1e30, window_s=1e-6)
    with pytest.raises(ValueError):
        plan_windows(float(MAX_RUN_WINDOWS + 1), bounds=np.arange(MAX_RUN_WINDOWS + 3.0))
    # ... but not when the windows before were handed out already
    assert plan_windows(float(MAX_RUN_WINDOWS), k_open=MAX_RUN_WINDOWS - 2, window_s=1.0)[0] == 2
    for bad in (dict(), dict(window_s=0.1, bounds=[0, 1]), dict(window_s=0.0), dict(window_s=-1.0), dict(window_s=math.inf)):
        with pytest.raises(ValueError):
            plan_windows(1.0, **bad)
    with pytest.raises(ValueError):
        plan_windows(math.nan, window_s=0.1)
    with pytest.raises(ValueError):
        plan_windows(math.inf, window_s=0.1)


@pytest.mark.parametrize("kw", [
    dict(),                                                  # neither window_s nor bounds
    dict(window_s=0.01, bounds=[0.0, 1.0]),                  # both
    dict(window_s=0.0), dict(window_s=-1.0), dict(window_s=math.nan),
    dict(window_s=1e-30, t_start=1.0),                       # does not advance t_start
    dict(bounds=[0.0]), dict(bounds=[0.0, 2.0, 1.0]), dict(bounds=[0.0, math.inf]),
    dict(window_s=0.01, representations=()), dict(window_s=0.01, representations=("count", "histogram")),
    dict(window_s=0.01, representations=("count", "count")),
    dict(window_s=0.01, representations=("voxel",), voxel_bins=0),
    dict(window_s=0.01, max_scratch_bytes=0),
    dict(window_s=0.01, height=0),
])
def test_tensorizer_refuses_bad_arguments_before_it_needs_a_gpu(kw):
    from v2e_amd import EventTensorizer
    kw = dict(dict(height=4, width=6), **kw)
    with pytest.raises(ValueError):
        EventTensorizer(**kw)


def test_tensorizer_has_no_cpu_fallback():
    import torch
    from v2e_amd import EventTensorizer, V2EAmdError
    if torch.cuda.is_available():
        assert EventTensorizer(4, 6, window_s=0.01).representations == ("count",)
    else:
        with pytest.raises(V2EAmdError):
            EventTensorizer(4, 6, window_s=0.01)
