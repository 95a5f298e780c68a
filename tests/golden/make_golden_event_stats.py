#!/usr/bin/env python
"""Golden time-bin counts of the reference (v2ecore/v2e_utils.py:384-471, imported from /root/reference): seeded rows at 346 x 260
through select_events_in_roi and histogram_events_in_time_bins for polarity 1 and -1, what ddd_plot_event_counts.py plots.

  event_stats_time_bins.npz   rows float32 [4000,4] (t, x, y, p = +-1), roi_x, roi_y (inclusive pairs), start, stop, time_bin_ms, and
                              ts_on / ts_off: float64 [K,2] of (bin centre, count), the reference's return values

Every t and every tick is a multiple of 2^-10 below 2^13 (31.25 ms bins), so the reference's comparisons of the float32 times with
its float64 ticks are exact whatever the numpy version's promotion rule; the rows start before the first tick and end behind the
last one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

H, W, N = 260, 346, 4000
ROI_X, ROI_Y = (40, 300), (25, 199)
START, STOP, TIME_BIN_MS = 0.25, 3.5, 31.25


def main():
    rh.install_stubs()
    from v2ecore.v2e_utils import histogram_events_in_time_bins, select_events_in_roi
    rng = np.random.RandomState(22)
    t = np.sort(rng.randint(0, 4 * 1024, size=N)) * 2.0 ** -10          # 0 .. 4 s: before the first tick and behind the last
    t[::97] = START + rng.randint(0, 100, size=len(t[::97])) * 0.03125   # some exactly on a tick
    rows = np.stack([t, rng.randint(0, W, size=N), rng.randint(0, H, size=N), rng.choice([-1.0, 1.0], size=N)], axis=1).astype(np.float32)
    ticks = np.arange(START, STOP, TIME_BIN_MS * 0.001)
    assert np.array_equal(ticks * 1024, np.round(ticks * 1024)) and np.array_equal(rows[:, 0].astype(np.float64), t)
    inside = select_events_in_roi(rows, ROI_X, ROI_Y)
    ts_on = histogram_events_in_time_bins(inside, start=START, stop=STOP, time_bin_ms=TIME_BIN_MS, polarity=1)
    ts_off = histogram_events_in_time_bins(inside, start=START, stop=STOP, time_bin_ms=TIME_BIN_MS, polarity=-1)
    print("rows %d, in ROI %d, bins %d, ON %d, OFF %d" % (N, len(inside), len(ts_on), ts_on[:, 1].sum(), ts_off[:, 1].sum()))
    path = os.path.join(HERE, "event_stats_time_bins.npz")
    np.savez_compressed(path, rows=rows, roi_x=np.array(ROI_X), roi_y=np.array(ROI_Y), start=START, stop=STOP, time_bin_ms=TIME_BIN_MS,
                        ts_on=ts_on, ts_off=ts_off)
    print("event_stats_time_bins.npz", os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
