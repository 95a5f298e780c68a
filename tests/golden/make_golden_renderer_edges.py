#!/usr/bin/env python
"""Crafted edge packets through the reference's EventRenderer (v2ecore/renderer.py:161-400, imported from the reference tree
with ref_harness' stubs; numba's @jit is an identity stub, cv2 a stub whose video writer swallows the frames).  Every case is
one renderer fed its packets in order through render_events_to_frames(return_frames=True), with `output_path` and `dvs_vid`
set so that the class works out the time of every frame (taken from the writing frame, as make_golden_render_run.py does).

  renderer_edges.npz   numpy_version    the numpy this was generated with
                       f32_time         1 if np.float32(0) + 0.5 is a float32 there (the frame start time then stays float32)
                       rows             the events of all cases, concatenated ([N,4] float32)
                       frames, cur, ac, start, times
                                        1-D pools of what every case returned and left behind (float64; ac int64)
                       cases            JSON: name -> family, mode, value, full_scale_count, area_dimension, h, w and
                         cuts           [P+1] packet k = rows[rows_at + cuts[k] : rows_at + cuts[k+1]]
                         nframes        [P] numFramesWritten after every packet: packet k returned frames nframes[k-1] ..
                                        nframes[k]-1 of the case ([h,w] float64 in 0..1 each, from frames[frames_at:]), or None
                         has_cur        [P] whether currentFrame was an array after packet k; those that were lie one after
                                        the other ([h,w] float64 each) from cur[cur_at:]
                         ac_shape       (nw, nh): area_counts after every packet, [P,nw,nh] from ac[ac_at:] (AREA_COUNT)
                         start_at       currentFrameStartTime after every packet, [P] from start[start_at:] (DURATION)
                         times_at       the time of every frame written, [nframes[-1]] from times[times_at:]
(tests/renderer_ref.py: load_fixture reads it back into one record per case.)

Sensor 24x32 (h x w), 12x16 for the down-scaled histogram cases; time stamps k * 2^-8 unless the case says otherwise.
Families: area_one_cell, area_cells, area_carry, duration_grid, duration_offgrid, count, source, hist.

Dropped cases: none of the listed ones.  `area_count` <= 1 is not generated at all: the reference does not return for it (the
trigger event ends its own window again and again), and v2e_render_area_segments refuses it.
"""
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
from make_golden_render_run import TimesTap  # noqa: E402

H, W = 24, 32
GRID = 2.0 ** -8
INTERVAL = 2.0 ** -6
VIDEO = "dvs-video.avi"


def events(k, x, y, p):
    """[n,4] float32 rows with stamps k * 2^-8."""
    ev = np.zeros((len(k), 4), dtype=np.float32)
    ev[:, 0] = np.asarray(k, dtype=np.float64) * GRID
    ev[:, 1], ev[:, 2], ev[:, 3] = x, y, p
    return ev


def in_cells(rng, cells, dim, k0=0):
    """One event per entry of `cells` ((cx, cy) pairs) at a random pixel of that cell, random polarity, consecutive stamps."""
    cells = np.asarray(cells).reshape(-1, 2)
    n = len(cells)
    return events(k0 + np.arange(n), cells[:, 0] * dim + rng.integers(0, dim, n), cells[:, 1] * dim + rng.integers(0, dim, n),
                  rng.choice([1, -1], n))


def hist_packet(h, w):
    """The histogram rule: the edge coordinates of the output, bins past full scale, cancelling bins, odd polarities.  The last
    event is never accumulated."""
    rows = []
    for x in (0, w - 1, w - 0.1, w):
        for y in (0, h - 1, h - 0.1, h):
            rows.append((x, y, 1))
    rows += [(3, 2, 1)] * 5 + [(4, 2, -1)] * 5  # more than fs ON / OFF events in one bin
    rows += [(5, 2, 1), (5, 2, -1)] * 3  # ON and OFF cancel
    rows += [(6, 2, 1), (6, 2, 1), (6, 2, -1)]
    rows += [(7, 2, 0)] * 2 + [(8, 2, 0), (8, 2, 1), (8, 2, 1)]  # polarity 0 counts as OFF
    rows += [(9, 2, 2), (9, 3, 0.5), (9, 4, -2)]  # and so does everything else that is not 1
    rows += [(5.5, 3.99, 1), (5.99, 3.01, 1), (6.0, 4.0, -1), (10.5, 5.5, 1)]  # fractional coordinates
    rows.append((1, 1, 1))
    a = np.array(rows, dtype=np.float64)
    return events(np.arange(len(a)), a[:, 0], a[:, 1], a[:, 2])


def build_cases():
    """name -> (family, mode, value, fs, area_dimension, (h, w), [packets])."""
    cases = {}

    def add(name, family, mode, value, packets, fs=3, dim=None, size=(H, W)):
        assert name not in cases and all(len(p) <= 300 for p in packets)
        cases[name] = (family, mode, value, fs, dim, size, [np.ascontiguousarray(p, dtype=np.float32) for p in packets])

    # AREA_COUNT, one cell: triggers in lane 0, lane 63 and mid-chunk, many per chunk, on n - 2 and on n - 1
    for ac in (2, 3, 5, 63, 64, 65):
        for n in (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 200):
            rng = np.random.default_rng(1000 * ac + n)
            add("area1_c%d_n%d" % (ac, n), "area_one_cell", "area_count", ac, [in_cells(rng, [(1, 1)] * n, 8)], dim=8)

    # AREA_COUNT, several cells
    rng = np.random.default_rng(11)
    add("area_two_cells_c3", "area_cells", "area_count", 3, [in_cells(rng, [(0, 0), (2, 1)] * 65, 8)], dim=8)
    add("area_three_cells_c4", "area_cells", "area_count", 4,
        [in_cells(rng, np.array([(0, 0), (3, 2), (1, 2)])[rng.integers(0, 3, 150)], 8)], dim=8)
    for dim, ac in ((8, 3), (16, 4)):
        n = 140
        add("area_borders_dim%d_c%d" % (dim, ac), "area_cells", "area_count", ac,
            [events(np.arange(n), rng.choice([0, 7.9, 8.0, 15.5, 16, 24, 31], n), rng.choice([0, 7.9, 8.0, 16, 23], n),
                    rng.choice([1, -1], n))], dim=dim)
    add("area_random_dim16_c5", "area_cells", "area_count", 5,
        [events(np.arange(200), rng.integers(0, W, 200), rng.integers(0, H, 200), rng.choice([1, -1], 200))], dim=16)

    # AREA_COUNT, carried counters: packet 0 leaves area_count - 1 in cell A (and 2 in B), event 0 of packet 1 triggers;
    # packet 2 ends on a trigger (on its last event, or on the one before), packet 3 follows
    A, B, Cc = (1, 1), (3, 0), (2, 2)
    for L, tail in ((1, 5), (2, 6), (5, 5), (70, 6)):
        rng = np.random.default_rng(20 + L)
        p0 = in_cells(rng, [A, B, A, A, B, A], 8, 0)
        p1 = in_cells(rng, [A] + [B, A, Cc, A][:max(L - 1, 0)] + [A] * max(L - 5, 0), 8, 10)
        p2 = in_cells(rng, [(0, 2)] * tail, 8, 100)  # (0, 2) is untouched so far: its fifth event triggers
        p3 = in_cells(rng, [A, A, B, A, A, A, A, B], 8, 120)
        add("area_carry_next%d" % L, "area_carry", "area_count", 5, [p0, p1, p2, p3], dim=8)
    rng = np.random.default_rng(31)
    packets, k = [], 0
    for _ in range(70):  # more packets than one block of the run kernels, the counters carried through all of them
        n = int(rng.integers(1, 10))
        packets.append(in_cells(rng, np.array([A, B])[rng.integers(0, 2, n)], 8, k))
        k += n
    add("area_carry_long", "area_carry", "area_count", 5, packets, dim=8)

    # DURATION on the binary grid: interval 2^-6 = 4 grid steps, so every boundary can be hit exactly
    def grid(rng, k):
        n = len(k)
        return events(k, rng.integers(0, W, n), rng.integers(0, H, n), rng.choice([1, -1], n))

    rng = np.random.default_rng(41)
    base = 16 * 256 + 3  # 16 s + 3 grid steps
    add("dur_grid_every", "duration_grid", "duration", INTERVAL, [grid(rng, base + np.arange(100))])
    add("dur_grid_multi", "duration_grid", "duration", INTERVAL, [grid(rng, base + np.repeat(np.arange(40), 3))])
    add("dur_grid_sl_on", "duration_grid", "duration", INTERVAL, [grid(rng, base + np.r_[np.arange(20), 24, 25])])
    add("dur_grid_sl_past", "duration_grid", "duration", INTERVAL, [grid(rng, base + np.r_[np.arange(20), 25, 26])])
    add("dur_grid_sl_on_twice", "duration_grid", "duration", INTERVAL, [grid(rng, base + np.r_[np.arange(20), 24, 24, 24])])
    add("dur_grid_n1", "duration_grid", "duration", INTERVAL, [grid(rng, [base])])
    add("dur_grid_n2", "duration_grid", "duration", INTERVAL, [grid(rng, [base, base + 400])])
    add("dur_grid_n3_far", "duration_grid", "duration", INTERVAL, [grid(rng, [base, base + 12, base + 400])])
    add("dur_grid_same", "duration_grid", "duration", INTERVAL, [grid(rng, [base] * 20)])
    add("dur_grid_long_interval", "duration_grid", "duration", 1.0, [grid(rng, base + np.arange(50))])
    add("dur_grid_carry", "duration_grid", "duration", INTERVAL,  # the start time carried; gaps give empty complete frames
        [grid(rng, base + np.arange(31)), grid(rng, base + 52 + np.arange(9)), grid(rng, [base + 61]),
         grid(rng, [base + 64, base + 100]), grid(rng, base + 100 + np.repeat(np.arange(0, 40, 2), 2))])
    packets, k = [], base
    for _ in range(70):  # more than the 64 packets the window kernel holds at a time
        n = int(rng.integers(1, 13))
        steps = rng.choice([0, 1, 1, 2, 4], n)
        packets.append(grid(rng, k + np.cumsum(steps)))
        k += int(steps.sum()) + int(rng.choice([0, 1, 9]))
    add("dur_grid_long", "duration_grid", "duration", INTERVAL, packets)

    # DURATION off the grid: stamps near 1000 s, interval 1 / 300 (what numpy makes of float32 + float decides the frames)
    rng = np.random.default_rng(51)
    t = (1000.0 + np.cumsum(rng.uniform(0, 0.0012, 260))).astype(np.float32)
    ev = grid(rng, np.zeros(260))
    ev[:, 0] = t
    add("dur_off_1000", "duration_offgrid", "duration", 1 / 300.0, [ev[:120], ev[120:121], ev[121:]])

    # COUNT
    rng = np.random.default_rng(61)
    lens = (1, 2, 50, 51, 52, 100, 101, 102)
    for n in lens:
        add("count50_n%d" % n, "count", "count", 50, [grid(rng, np.arange(n))])
    add("count1_n5", "count", "count", 1, [grid(rng, np.arange(5))])
    offs = np.concatenate(([0], np.cumsum(lens)))
    add("count50_seq", "count", "count", 50, [grid(rng, np.arange(a, b)) for a, b in zip(offs, offs[1:])])

    # SOURCE
    add("source_seq", "source", "source", None, [grid(rng, [0]), grid(rng, [5, 6]), grid(rng, 10 + np.arange(7))])

    # the histogram rule, emitted (SOURCE) and left behind (DURATION with an interval longer than the packet), and with the
    # edge coordinates in the first of several windows
    for fs in (1, 3):
        for (h, w) in ((H, W), (H // 2, W // 2)):
            pk = hist_packet(h, w)
            add("hist_source_fs%d_%dx%d" % (fs, h, w), "hist", "source", None, [pk], fs=fs, size=(h, w))
            add("hist_open_fs%d_%dx%d" % (fs, h, w), "hist", "duration", 1.0, [pk], fs=fs, size=(h, w))
            tail = grid(np.random.default_rng(71), int(pk[-1, 0] / GRID) + 1 + np.arange(12))
            tail[:, 1:3] //= 2
            add("hist_first_window_fs%d_%dx%d" % (fs, h, w), "hist", "count", len(pk), [np.concatenate((pk, tail))], fs=fs,
                size=(h, w))
    return cases


def main():
    rh.install_stubs()
    from v2ecore.renderer import EventRenderer, ExposureMode
    modes = {"duration": ExposureMode.DURATION, "count": ExposureMode.COUNT, "source": ExposureMode.SOURCE,
             "area_count": ExposureMode.AREA_COUNT}
    meta = {}
    pool = {"rows": [], "frames": [], "cur": [], "ac": [], "start": [], "times": []}  # what every case adds, in case order

    def put(key, arr):
        """Append to the pool `key`; returns the element offset the data starts at."""
        at = sum(a.size for a in pool[key]) if key != "rows" else sum(len(a) for a in pool[key])
        pool[key].append(np.asarray(arr))
        return at

    for name, (family, mode, value, fs, dim, (h, w), packets) in build_cases().items():
        with tempfile.TemporaryDirectory() as tmp:
            r = EventRenderer(full_scale_count=fs, output_path=tmp, dvs_vid=VIDEO, exposure_mode=modes[mode],
                              exposure_value=value if value is not None else 1 / 300.0, area_dimension=dim)
            r.width, r.height = w, h
            r._check_outputs_open()
            tap = r.frame_times_output_file = TimesTap(r.frame_times_output_file)
            frames, cur, has_cur, ac, start, nframes, empty_first = [], [], [], [], [], [], 0
            for k, pk in enumerate(packets):
                before = None if r.area_counts is None else r.area_counts.max()
                fr = r.render_events_to_frames(pk.copy(), height=h, width=w, return_frames=True)
                if fr is not None:
                    assert fr.dtype == np.float64 and fr.shape[1:] == (h, w)
                    frames.append(fr)
                    empty_first += mode == "area_count" and bool(np.all(fr[0] == 0.5)) and before == value - 1
                has_cur.append(int(r.currentFrame is not None))
                if r.currentFrame is not None:
                    assert r.currentFrame.dtype == np.float64 and r.currentFrame.shape == (h, w)
                    cur.append(r.currentFrame)
                if mode == "area_count":
                    ac.append(np.array(r.area_counts, dtype=np.int64))
                if mode == "duration":
                    start.append(np.float64(r.currentFrameStartTime))
                nframes.append(int(r.numFramesWritten))
                assert nframes[-1] == sum(len(f) for f in frames)
            r.cleanup()
        assert len(tap.times) == r.numFramesWritten
        if family == "area_carry":  # the carried counter did fire on event 0 of a later packet
            assert empty_first >= (3 if name.endswith("long") else len(packets[1]) > 1), (name, empty_first)
            if not name.endswith("long"):
                assert ac[0][1, 1] == 4 and (len(packets[1]) > 1 or not ac[1].any()), name
                assert len(packets[2]) != 5 or (not ac[2].any() and has_cur[2]), name
        meta[name] = dict(family=family, mode=mode, value=value, full_scale_count=fs, area_dimension=dim, h=h, w=w,
                          cuts=[int(c) for c in np.concatenate(([0], np.cumsum([len(p) for p in packets])))],
                          nframes=nframes, has_cur=has_cur,
                          rows_at=put("rows", np.concatenate(packets)),
                          frames_at=put("frames", np.concatenate(frames).ravel() if frames else np.zeros(0)),
                          cur_at=put("cur", np.concatenate(cur).ravel() if cur else np.zeros(0)),
                          ac_at=put("ac", np.stack(ac).ravel() if ac else np.zeros(0, np.int64)),
                          ac_shape=list(ac[0].shape) if ac else None,
                          start_at=put("start", np.array(start, dtype=np.float64)),
                          times_at=put("times", np.array(tap.times, dtype=np.float64)))
        print("%-28s packets %2d  events %4d  frames %3d" % (name, len(packets), sum(len(p) for p in packets), r.numFramesWritten))
    out = {k: np.concatenate(v) for k, v in pool.items()}
    assert out["rows"].dtype == np.float32 and out["ac"].dtype == np.int64 and out["frames"].dtype == np.float64
    out["cases"] = np.array(json.dumps(meta, sort_keys=True))
    out["numpy_version"] = np.array(np.__version__)
    out["f32_time"] = np.array(int(type(np.float32(0) + 0.5) is np.float32), dtype=np.int64)
    path = os.path.join(HERE, "renderer_edges.npz")
    with zipfile.ZipFile(path, "w") as zf:  # np.savez_compressed, with a fixed date in every entry: reruns give the same bytes
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print("renderer_edges.npz", os.path.getsize(path) // 1024, "KB,", len(meta), "cases")


if __name__ == "__main__":
    main()
