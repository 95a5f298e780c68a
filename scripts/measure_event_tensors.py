#!/usr/bin/env python
"""Event tensors of one device-resident run: EventTensorizer.add_run + flush for each representation (count, voxel,
time_surface) against EventRenderer.render_run + flush_run (DURATION) on the same rows -- the DVS video pass is the yardstick:
existing code that reads the same rows and scatters them with the same kind of atomics.

Workload (that of scripts/measure_render_run.py): 346x260, Philox, set_dvs_params('noisy'), one run of 300 frames at 1/300 s;
windows of 1/300 s.  Each repetition uses a fresh EventTensorizer / EventRenderer, starts with the device idle and ends with a
device synchronise (host clock around it); the tensorizer and the renderer alternate within one process, after warm-up
repetitions of both; median, minimum and the 10th / 90th percentiles of `--reps` repetitions are printed.  The tensors are
compared with the numpy definition (tests/event_tensors_ref.py) first.

  python scripts/measure_event_tensors.py [--reps 40] [--frames 300]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=300, leak_rate_hz=0.01, shot_noise_rate_hz=0.001,
          refractory_period_s=0.0005)
H, W, BS, BINS = 260, 346, 8, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--frames", type=int, default=300)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_event_tensors.py needs a GPU")
    from event_tensors_ref import event_tensors, uniform_bounds
    from v2e_amd import EventEmulator, EventTensorizer
    from v2e_amd.renderer import EventRenderer, ExposureMode
    from v2e_amd.synth import int_gradient_frames
    n = args.frames
    frames = int_gradient_frames(n + 1, H, W, seed=1, noise=6, as_array=True)
    times = [i / 300 for i in range(n + 1)]
    emu = EventEmulator(device="cuda", seed=8, rng_mode="philox", **KW)
    emu.set_dvs_params("noisy")
    ev, counts = emu.generate_events_batch(frames, times, return_device=True)
    torch.cuda.synchronize()
    ev, counts = ev.clone(), np.asarray(counts)
    print("run: %d frames, %d events; windows of 1/300 s, %d voxel bins" % (n, int(counts.sum()), BINS))

    def tensorize(rep):
        tz = EventTensorizer(H, W, representations=(rep,), window_s=1 / 300.0, voxel_bins=BINS, frame_times=times)
        a = tz.add_run(ev, counts, 0)
        b = tz.flush()
        return tz, (a, b)

    def render(_):
        r = EventRenderer(exposure_mode=ExposureMode.DURATION, exposure_value=1 / 300.0)
        a = r.render_run(ev, counts, H, W, frame0=0, batch_size=BS)
        b = r.flush_run(H, W)
        return r, (a, b)

    # the tensors are right first (the definition on the host copy of the rows)
    host = ev.cpu().numpy()
    ref = None
    for rep in ("count", "voxel", "time_surface"):
        tz, (a, b) = tensorize(rep)
        got = torch.cat((a[rep], b[rep])).cpu().numpy()
        if ref is None:
            ref = event_tensors(host, uniform_bounds(0.0, 1 / 300.0, got.shape[0]), H, W, bins=BINS)
        assert got.shape == ref[rep].shape and np.array_equal(got.view(np.uint32), ref[rep].view(np.uint32)), rep
        c = tz.check()
        print("%-12s %s %s, %d windows, matches the definition; read-backs before check(): %d; skipped rows: %r"
              % (rep, got.dtype, list(got.shape), got.shape[0], tz.host_syncs - 1, c))
    del ref, host, got, a, b, tz

    for rep in ("count", "voxel", "time_surface"):
        t = {"tensorize": [], "render_run": []}
        for i in range(-5, args.reps):
            for key, fn in (("tensorize", tensorize), ("render_run", render)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                keep = fn(rep)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                del keep
                if i >= 0:
                    t[key].append(dt * 1e3)
        print("%s (alternating with render_run + flush_run, DURATION 1/300 s)" % rep)
        med = {}
        for key in ("tensorize", "render_run"):
            v = np.sort(np.array(t[key]))
            med[key] = float(np.median(v))
            print("  %-10s median %8.3f ms   min %8.3f   p10 %8.3f   p90 %8.3f   (%d reps)"
                  % (key, med[key], v[0], v[len(v) // 10], v[(9 * len(v)) // 10], len(v)))
        print("  ratio tensorize / render_run (medians): %.2f" % (med["tensorize"] / med["render_run"]))


if __name__ == "__main__":
    main()
