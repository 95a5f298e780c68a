#!/usr/bin/env python
"""DVS video of one device-resident run: EventRenderer.render_run + flush_run (one pass) against the per-packet loop over the
same packets (render_events_to_frames(return_frames=False) for every packet of run_packets -- the only way before render_run
existed), frames left on the device in both.

Workload: 346x260, Philox, set_dvs_params('noisy'), one run of 300 frames at 1/300 s, batch_size 8 (38 packets); DURATION at
1/300 s and COUNT.  Each repetition uses a fresh EventRenderer, starts with the device idle and ends with a device synchronise
(host clock around it); the two methods alternate within one process, after warm-up repetitions of both; median, minimum and
the 10th / 90th percentiles of `--reps` repetitions are printed, and the frames of both methods are compared first.

  python scripts/measure_render_run.py [--reps 40] [--frames 300]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=300, leak_rate_hz=0.01, shot_noise_rate_hz=0.001,
          refractory_period_s=0.0005)
H, W, BS = 260, 346, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--frames", type=int, default=300)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_render_run.py needs a GPU")
    from v2e_amd import EventEmulator
    from v2e_amd.renderer import EventRenderer, ExposureMode, run_packets
    from v2e_amd.synth import int_gradient_frames
    n = args.frames
    frames = int_gradient_frames(n + 1, H, W, seed=1, noise=6, as_array=True)
    emu = EventEmulator(device="cuda", seed=8, rng_mode="philox", **KW)
    emu.set_dvs_params("noisy")
    t0 = time.perf_counter()
    ev, counts = emu.generate_events_batch(frames, [i / 300 for i in range(n + 1)], return_device=True)
    torch.cuda.synchronize()
    ev, counts = ev.clone(), np.asarray(counts)
    packets, _ = run_packets(counts, 0, BS)
    ranges = [tuple(p) for p in packets.tolist()] + [(int(packets[-1, 1]), int(counts.sum()))]
    ranges = [(a, b) for a, b in ranges if b > a]
    print("run: %d frames, %d events, %d packets of %d..%d events (emulator run incl. upload %.1f ms, first call)"
          % (n, int(counts.sum()), len(ranges), min(b - a for a, b in ranges), max(b - a for a, b in ranges),
             (time.perf_counter() - t0) * 1e3))

    def per_packet(kw, return_frames=False):
        r = EventRenderer(**kw)
        out = [r.render_events_to_frames(ev[a:b], H, W, return_frames=return_frames) for a, b in ranges]
        return r, out

    def one_pass(kw, return_frames=True):
        r = EventRenderer(**kw)
        a = r.render_run(ev, counts, H, W, frame0=0, batch_size=BS, return_frames=return_frames)
        b = r.flush_run(H, W, return_frames=return_frames)
        return r, (a, b)

    for name, kw in (("DURATION 1/300 s", dict(exposure_mode=ExposureMode.DURATION, exposure_value=1 / 300.0)),
                     ("COUNT 20000", dict(exposure_mode=ExposureMode.COUNT, exposure_value=20000))):
        # same results first
        rl, out = per_packet(kw, return_frames=True)
        want = np.concatenate([f for f in out if f is not None])
        rr, (a, b) = one_pass(kw)
        got = torch.cat([p[0] for p in (a, b) if p[0] is not None]).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), name
        assert torch.equal(rr.currentFrame, rl.currentFrame)
        t = {"per_packet": [], "one_pass": []}
        for rep in range(-5, args.reps):
            for key, fn in (("per_packet", per_packet), ("one_pass", one_pass)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                keep = fn(kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                del keep
                if rep >= 0:
                    t[key].append(dt * 1e3)
        print("%s: %d DVS frames, %d read-backs per one-pass clip" % (name, len(want), rr.host_syncs))
        med = {}
        for key in ("per_packet", "one_pass"):
            v = np.sort(np.array(t[key]))
            med[key] = float(np.median(v))
            print("  %-10s median %8.3f ms   min %8.3f   p10 %8.3f   p90 %8.3f   (%d reps)"
                  % (key, med[key], v[0], v[len(v) // 10], v[(9 * len(v)) // 10], len(v)))
        print("  ratio per_packet / one_pass (medians): %.2f" % (med["per_packet"] / med["one_pass"]))


if __name__ == "__main__":
    main()
