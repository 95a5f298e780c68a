#!/usr/bin/env python
"""ThresholdSweep.run against what it replaces: one fresh Philox-mode emulator run per threshold, rows counted on the device.

Workload: the reference's 95 thresholds (np.arange(1, 0.05, -0.01), dataset_scripts/ddd/ddd_find_thresholds.py:110) on 300 frames
of the BASELINE configs[0] source (scripts/moving_dot.py, rendered on the device) at 346 x 260, the emulator's default model
parameters, counts inside a central ROI.

Both legs run in one process on one GPU and alternate round by round after a warm-up round of each; every timing starts with the
device idle and ends behind the read-back of the counts (host clock).  A round times `--inner` consecutive sweeps for each column
chunk (cols_per_thread 4, 8, 16: the same kernel template), ONE pass of 95 fresh emulators and ONE pass of one emulator that is
reset() and given new thresholds per column (what ddd_find_thresholds.py does); median, minimum and maximum over `--rounds` rounds
are reported.  The two legs' counts are compared first (equal, or the script stops).

  python scripts/bench_threshold_sweep.py [--rounds 5] [--inner 10] [--out profiles/r14_threshold_sweep.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, FRAMES = 260, 346, 300
ROI = ((53, 292), (40, 219))
SEED = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--frames", type=int, default=FRAMES)
    # (with sigma_thres 0.03 a few percent of the pixels of the lowest columns sit at the 0.01 clamp: a dot crossing one fires some
    # 300 events in a frame, past the emulator's default max_iters of 64, which makes the run fail)
    ap.add_argument("--max-iters", type=int, default=512, help="of the emulators of the per-threshold leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_threshold_sweep.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_threshold_sweep.py needs a GPU")
    from v2e_amd import EventEmulator, ThresholdSweep, _capi
    from v2e_amd.sweep import count_rows_in_roi
    from v2e_amd.synthetic import moving_dot

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dev = "cuda:0"
    thresholds = np.arange(1, 0.05, -0.01)
    T = len(thresholds)
    frames, times = moving_dot(W, H, arg_list=["--cycles", "1"], device=dev).frames_block(0, args.frames)
    times = [float(t) for t in times]
    torch.cuda.synchronize()
    say("threshold sweep: %d thresholds %.2f .. %.2f, %d frames %dx%d of moving_dot (dt %.0f us), ROI x %r y %r, seed %d, default model "
        "parameters (sigma_thres 0.03, leak_rate_hz 0.1, no cutoff: float32 state, no refractory period)"
        % (T, thresholds[0], thresholds[-1], len(times), W, H, (times[1] - times[0]) * 1e6, ROI[0], ROI[1], SEED))
    say("device: %s; emulators of the per-threshold leg: max_iters=%d (the default 64 fails at the lowest thresholds)"
        % (torch.cuda.get_device_name(0), args.max_iters))

    def sweep(cols):
        sw = ThresholdSweep(H, W, thresholds, roi=ROI, seed=SEED, device=dev, cols_per_thread=cols)
        r = sw.run(frames, times)
        return r, sw.recomputed_columns

    def per_threshold(reuse=False):
        """One emulator run per threshold: a fresh EventEmulator each, or (reuse) one instance with reset() and new thresholds per
        column, as ddd_find_thresholds.py:132-137 does."""
        on, off = [], []
        emu = None
        for th in thresholds:
            if emu is None:
                emu = EventEmulator(pos_thres=float(th), neg_thres=float(th), rng_mode="philox", seed=SEED, device=dev,
                                    max_iters=args.max_iters)
            else:
                emu.pos_thres = emu.neg_thres = float(th)
                emu.reset()
                emu.t_previous = 0  # (reset() keeps the clock, as the reference's does; the clip starts over)
            ev, _ = emu.generate_events_batch(frames, times, return_device=True)
            c = count_rows_in_roi(ev, ROI).cpu().tolist()
            del ev
            if not reuse:
                emu.cleanup()
                emu = None
            on.append(c[0])
            off.append(c[1])
        if emu is not None:
            emu.cleanup()
        return np.array(on, np.int64), np.array(off, np.int64)

    # the two legs compute the same thing (also the warm-up of both)
    ref_on, ref_off = per_threshold()
    re_on, re_off = per_threshold(reuse=True)
    if not (np.array_equal(re_on, ref_on) and np.array_equal(re_off, ref_off)):
        say("MISMATCH between fresh emulators and one emulator with reset()")
        sys.exit(1)
    recomputed = 0
    for cols in (4, 8, 16, 0):
        r, recomputed = sweep(cols)
        if not (np.array_equal(r.on, ref_on) and np.array_equal(r.off, ref_off)):
            say("MISMATCH cols_per_thread=%d\n on  %r\n ref %r\n off %r\n ref %r" % (cols, r.on.tolist(), ref_on.tolist(), r.off.tolist(),
                                                                             ref_off.tolist()))
            sys.exit(1)
    say("counts: sweep == %d emulator runs for cols_per_thread 4, 8, 16 and the default; ON %d .. %d, OFF %d .. %d; columns recomputed by "
        "the emulator: %d" % (T, ref_on.min(), ref_on.max(), ref_off.min(), ref_off.max(), recomputed))

    lib = _capi.lib()
    info = {}
    for cols in (4, 8, 16, 0):
        c_out, vg, occ = C.c_int(0), C.c_int(0), C.c_int(0)
        _capi.check(lib.v2e_thres_sweep_info(0, 0, cols, C.byref(c_out), C.byref(vg), C.byref(occ)), "v2e_thres_sweep_info")
        info[cols] = (c_out.value, vg.value, occ.value)
    default_cols = info[0][0]

    t_sweep = {4: [], 8: [], 16: []}
    t_emus, t_reuse = [], []
    for rnd in range(-1, args.rounds):
        for cols in (4, 8, 16):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                sweep(cols)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.inner
            if rnd >= 0:
                t_sweep[cols].append(dt * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_threshold()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rnd >= 0:
            t_emus.append(dt * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_threshold(reuse=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rnd >= 0:
            t_reuse.append(dt * 1e3)

    def stat(v):
        v = np.sort(np.array(v))
        return float(np.median(v)), float(v[0]), float(v[-1])

    say("")
    say("per call, host clock from idle device to counts on the host; %d rounds alternating, sweeps averaged over %d consecutive calls"
        % (args.rounds, args.inner))
    say("%-44s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"))
    med = {}
    for cols in (4, 8, 16):
        m, lo, hi = stat(t_sweep[cols])
        med[cols] = m
        say("%-44s %10.3f %10.3f %10.3f   VGPRs %d, workgroups/CU %d (%d waves/SIMD)"
            % ("ThresholdSweep.run, cols_per_thread=%d" % cols, m, lo, hi, info[cols][1], info[cols][2], info[cols][2]))
    m_e, lo_e, hi_e = stat(t_emus)
    say("%-44s %10.3f %10.3f %10.3f" % ("%d x fresh EventEmulator + batch run + count" % T, m_e, lo_e, hi_e))
    m_r, lo_r, hi_r = stat(t_reuse)
    say("%-44s %10.3f %10.3f %10.3f" % ("%d x (reset + thresholds) + batch run + count" % T, m_r, lo_r, hi_r))
    best = min(med, key=med.get)
    say("")
    say("fastest chunk by median: cols_per_thread=%d; the library's default (SWEEP_TB_DEFAULT): %d" % (best, default_cols))
    say("ratio (%d fresh emulator runs) / (sweep at the default chunk), medians: %.1f" % (T, m_e / med[default_cols]))
    say("ratio (%d runs of one emulator, reset() between) / (sweep at the default chunk), medians: %.1f" % (T, m_r / med[default_cols]))
    say("pixel-frame-columns per second of the sweep at the default chunk: %.3g"
        % (H * W * (len(times) - 1) * T / (med[default_cols] * 1e-3)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
