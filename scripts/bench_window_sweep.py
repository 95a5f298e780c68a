#!/usr/bin/env python
"""WindowSweep.add_run on the rows of one emulator run, beside what it replaces: the definitional numpy loop on the host, once per
(L, sigma, k).

Workload: that of scripts/bench_denoise_sweep.py (profiles/r15_denoise_sweep.txt), so that the numbers stand beside DenoiseSweep's:
300 frames of scripts/moving_dot.py at 346 x 260 (rendered on the device, dt 100 us) through one Philox-mode emulator with
set_dvs_params("noisy") and shot_noise_rate_hz 50, seed 5; labels from the run's counts and EventEmulator.last_n_signal.  Two
tables: 64 window lengths up to 1024 (1 .. 32, then log-spaced) and the 64 lengths 1 .. 64, each with the 8 sigmas 0, 1, 2, 3, 4,
6, 8, 12.

Everything runs in one process on one GPU.  Each timing starts with the device idle and ends behind a device synchronise (host
clock); a round times `--inner` consecutive add_run calls of each table, the tables alternating; median, minimum and maximum over
`--rounds` rounds.  The device's count and mask for one (L, sigma, k) are compared first with the host loop's on the rows the loop
is timed on (equal, or the script stops).

  python scripts/bench_window_sweep.py [--rounds 5] [--inner 20] [--out profiles/r27_window_sweep.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_window_sweep.py --trace-runs 20       # the kernels of add_run, traced
  python scripts/bench_window_sweep.py --kernel-stats DIR [--out FILE]                                  # ... summed per add_run (appended)
"""
import argparse
import csv
import glob
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_denoise_sweep import FRAMES, H, SEED, W, workload  # noqa: E402  (the workload itself, not a copy of it)

LONG_LENGTHS = list(range(1, 33)) + [int(v) for v in np.round(np.geomspace(36, 1024, 32))]
SHORT_LENGTHS = list(range(1, 65))
SIGMAS = [0, 1, 2, 3, 4, 6, 8, 12]
HOST_L, HOST_SIGMA, HOST_K = LONG_LENGTHS[44], 6, 2  # (table entries: the histogram holds the same count)
TABLES = (("64 lengths up to 1024, 8 sigmas", LONG_LENGTHS), ("64 lengths up to 64, 8 sigmas", SHORT_LENGTHS))


def host_loop(rows, L, sigma, k):
    """The definition as a user would write it on the host for ONE (L, sigma, k): a ring of the last L coordinates and a loop over
    the rows (all valid: the workload has no bad row).  Returns the keep mask."""
    far = -(1 << 20)  # (an empty slot is further away than any sigma)
    bx, by = np.full(L, far, dtype=np.int64), np.full(L, far, dtype=np.int64)
    keep = np.zeros(len(rows), dtype=bool)
    xs, ys = rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64)
    for i in range(len(rows)):
        x, y = xs[i], ys[i]
        keep[i] = np.count_nonzero(np.abs(bx - x) + np.abs(by - y) <= sigma) >= k
        bx[i % L], by[i % L] = x, y
    return keep


def kernel_stats(d, say):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        sys.exit("no kernel_stats.csv under %s" % d)
    ours = [r for r in rows if "k_window" in r["Name"]]
    calls = max(int(r["Calls"]) for r in ours if "k_window_tail" in r["Name"])
    groups = {"torch bookkeeping (zeroed counters)": []}
    other = []
    for r in rows:
        name = r["Name"]
        if "k_window" in name:
            groups.setdefault(re.search(r"k_window_\w+(<[\w ,]+>)?", name).group(0), []).append(r)
        elif "FillFunctor<long>" in name:
            groups["torch bookkeeping (zeroed counters)"].append(r)
        else:
            other.append(r)
    say("")
    say("rocprofv3 --kernel-trace --stats of %d add_run calls (a run of its own; %s), kernel time per add_run:" % (calls, TABLES[0][0]))
    say("%-66s %8s %12s" % ("kernel", "calls", "us / add_run"))
    per = {}
    for name, rs in groups.items():
        n = sum(int(r["Calls"]) for r in rs)
        tot = sum(float(r["TotalDurationNs"]) for r in rs)
        per[name] = tot / calls / 1e3
        say("%-66s %8d %12.1f" % (name[:66], n, per[name]))
    say("sum: %.1f us, of which the kernels of window.hip %.1f us" % (sum(per.values()), sum(v for k, v in per.items() if k.startswith("k_window"))))
    say("not part of add_run (the emulator runs and the frames of the workload): %d launches, %.1f us in all"
        % (sum(int(r["Calls"]) for r in other), sum(float(r["TotalDurationNs"]) for r in other) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rate", type=float, default=50.0, help="shot_noise_rate_hz of the emulator run")
    ap.add_argument("--long-copies", type=int, default=32, help="copies of the rows in the long run")
    ap.add_argument("--trace-runs", type=int, default=0, help="only run add_run this often (for rocprofv3) and exit")
    ap.add_argument("--kernel-stats", help="summarise the kernel_stats.csv of a rocprofv3 run under this directory, appended to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_window_sweep.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.kernel_stats:
        kernel_stats(args.kernel_stats, say)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_window_sweep.py needs a GPU")
    from v2e_amd import WindowSweep
    dev = "cuda:0"
    rows, counts, n_signal, emu_sec = workload(args.rate, dev)
    n = int(rows.shape[0])

    def sweep(lengths=LONG_LENGTHS):
        return WindowSweep(H, W, lengths, SIGMAS, device=dev)

    def run(ws, times=1):
        for _ in range(times):
            ws.add_run(rows, counts, 0, n_signal=n_signal)

    if args.trace_runs:
        run(sweep(), args.trace_runs)
        torch.cuda.synchronize()
        return

    ws = sweep()
    run(ws)
    r = ws.result()
    say("window sweep: FWF k = 1 .. 4 x %d sigmas %d .. %d x %d lengths %d .. %d on the rows of %d frames %dx%d of moving_dot (dt 100 us), "
        "noisy preset with shot_noise_rate_hz %g, seed %d" % (len(SIGMAS), SIGMAS[0], SIGMAS[-1], len(LONG_LENGTHS), LONG_LENGTHS[0],
                                                               LONG_LENGTHS[-1], FRAMES, W, H, args.rate, SEED))
    say("device: %s" % torch.cuda.get_device_name(0))
    say("rows %d: signal %d, noise %d (%.1f %%), bad %d; the emulator run that made them: %.2f ms"
        % (n, r.n_signal, r.n_noise, 100.0 * r.n_noise / max(n, 1), r.n_bad, emu_sec * 1e3))
    L, sigma, k, tpr, fpr = r.best()
    say("best tpr - fpr: L = %d, sigma = %d, k = %d, tpr %.4f, fpr %.4f" % (L, sigma, k, tpr, fpr))

    # the host loop for one (L, sigma, k), and the device's count for the same rows
    host_rows = rows.cpu().numpy()
    t0 = time.perf_counter()
    keep = host_loop(host_rows, HOST_L, HOST_SIGMA, HOST_K)
    host_sec = time.perf_counter() - t0
    ws = sweep()
    out = ws.add_run(rows, keep=(HOST_L, HOST_SIGMA, HOST_K))
    passed = int(ws.result().passed[HOST_K - 1, SIGMAS.index(HOST_SIGMA), :, LONG_LENGTHS.index(HOST_L)].sum())
    if not np.array_equal(out["mask"].cpu().numpy(), keep) or passed != int(keep.sum()):
        say("MISMATCH between the host loop (%d rows pass) and the device (%d in the histogram, %d in the mask)"
            % (int(keep.sum()), passed, int(out["mask"].sum())))
        sys.exit(1)
    settings = 4 * len(SIGMAS) * len(LONG_LENGTHS)
    say("host loop, one (L, sigma, k) = (%d, %d, %d): %.2f s on %d rows (%d pass, as on the device); all %d (L, sigma, k): %.0f s"
        % (HOST_L, HOST_SIGMA, HOST_K, host_sec, n, int(keep.sum()), settings, host_sec * settings))

    legs = {name: (lambda ws=sweep(lengths): run(ws)) for name, lengths in TABLES}
    t = {name: [] for name in legs}
    for rnd in range(-1, args.rounds):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            if rnd >= 0:
                t[name].append((time.perf_counter() - t0) / args.inner * 1e3)
    say("")
    say("add_run per call, host clock from idle device to device idle; %d rounds alternating, %d consecutive calls each" % (args.rounds, args.inner))
    say("%-44s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"))
    med = {}
    for name, v in t.items():
        v = np.sort(np.array(v))
        med[name] = float(np.median(v))
        say("%-44s %10.3f %10.3f %10.3f" % (name, med[name], v[0], v[-1]))
    first = TABLES[0][0]
    say("")
    say("%s: rows per second: %.3g; add_run / emulator run: %.2f; host loop for all (L, sigma, k) / add_run: %.3g"
        % (first, n / (med[first] * 1e-3), med[first] * 1e-3 / emu_sec, host_sec * settings / (med[first] * 1e-3)))

    # the same rows several times over: a run long enough that launches do not dominate, and the scratch of one pass measured (torch's
    # allocator: peak over the call minus what was allocated before it)
    reps = args.long_copies
    big = rows.repeat(reps, 1)
    nb = int(big.shape[0])
    say("")
    say("long run: the rows %d times over, %d rows in one pass (labels: all signal), %d rounds of %d calls" % (reps, nb, 3, 3))
    for name, lengths in TABLES:
        ws = sweep(lengths)
        ws.add_run(big)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ws.add_run(big)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        v = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                ws.add_run(big)
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) / 3 * 1e3)
        say("%s: add_run median %.3f ms (min %.3f, max %.3f), %.3g rows/s; peak scratch %.1f bytes per row"
            % (name, float(np.median(v)), min(v), max(v), nb / (float(np.median(v)) * 1e-3), peak / nb))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
