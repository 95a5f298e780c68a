#!/usr/bin/env python
"""DoubleWindowSweep.add_run on the rows of one emulator run, beside what it replaces (the definitional loop on the host, once per
(L, sigma, k)) and beside WindowSweep.add_run on the same rows.

Workload: that of scripts/bench_window_sweep.py (profiles/r27_window_sweep.txt): 300 frames of scripts/moving_dot.py at 346 x 260
through one Philox-mode emulator with set_dvs_params("noisy") and shot_noise_rate_hz 50, seed 5; labels from the run's counts and
EventEmulator.last_n_signal.  Three tables: 16 lengths up to 512 and 16 lengths up to 64, each with the 8 sigmas 0, 1, 2, 3, 4, 6,
8, 12 and the supports 1 .. 4 (512 settings), and the single setting (512, 3, 1).  The design rests on "512 settings cost about
what one costs" (one wavefront per setting, no wave waits for another): the ratio of the first table to the single setting is
reported.

Everything runs in one process on one GPU.  Each timing starts with the device idle and ends behind a device synchronise (host
clock); a round times `--inner` consecutive add_run calls of each leg, the legs alternating; median, minimum and maximum over
`--rounds` rounds.  The device's counts and mask for one (L, sigma, k) are compared first with the host loop's on the rows the loop
is timed on (equal, or the script stops).

  python scripts/bench_double_window_sweep.py [--rounds 5] [--inner 3] [--out profiles/r28_double_window_sweep.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_double_window_sweep.py --trace-runs 5   # traced
  python scripts/bench_double_window_sweep.py --kernel-stats DIR [--out FILE]                           # ... summed per add_run (appended)
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
from bench_window_sweep import LONG_LENGTHS as FWF_LENGTHS  # noqa: E402

LONG_LENGTHS = [int(v) for v in np.round(np.geomspace(8, 512, 16))]
SHORT_LENGTHS = [int(v) for v in np.round(np.linspace(4, 64, 16))]
SIGMAS = [0, 1, 2, 3, 4, 6, 8, 12]
SUPPORTS = [1, 2, 3, 4]
SINGLE = (512, 3, 1)
HOST = (LONG_LENGTHS[-1], 3, 1)
LEGS = (("16 lengths up to 512 x 8 sigmas x 4 supports", LONG_LENGTHS, SIGMAS, SUPPORTS),
        ("16 lengths up to 64 x 8 sigmas x 4 supports", SHORT_LENGTHS, SIGMAS, SUPPORTS),
        ("the single setting (512, 3, 1)", [SINGLE[0]], [SINGLE[1]], [SINGLE[2]]))


def host_loop(rows, L, sigma, k):
    """The definition as a user would write it on the host for ONE (L, sigma, k): two rings of L coordinates and a loop over the
    rows (all valid: the workload has no bad row).  Returns the keep mask."""
    far = -(1 << 20)  # (an empty slot is further away than any sigma)
    bx, by = np.full((2, L), far, dtype=np.int64), np.full((2, L), far, dtype=np.int64)
    at = [0, 0]
    keep = np.zeros(len(rows), dtype=bool)
    xs, ys = rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64)
    for i in range(len(rows)):
        x, y = xs[i], ys[i]
        keep[i] = np.count_nonzero(np.abs(bx - x) + np.abs(by - y) <= sigma) >= k
        w = 0 if keep[i] else 1
        bx[w, at[w] % L], by[w, at[w] % L] = x, y
        at[w] += 1
    return keep


def kernel_stats(d, say):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        sys.exit("no kernel_stats.csv under %s" % d)
    calls = max(int(r["Calls"]) for r in rows if "k_dwindow_sweep" in r["Name"])
    groups, other = {}, []
    for r in rows:
        m = re.search(r"k_d?window_\w+", r["Name"])
        if m:
            groups.setdefault(m.group(0), []).append(r)
        elif "FillFunctor<long>" in r["Name"]:
            groups.setdefault("torch bookkeeping (zeroed counters)", []).append(r)
        else:
            other.append(r)
    say("")
    say("rocprofv3 --kernel-trace --stats of %d add_run calls (a run of its own; %s), kernel time per add_run:" % (calls, LEGS[0][0]))
    say("%-66s %8s %12s" % ("kernel", "calls", "us / add_run"))
    per = {}
    for name, rs in groups.items():
        per[name] = sum(float(r["TotalDurationNs"]) for r in rs) / calls / 1e3
        say("%-66s %8d %12.1f" % (name[:66], sum(int(r["Calls"]) for r in rs), per[name]))
    say("sum: %.1f us, of which k_dwindow_sweep %.1f us" % (sum(per.values()), per["k_dwindow_sweep"]))
    say("not part of add_run (the emulator runs and the frames of the workload): %d launches, %.1f us in all"
        % (sum(int(r["Calls"]) for r in other), sum(float(r["TotalDurationNs"]) for r in other) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--rate", type=float, default=50.0, help="shot_noise_rate_hz of the emulator run")
    ap.add_argument("--trace-runs", type=int, default=0, help="only run add_run this often (for rocprofv3) and exit")
    ap.add_argument("--kernel-stats", help="summarise the kernel_stats.csv of a rocprofv3 run under this directory, appended to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_double_window_sweep.txt"))
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
        sys.exit("bench_double_window_sweep.py needs a GPU")
    from v2e_amd import DoubleWindowSweep, WindowSweep
    dev = "cuda:0"
    rows, counts, n_signal, emu_sec = workload(args.rate, dev)
    n = int(rows.shape[0])

    def sweep(lengths=LONG_LENGTHS, sigmas=SIGMAS, supports=SUPPORTS):
        return DoubleWindowSweep(H, W, lengths, sigmas, supports, device=dev)

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
    say("double window sweep: DWF %d supports x %d sigmas %d .. %d x %d lengths %d .. %d on the rows of %d frames %dx%d of moving_dot "
        "(dt 100 us), noisy preset with shot_noise_rate_hz %g, seed %d" % (len(SUPPORTS), len(SIGMAS), SIGMAS[0], SIGMAS[-1], len(LONG_LENGTHS),
                                                                          LONG_LENGTHS[0], LONG_LENGTHS[-1], FRAMES, W, H, args.rate, SEED))
    say("device: %s" % torch.cuda.get_device_name(0))
    say("rows %d: signal %d, noise %d (%.1f %%), bad %d; the emulator run that made them: %.2f ms"
        % (n, r.n_signal, r.n_noise, 100.0 * r.n_noise / max(n, 1), r.n_bad, emu_sec * 1e3))
    L, sigma, k, tpr, fpr = r.best()
    say("best tpr - fpr: L = %d, sigma = %d, k = %d, tpr %.4f, fpr %.4f" % (L, sigma, k, tpr, fpr))

    # the host loop for one (L, sigma, k), and the device's verdicts for the same rows
    host_rows = rows.cpu().numpy()
    t0 = time.perf_counter()
    keep = host_loop(host_rows, *HOST)
    host_sec = time.perf_counter() - t0
    ws = sweep()
    out = ws.add_run(rows, keep=HOST)
    passed = int(ws.result().passed[SUPPORTS.index(HOST[2]), SIGMAS.index(HOST[1]), LONG_LENGTHS.index(HOST[0])].sum())
    if not np.array_equal(out["mask"].cpu().numpy(), keep) or passed != int(keep.sum()):
        say("MISMATCH between the host loop (%d rows pass) and the device (%d in the counts, %d in the mask)"
            % (int(keep.sum()), passed, int(out["mask"].sum())))
        sys.exit(1)
    settings = len(SUPPORTS) * len(SIGMAS) * len(LONG_LENGTHS)
    say("host loop, one (L, sigma, k) = (%d, %d, %d): %.2f s on %d rows (%d pass, as on the device); all %d (L, sigma, k): %.0f s"
        % (HOST + (host_sec, n, int(keep.sum()), settings, host_sec * settings)))

    fwf = WindowSweep(H, W, FWF_LENGTHS, SIGMAS, device=dev)
    legs = {name: (lambda ws=sweep(*tables): run(ws)) for name, *tables in LEGS}
    legs["WindowSweep.add_run, 64 lengths up to 1024, 8 sigmas"] = lambda: fwf.add_run(rows, counts, 0, n_signal=n_signal)
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
    say("%-56s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"))
    med = {}
    for name, v in t.items():
        v = np.sort(np.array(v))
        med[name] = float(np.median(v))
        say("%-56s %10.3f %10.3f %10.3f" % (name, med[name], v[0], v[-1]))
    first, short, single = (leg[0] for leg in LEGS)
    say("")
    say("%s: %.1f ns per row (the slowest wave sets the pass); up to 64: %.1f ns per row; the single setting: %.1f ns per row"
        % (first, med[first] * 1e6 / n, med[short] * 1e6 / n, med[single] * 1e6 / n))
    say("512 settings / the single setting at Lmax = 512: %.2f; host loop for all %d (L, sigma, k) / add_run: %.3g"
        % (med[first] / med[single], settings, host_sec * settings / (med[first] * 1e-3)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
