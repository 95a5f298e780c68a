#!/usr/bin/env python
"""DenoiseSweep.add_run on the rows of one emulator run, beside what it replaces: the definitional numpy loop on the host, once per
(k, tau).

Workload: 300 frames of scripts/moving_dot.py at 346 x 260 (rendered on the device, dt 100 us) through one Philox-mode emulator with
set_dvs_params("noisy") and shot_noise_rate_hz raised (--rate) until the shot noise is a visible share of the rows; 64 taus,
log-spaced from 100 us to 100 ms; labels from the run's counts and EventEmulator.last_n_signal.

Everything runs in one process on one GPU.  Each timing starts with the device idle and ends behind a device synchronise (host
clock); a round times `--inner` consecutive add_run calls and the sort alone (keys + torch.sort) the same way, the two alternating;
median, minimum and maximum over `--rounds` rounds.  The device's count and mask for one (k, tau) are compared first with the host
loop's on the rows the loop is timed on (equal, or the script stops).

  python scripts/bench_denoise_sweep.py [--rounds 5] [--inner 20] [--out profiles/r15_denoise_sweep.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_denoise_sweep.py --trace-runs 20      # the kernels of add_run, traced
  python scripts/bench_denoise_sweep.py --kernel-stats DIR [--out FILE]                                 # ... summed per add_run (appended)
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

H, W, FRAMES = 260, 346, 300
SEED = 5
HOST_LOOP_ROWS = 200000
HOST_K, HOST_TAU_INDEX = 2, 32


def workload(rate, dev):
    """(rows on the device, counts, n_signal, seconds of the emulator run that made them -- the second of two identical runs)."""
    import torch
    from v2e_amd import EventEmulator
    from v2e_amd.synthetic import moving_dot
    frames, times = moving_dot(W, H, arg_list=["--cycles", "1"], device=dev).frames_block(0, FRAMES)
    times = [float(t) for t in times]
    sec = None
    for _ in range(2):
        emu = EventEmulator(rng_mode="philox", seed=SEED, device=dev)
        emu.set_dvs_params("noisy")
        emu.shot_noise_rate_hz = rate
        emu.generate_events_batch(frames[:1], times[:1])  # the first frame only initialises the state
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, counts = emu.generate_events_batch(frames[1:], times[1:], return_device=True)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        rows, counts, n_signal = rows.clone(), np.array(counts), np.array(emu.last_n_signal)
        emu.cleanup()
    return rows, counts, n_signal, sec


def host_loop(rows, k, tau):
    """The definition as a user would write it on the host for ONE (k, tau): a timestamp map and a loop over the rows.  Returns the
    keep mask."""
    last = np.full((H + 2, W + 2), -np.inf)  # (a border of -inf: a neighbour outside the sensor never supports)
    keep = np.zeros(len(rows), dtype=bool)
    t = rows[:, 0].astype(np.float64)
    xs = rows[:, 1].astype(np.int64) + 1
    ys = rows[:, 2].astype(np.int64) + 1
    for i in range(len(rows)):
        x, y = xs[i], ys[i]
        win = last[y - 1:y + 2, x - 1:x + 2]
        keep[i] = np.count_nonzero(t[i] - win <= tau) - (1 if t[i] - win[1, 1] <= tau else 0) >= k
        last[y, x] = t[i]
    return keep


def kernel_stats(d, say):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        sys.exit("no kernel_stats.csv under %s" % d)
    ours = [r for r in rows if "k_denoise" in r["Name"]]
    calls = max(int(r["Calls"]) for r in ours if "k_denoise_keys" in r["Name"])
    groups = {"torch.sort (rocprim block sort and merge passes, index fill)": [], "torch bookkeeping (zeroed counters, n_bad +=)": []}
    other = []
    for r in rows:
        name = r["Name"]
        if "k_denoise" in name:
            groups.setdefault(re.search(r"k_denoise_\w+(<\w+>)?", name).group(0), []).append(r)
        elif "rocprim" in name or "fill_reverse_indices" in name or "radix" in name:
            groups["torch.sort (rocprim block sort and merge passes, index fill)"].append(r)
        elif "CUDAFunctor_add<long>" in name or "FillFunctor<long>" in name:
            groups["torch bookkeeping (zeroed counters, n_bad +=)"].append(r)
        else:
            other.append(r)
    say("")
    say("rocprofv3 --kernel-trace --stats of %d add_run calls (a run of its own), kernel time per add_run:" % calls)
    say("%-66s %8s %12s" % ("kernel", "calls", "us / add_run"))
    per = {}
    for name, rs in groups.items():
        n = sum(int(r["Calls"]) for r in rs)
        tot = sum(float(r["TotalDurationNs"]) for r in rs)
        per[name] = tot / calls / 1e3
        say("%-66s %8d %12.1f" % (name[:66], n, per[name]))
    total = sum(per.values())
    sort = per["torch.sort (rocprim block sort and merge passes, index fill)"]
    say("sum: %.1f us, of which the sort %.1f us (%.0f %%) and the kernels of denoise.hip %.1f us"
        % (total, sort, 100.0 * sort / total, sum(v for k, v in per.items() if k.startswith("k_denoise"))))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_denoise_sweep.txt"))
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
        sys.exit("bench_denoise_sweep.py needs a GPU")
    from v2e_amd import DenoiseSweep, _capi
    dev = "cuda:0"
    taus = np.geomspace(1e-4, 1e-1, 64)
    rows, counts, n_signal, emu_sec = workload(args.rate, dev)
    n = int(rows.shape[0])

    def sweep():
        return DenoiseSweep(H, W, taus, device=dev)

    def run(ds, times=1):
        for _ in range(times):
            ds.add_run(rows, counts, 0, n_signal=n_signal)

    if args.trace_runs:
        run(sweep(), args.trace_runs)
        torch.cuda.synchronize()
        return

    ds = sweep()
    run(ds)
    r = ds.result()
    say("denoise sweep: STCF k = 1 .. 8 x %d taus %.0f us .. %.0f ms on the rows of %d frames %dx%d of moving_dot (dt 100 us), noisy preset "
        "with shot_noise_rate_hz %g, seed %d" % (len(taus), taus[0] * 1e6, taus[-1] * 1e3, FRAMES, W, H, args.rate, SEED))
    say("device: %s" % torch.cuda.get_device_name(0))
    say("rows %d: signal %d, noise %d (%.1f %%), bad %d; the emulator run that made them: %.2f ms"
        % (n, r.n_signal, r.n_noise, 100.0 * r.n_noise / max(n, 1), r.n_bad, emu_sec * 1e3))
    say("(the preset's 30 Hz cut-off leaves little of a dot that moves every 100 us: the rows are mostly shot noise)")
    k, tau, tpr, fpr = r.best()
    say("best tpr - fpr: k = %d, tau = %.3g s, tpr %.4f, fpr %.4f" % (k, tau, tpr, fpr))

    # the host loop for one (k, tau), on at most HOST_LOOP_ROWS rows, and the device's count for the same rows
    m = min(n, HOST_LOOP_ROWS)
    host_rows = rows[:m].cpu().numpy()
    t0 = time.perf_counter()
    keep = host_loop(host_rows, HOST_K, taus[HOST_TAU_INDEX])
    host_sec = time.perf_counter() - t0
    ds = sweep()
    out = ds.add_run(rows[:m], keep=(HOST_K, taus[HOST_TAU_INDEX]))
    passed = int(ds.result().passed[HOST_K - 1, :, HOST_TAU_INDEX].sum())
    if passed != int(keep.sum()) or not np.array_equal(out["mask"].cpu().numpy(), keep):
        say("MISMATCH between the host loop (%d rows pass) and the device (%d)" % (int(keep.sum()), passed))
        sys.exit(1)
    say("host loop, one (k, tau) = (%d, %.3g s): %.2f s on %d rows (%d pass, as on the device), %.2f s scaled to %d rows; all %d (k, tau): %.0f s"
        % (HOST_K, taus[HOST_TAU_INDEX], host_sec, m, passed, host_sec * n / m, n, 8 * len(taus), host_sec * n / m * 8 * len(taus)))

    lib = _capi.lib()
    import ctypes as C

    def sort_only():
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        _capi.check(lib.v2e_denoise_keys(C.c_void_p(rows.data_ptr()), n, H, W, C.c_void_p(keys.data_ptr()), None,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "v2e_denoise_keys")
        return torch.sort(keys)[0]

    legs = {"add_run": lambda ds=sweep(): run(ds), "keys + torch.sort alone": sort_only}
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
    say("per call, host clock from idle device to device idle; %d rounds alternating, %d consecutive calls each" % (args.rounds, args.inner))
    say("%-44s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"))
    med = {}
    for name, v in t.items():
        v = np.sort(np.array(v))
        med[name] = float(np.median(v))
        say("%-44s %10.3f %10.3f %10.3f" % (name, med[name], v[0], v[-1]))
    names = list(legs)
    say("")
    say("sort's share of add_run, host clock: %.0f %%" % (100.0 * med[names[1]] / med[names[0]]))
    say("rows per second: %.3g; add_run / emulator run: %.2f; host loop for all (k, tau) / add_run: %.3g"
        % (n / (med[names[0]] * 1e-3), med[names[0]] * 1e-3 / emu_sec, host_sec * n / m * 8 * len(taus) / (med[names[0]] * 1e-3)))

    # the same rows several times over, each copy later in time than the one before: a run long enough that launches do not dominate, and
    # the scratch of one pass measured (torch's allocator: peak over the call minus what was allocated before it)
    reps = args.long_copies
    span = float(rows[:, 0].max().item()) + 1e-4
    big = rows.repeat(reps, 1)
    big[:, 0] += torch.arange(reps, device=dev, dtype=torch.float32).repeat_interleave(n) * span
    nb = int(big.shape[0])
    say("")
    say("long run: the rows %d times over, %d rows in one pass (labels: all signal), %d rounds of %d calls" % (reps, nb, 3, 3))
    ds = sweep()
    ds.add_run(big)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ds.add_run(big)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    v = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            ds.add_run(big)
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) / 3 * 1e3)
    say("add_run: median %.3f ms (min %.3f, max %.3f), %.3g rows/s; peak scratch %.1f bytes per row"
        % (float(np.median(v)), min(v), max(v), nb / (float(np.median(v)) * 1e-3), peak / nb))
    v = []
    for _ in range(3):
        keys = torch.empty((nb,), dtype=torch.int64, device=dev)
        _capi.check(lib.v2e_denoise_keys(C.c_void_p(big.data_ptr()), nb, H, W, C.c_void_p(keys.data_ptr()), None,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "v2e_denoise_keys")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.sort(keys)
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    say("torch.sort of its keys alone: median %.3f ms" % float(np.median(v)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
