#!/usr/bin/env python
"""EventStats.add_run on the rows of one emulator run, beside two baselines: (a) the numpy reference on the host
(tests/event_stats_ref.py, the row loop and the vectorised form) and (b) the same sums in plain torch on the same GPU (sort, gather,
diff, bucketize, bincount), and beside DenoiseSweep.add_run on the same rows.

Workload: scripts/bench_denoise_sweep.py's -- 300 frames of moving_dot at 346 x 260 (dt 100 us) through one Philox-mode emulator with
set_dvs_params("noisy") and shot_noise_rate_hz 50; labels from the run's counts and EventEmulator.last_n_signal; the default 61
interval edges, 50 time bins over the clip, the whole sensor as ROI.  Then the same rows 32 times over in one pass.

Everything runs in one process on one GPU.  Each timing starts with the device idle and ends behind a device synchronise (host
clock); a round times `--inner` consecutive calls of every leg, the legs alternating; median, minimum and maximum over `--rounds`
rounds.  The device's sums are compared first with the vectorised reference's and the torch formulation's (equal, or the script
stops).

  python scripts/bench_event_stats.py [--rounds 5] [--inner 20] [--out profiles/r22_event_stats.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_event_stats.py --trace-runs 20     # the kernels of add_run, traced
  python scripts/bench_event_stats.py --kernel-stats DIR [--out FILE]                                # ... summed per add_run (appended)
"""
import argparse
import csv
import ctypes as C
import glob
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_denoise_sweep import FRAMES, H, SEED, W, workload  # noqa: E402

BINS = 50
SORT = "torch.sort (rocprim block sort and merge passes, index fill)"
BOOK = "torch bookkeeping (zeroed counters, n_bad +=)"


class TorchStats(object):
    """Baseline (b): EventStats' sums as a user would write them in plain torch on the device, state carried the same way."""

    def __init__(self, edges, bounds, dev):
        import torch
        self.t = torch
        npx, E, K = H * W, len(edges), len(bounds) - 1
        self.edges, self.bounds = torch.from_numpy(edges).to(dev), torch.from_numpy(bounds).to(dev)
        self.count = torch.zeros(4 * npx + 1, dtype=torch.int64, device=dev)      # (the last cell of each: where bad rows go)
        self.isi_hist = torch.zeros(8 * (E + 1) + 1, dtype=torch.int64, device=dev)
        self.time_hist = torch.zeros(4 * K + 1, dtype=torch.int64, device=dev)
        self.n_first = torch.zeros(5, dtype=torch.int64, device=dev)
        self.n_backwards = torch.zeros(3, dtype=torch.int64, device=dev)
        self.n_before = torch.zeros((), dtype=torch.int64, device=dev)
        self.n_after = torch.zeros((), dtype=torch.int64, device=dev)
        self.min_isi = torch.full((9,), float("inf"), dtype=torch.float64, device=dev)
        self.t_first = torch.full((), float("inf"), device=dev)
        self.t_last = torch.full((), float("-inf"), device=dev)
        self.last_t = torch.full((npx + 2,), float("-inf"), device=dev)            # (+ the bad rows' slot and a slot to scatter to)
        self.last_on = torch.zeros(npx + 2, dtype=torch.int64, device=dev)

    def add_run(self, rows, labels):
        torch = self.t
        npx, E, K = H * W, len(self.edges), len(self.bounds) - 1
        t, x, y, p = rows.unbind(1)
        valid = torch.isfinite(t) & (x == x.floor()) & (y == y.floor()) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        pix = torch.where(valid, y.long() * W + x.long(), npx)
        skey = torch.sort((pix << 32) | torch.arange(len(t), device=rows.device))[0]
        order, sp = skey & 0xFFFFFFFF, skey >> 32
        ok = sp < npx
        ts, on, lab = t[order], (p[order] > 0).long(), labels[order].long()
        follows = torch.cat([torch.zeros(1, dtype=torch.bool, device=rows.device), sp[1:] == sp[:-1]])
        t_prev = torch.where(follows, ts.roll(1), self.last_t[sp])
        on_prev = torch.where(follows, on.roll(1), self.last_on[sp])
        c = 2 * lab + on
        self.count += torch.bincount(torch.where(ok, c * npx + sp, 4 * npx), minlength=4 * npx + 1)
        self.t_first = torch.minimum(self.t_first, torch.where(ok, ts, float("inf")).min())
        self.t_last = torch.maximum(self.t_last, torch.where(ok, ts, float("-inf")).max())
        t64 = ts.double()
        k = torch.bucketize(t64, self.bounds, right=True) - 1
        self.n_before += (ok & (k < 0)).sum()
        self.n_after += (ok & (k >= K)).sum()
        self.time_hist += torch.bincount(torch.where(ok & (k >= 0) & (k < K), c * K + k, 4 * K), minlength=4 * K + 1)
        none = t_prev == float("-inf")
        self.n_first += torch.bincount(torch.where(ok & none, c, 4), minlength=5)
        has = ok & ~none
        d = t64 - t_prev.double()
        cell = lab * 4 + 2 * on_prev + on
        self.isi_hist += torch.bincount(torch.where(has, cell * (E + 1) + torch.bucketize(d, self.edges, right=True), 8 * (E + 1)),
                                        minlength=8 * (E + 1) + 1)
        self.n_backwards += torch.bincount(torch.where(has & (d < 0), lab, 2), minlength=3)
        self.min_isi.scatter_reduce_(0, torch.where(has & (d >= 0), cell, 8), d, "amin")
        last = torch.cat([sp[1:] != sp[:-1], torch.ones(1, dtype=torch.bool, device=rows.device)]) & ok
        slot = torch.where(last, sp, npx + 1)
        self.last_t.scatter_(0, slot, ts)
        self.last_on.scatter_(0, slot, on)


def kernel_stats(d, say):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        sys.exit("no kernel_stats.csv under %s" % d)
    calls = max(int(r["Calls"]) for r in rows if "k_stats_rows" in r["Name"])
    groups, other = {SORT: [], BOOK: []}, []
    for r in rows:
        name = r["Name"]
        ours = re.search(r"k_(stats|denoise)_\w+", name)
        if ours:
            groups.setdefault(ours.group(0), []).append(r)
        elif "rocprim" in name or "fill_reverse_indices" in name or "radix" in name:
            groups[SORT].append(r)
        elif "CUDAFunctor_add<long>" in name or "FillFunctor<long>" in name:
            groups[BOOK].append(r)
        else:
            other.append(r)
    say("")
    say("rocprofv3 --kernel-trace --stats of %d add_run calls (a run of its own), kernel time per add_run:" % calls)
    say("%-66s %8s %12s" % ("kernel", "calls", "us / add_run"))
    per = {}
    for name, rs in groups.items():
        per[name] = sum(float(r["TotalDurationNs"]) for r in rs) / calls / 1e3
        say("%-66s %8d %12.1f" % (name[:66], sum(int(r["Calls"]) for r in rs), per[name]))
    total = sum(per.values())
    say("sum: %.1f us, of which the sort %.1f us (%.0f %%), the row index (k_denoise_keys, k_denoise_segments) %.1f us and the kernels of "
        "stats.hip %.1f us" % (total, per[SORT], 100.0 * per[SORT] / total, sum(v for k, v in per.items() if k.startswith("k_denoise")),
                               sum(v for k, v in per.items() if k.startswith("k_stats"))))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_event_stats.txt"))
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
        sys.exit("bench_event_stats.py needs a GPU")
    from denoise_ref import labels_from_counts
    from event_stats_ref import result_dict, same, stats_loop, stats_vectorised
    from v2e_amd import DenoiseSweep, EventStats, _capi
    dev = "cuda:0"
    rows, counts, n_signal, emu_sec = workload(args.rate, dev)
    n = int(rows.shape[0])
    span = float(rows[:, 0].max().item()) + 1e-4
    edges, bounds = np.geomspace(1e-5, 10.0, 61), np.linspace(0.0, span, BINS + 1)
    labels = torch.from_numpy(labels_from_counts(counts, n_signal)).to(dev)

    def stats():
        return EventStats(H, W, isi_edges=edges, time_bounds=bounds, device=dev)

    def run(es, times=1):
        for _ in range(times):
            es.add_run(rows, counts, 0, n_signal=n_signal)

    if args.trace_runs:
        run(stats(), args.trace_runs)
        torch.cuda.synchronize()
        return

    say("event stats: count map, %d interval edges %.0f us .. %.0f s, %d time bins on the rows of %d frames %dx%d of moving_dot (dt 100 us), "
        "noisy preset with shot_noise_rate_hz %g, seed %d" % (len(edges), edges[0] * 1e6, edges[-1], BINS, FRAMES, W, H, args.rate, SEED))
    say("device: %s" % torch.cuda.get_device_name(0))
    es = stats()
    run(es)
    res = es.result()
    say("rows %d: signal %d, noise %d, bad %d; pixels with a row %d, most rows on one pixel %d; the emulator run that made them: %.2f ms"
        % (n, res.count[1].sum(), res.count[0].sum(), res.n_bad, (res.count.sum(axis=(0, 1)) > 0).sum(), res.count.sum(axis=(0, 1)).max(),
           emu_sec * 1e3))

    # (a) the numpy reference on the host, and the device's sums against it
    host_rows, host_labels = rows.cpu().numpy(), labels.cpu().numpy()
    t0 = time.perf_counter()
    ref = stats_vectorised(host_rows, H, W, edges, bounds, None, host_labels)
    vec_sec = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref_loop = stats_loop(host_rows, H, W, edges, bounds, None, host_labels)
    loop_sec = time.perf_counter() - t0
    if not same(result_dict(res, es.last_t.cpu().numpy(), es.last_p.cpu().numpy()), ref) or not same(ref, ref_loop):
        say("MISMATCH between the device and the numpy reference")
        sys.exit(1)
    say("(a) numpy on the host, %d rows: the row loop %.2f s, the vectorised form %.1f ms; both equal to the device's sums" % (n, loop_sec, vec_sec * 1e3))

    # (b) plain torch on the device, and its sums against the device's
    ts = TorchStats(edges, bounds, dev)
    ts.add_run(rows, labels)
    E = len(edges)
    eq = (np.array_equal(ts.count[:-1].cpu().numpy().reshape(res.count.shape), res.count)
          and np.array_equal(ts.isi_hist[:-1].cpu().numpy().reshape(2, 4, E + 1), res.isi_hist)
          and np.array_equal(ts.time_hist[:-1].cpu().numpy().reshape(2, 2, BINS), res.time_hist)
          and np.array_equal(ts.n_first[:4].cpu().numpy().reshape(2, 2), res.n_first)
          and np.array_equal(ts.n_backwards[:2].cpu().numpy(), res.n_backwards)
          and np.array_equal(ts.min_isi[:8].cpu().numpy().reshape(2, 4), res.min_isi)
          and (int(ts.n_before), int(ts.n_after), float(ts.t_first), float(ts.t_last)) == (res.n_before, res.n_after, res.t_first, res.t_last)
          and np.array_equal(ts.last_t[:H * W].cpu().numpy().reshape(H, W), es.last_t.cpu().numpy()))
    if not eq:
        say("MISMATCH between the torch formulation and the device")
        sys.exit(1)
    say("(b) plain torch on the device (sort, gather, diff, bucketize, bincount, scatter): equal to the kernels' sums")

    lib = _capi.lib()

    def sort_only():
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        _capi.check(lib.v2e_denoise_keys(C.c_void_p(rows.data_ptr()), n, H, W, C.c_void_p(keys.data_ptr()), None,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "v2e_denoise_keys")
        return torch.sort(keys)[0]

    taus = np.geomspace(1e-4, 1e-1, 64)
    legs = {"EventStats.add_run": lambda es=stats(): run(es),
            "keys + torch.sort alone": sort_only,
            "(b) plain torch, the same sums": lambda ts=TorchStats(edges, bounds, dev): ts.add_run(rows, labels),
            "DenoiseSweep.add_run, 64 taus": lambda ds=DenoiseSweep(H, W, taus, device=dev): ds.add_run(rows, counts, 0, n_signal=n_signal)}
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
    say("%-52s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"))
    med = {}
    for name, v in t.items():
        v = np.sort(np.array(v))
        med[name] = float(np.median(v))
        say("%-52s %10.3f %10.3f %10.3f" % (name, med[name], v[0], v[-1]))
    names = list(legs)
    say("")
    say("sort's share of add_run, host clock: %.0f %%" % (100.0 * med[names[1]] / med[names[0]]))
    say("rows per second: %.3g; add_run / emulator run: %.2f; (a) vectorised numpy / add_run: %.0f; (b) plain torch / add_run: %.1f; "
        "add_run / DenoiseSweep.add_run: %.2f" % (n / (med[names[0]] * 1e-3), med[names[0]] * 1e-3 / emu_sec, vec_sec * 1e3 / med[names[0]],
                                                    med[names[2]] / med[names[0]], med[names[0]] / med[names[3]]))

    # the same rows several times over, each copy later in time than the one before (bench_denoise_sweep.py's long run)
    reps = args.long_copies
    big = rows.repeat(reps, 1)
    big[:, 0] += torch.arange(reps, device=dev, dtype=torch.float32).repeat_interleave(n) * span
    big_labels = labels.repeat(reps)
    nb = int(big.shape[0])
    big_bounds = np.linspace(0.0, span * reps, BINS + 1)
    say("")
    say("long run: the rows %d times over, %d rows in one pass (labels: a byte per row), %d rounds of %d calls" % (reps, nb, 3, 3))
    long_legs = {"EventStats.add_run": lambda es=EventStats(H, W, isi_edges=edges, time_bounds=big_bounds, device=dev):
                 es.add_run(big, labels=big_labels)}
    long_legs["(b) plain torch, the same sums"] = lambda ts=TorchStats(edges, big_bounds, dev): ts.add_run(big, big_labels)
    long_legs["DenoiseSweep.add_run, 64 taus"] = lambda ds=DenoiseSweep(H, W, taus, device=dev): ds.add_run(big, labels=big_labels)
    for name, fn in long_legs.items():
        fn()
        v = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) / 3 * 1e3)
        say("%-52s median %.3f ms (min %.3f, max %.3f), %.3g rows/s" % (name, float(np.median(v)), min(v), max(v), nb / (float(np.median(v)) * 1e-3)))
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

    # one hot pixel: every row of the long run on one pixel, one contended cell of every table
    hot = big.clone()
    hot[:, 1], hot[:, 2] = 100.0, 100.0
    say("")
    say("one hot pixel: the long run's rows all at (100, 100)")
    es = EventStats(H, W, isi_edges=edges, time_bounds=big_bounds, device=dev)
    es.add_run(hot, labels=big_labels)
    v = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        es.add_run(hot, labels=big_labels)
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    say("%-52s median %.3f ms (min %.3f, max %.3f)" % ("EventStats.add_run", float(np.median(v)), min(v), max(v)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
