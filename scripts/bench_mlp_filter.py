#!/usr/bin/env python
"""MLPFilter.add_run (patches, MLP and mask in one kernel) on the rows of one emulator run, beside the unfused way to the same mask:
EventPatches.add_run -> a float32 nn.Sequential on the features -> a compare.

Workload: scripts/bench_event_patches.py's -- the rows of 300 frames of moving_dot at 346 x 260 through one Philox-mode emulator
(noisy preset, shot_noise_rate_hz 50) -- and the same rows 32 times over, each copy later in time than the one before.  r = 3,
hidden = 20, tau 0.01 s; the weights are seeded normals (scaled by 0.2), which cost what trained ones cost.

Everything runs in one process on one GPU.  Each timing starts with the device idle and ends behind a device synchronise (host
clock); a round times `--inner` consecutive calls of each way, the two alternating; median, minimum and maximum over `--rounds`
rounds.  The fused scores are compared first with the numpy definition's on the same rows (equal bit for bit, or the script stops).

  python scripts/bench_mlp_filter.py [--rounds 5] [--inner 20] [--out profiles/r26_mlp_filter.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_mlp_filter.py --trace-runs 20 [--long]   # traced
  python scripts/bench_mlp_filter.py --kernel-stats DIR [--long] [--out FILE]                                   # ... summed per add_run (appended)
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_denoise_sweep import FRAMES, H, W, workload  # noqa: E402
from bench_event_patches import long_rows, table, timed  # noqa: E402

R, HIDDEN, TAU, KEEP = 3, 20, 0.01, 0.0
K = 2 * (2 * R + 1) ** 2
SORT = "torch.sort (rocprim block sort and merge passes, index fill)"
R17 = {False: 48.7, True: 4198.0}  # k_patches_features<3> per add_run in profiles/r17_event_patches.txt, us


def network():
    rng = np.random.RandomState(26)
    return ((0.2 * rng.randn(HIDDEN, K)).astype(np.float32), (0.2 * rng.randn(HIDDEN)).astype(np.float32),
            (0.2 * rng.randn(1, HIDDEN)).astype(np.float32), (0.2 * rng.randn(1)).astype(np.float32))


def kernel_stats(d, n_rows, long, say):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        sys.exit("no kernel_stats.csv under %s" % d)
    calls = max(int(r["Calls"]) for r in rows if "k_mlp_scores" in r["Name"])
    groups, other = {SORT: []}, []
    for r in rows:
        name = r["Name"]
        m = re.search(r"k_(mlp|patches|denoise)_\w+(<\w+>)?", name)
        if m:
            groups.setdefault(m.group(0), []).append(r)
        elif "rocprim" in name or "fill_reverse_indices" in name or "radix" in name:
            groups[SORT].append(r)
        else:
            other.append(r)
    say("")
    say("rocprofv3 --kernel-trace --stats of %d MLPFilter.add_run calls (r = %d, hidden = %d, keep given; a run of its own, no counters) "
        "on %d rows, kernel time per add_run:" % (calls, R, HIDDEN, n_rows))
    say("%-66s %8s %12s" % ("kernel", "calls", "us / add_run"))
    per = {}
    for name, rs in groups.items():
        per[name] = sum(float(r["TotalDurationNs"]) for r in rs) / calls / 1e3
        say("%-66s %8d %12.1f" % (name[:66], sum(int(r["Calls"]) for r in rs), per[name]))
    fused = [v for k, v in per.items() if "k_mlp_scores" in k][0]
    rest = sum(v for k, v in per.items() if k != SORT and "k_mlp_scores" not in k)
    say("sort %.1f us, fused kernel %.1f us, the rest %.1f us, sum %.1f us; k_patches_features<3> on the same rows in "
        "profiles/r17_event_patches.txt: %.1f us (fused / features kernel: %.2f)"
        % (per[SORT], fused, rest, per[SORT] + fused + rest, R17[long], fused / R17[long]))
    say("every other kernel of the process (the emulator runs, the frames of the workload, torch fills): %d launches, %.1f us in all"
        % (sum(int(r["Calls"]) for r in other), sum(float(r["TotalDurationNs"]) for r in other) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rate", type=float, default=50.0, help="shot_noise_rate_hz of the emulator run")
    ap.add_argument("--long-copies", type=int, default=32, help="copies of the rows in the long run")
    ap.add_argument("--long", action="store_true", help="--trace-runs / --kernel-stats: the long run's rows")
    ap.add_argument("--trace-runs", type=int, default=0, help="only run add_run this often (for rocprofv3) and exit")
    ap.add_argument("--kernel-stats", help="summarise the kernel_stats.csv of a rocprofv3 run under this directory, appended to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_mlp_filter.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def write(mode):
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, mode) as f:
            f.write("\n".join(lines) + "\n")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mlp_filter.py needs a GPU")
    from v2e_amd import EventPatches, MLPFilter
    dev = "cuda:0"
    rows, counts, n_signal, emu_sec = workload(args.rate, dev)
    n = int(rows.shape[0])
    big = long_rows(rows, args.long_copies)
    nb = int(big.shape[0])

    if args.kernel_stats:
        kernel_stats(args.kernel_stats, nb if args.long else n, args.long, say)
        write("a")
        return

    net = network()

    def fused():
        return MLPFilter(H, W, *net, radius=R, tau=TAU, device=dev)

    if args.trace_runs:
        flt = fused()
        for _ in range(args.trace_runs):
            flt.add_run(big if args.long else rows, keep=KEEP)
        torch.cuda.synchronize()
        return

    nn = torch.nn
    module = nn.Sequential(nn.Linear(K, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, 1))
    with torch.no_grad():
        for layer, w, b in ((module[0], net[0], net[1]), (module[2], net[2], net[3])):
            layer.weight.copy_(torch.from_numpy(w))
            layer.bias.copy_(torch.from_numpy(b))
    module = module.to(dev)

    def unfused_call(ep, ev):
        """The same mask without MLPFilter: the features in device memory, torch's float32 GEMMs, a compare."""
        out = ep.add_run(ev)
        with torch.no_grad():
            score = module(out["features"].reshape(-1, K)).reshape(-1)
        return score, out["valid"] & (score >= KEEP)

    say("MLP filter: (2r+1)^2 x 2 linear time-surface features per row, r = %d (K = %d), one hidden layer of %d, tau %g s, keep >= %g, on "
        "the rows of %d frames %dx%d of moving_dot (dt 100 us), noisy preset with shot_noise_rate_hz %g"
        % (R, K, HIDDEN, TAU, KEEP, FRAMES, W, H, args.rate))
    say("device: %s" % torch.cuda.get_device_name(0))
    say("rows %d (signal %d); the emulator run that made them: %.2f ms" % (n, int(n_signal.sum()), emu_sec * 1e3))

    # the numpy definition on the host, and both device ways, on the same rows
    from mlp_filter_ref import bits, mlp_filter_serial
    t0 = time.perf_counter()
    ref = mlp_filter_serial(rows.cpu().numpy(), H, W, R, TAU, *net, keep=KEEP)
    host_sec = time.perf_counter() - t0
    flt = fused()
    out = flt.add_run(rows, keep=KEEP)
    got = out["scores"].view(torch.int32).cpu().numpy().view(np.uint32)
    if not (np.array_equal(got, bits(ref[0])) and np.array_equal(out["mask"].cpu().numpy(), ref[2])
            and np.array_equal(flt.last_t.cpu().numpy(), ref[3]) and np.array_equal(flt.last_p.cpu().numpy(), ref[4])):
        say("MISMATCH between the numpy definition and the device")
        sys.exit(1)
    score32, mask32 = unfused_call(EventPatches(H, W, radius=R, mode="linear", tau=TAU, device=dev), rows)
    diff = (score32.double() - out["scores"].double()).abs().max().item()
    say("numpy definition (tests/mlp_filter_ref.py): %.2f s on %d rows; the fused scores, mask (%d of %d rows kept) and maps are equal "
        "to it bit for bit" % (host_sec, n, int(ref[2].sum()), n))
    say("unfused float32 torch scores against the fused ones: largest difference %.3g, %d of %d scores differ in their bits, %d mask "
        "entries differ" % (diff, int((score32.view(torch.int32) != out["scores"].view(torch.int32)).sum()), n,
                            int((mask32 != out["mask"]).sum())))
    del ref, score32, mask32, out

    def both(ev, inner, rounds):
        flt, ep = fused(), EventPatches(H, W, radius=R, mode="linear", tau=TAU, device=dev)
        legs = {"MLPFilter.add_run (fused)": lambda: flt.add_run(ev, keep=KEEP),
                "EventPatches.add_run + nn.Sequential + compare": lambda: unfused_call(ep, ev)}
        t = {name: [] for name in legs}
        for rnd in range(-1, rounds):
            for name, fn in legs.items():
                v = timed(fn, inner)
                if rnd >= 0:
                    t[name].append(v)
        med = table(say, t)
        a, b = med["MLPFilter.add_run (fused)"], med["EventPatches.add_run + nn.Sequential + compare"]
        say("unfused / fused: %.2f; fused rows per second: %.3g" % (b / a, int(ev.shape[0]) / (a * 1e-3)))
        peak = {}
        for name, fn in legs.items():
            fn()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        return peak

    say("")
    say("per call on %d rows, host clock from idle device to device idle; %d rounds alternating, %d consecutive calls each"
        % (n, args.rounds, args.inner))
    both(rows, args.inner, args.rounds)
    say("")
    say("long run: the rows %d times over, %d rows in one pass, 3 rounds alternating, 3 consecutive calls each" % (args.long_copies, nb))
    peak = both(big, 3, 3)
    say("peak device memory of one call on these rows above what was allocated before it (torch.cuda.max_memory_allocated):")
    for name, v in peak.items():
        say("%-52s %14d bytes, %6.1f per row" % (name, v, v / nb))
    say("derivable: the sort's 48 bytes per row in both; fused 4 (score) + 1 (valid) + 1 (mask); unfused %d (features) + 1 (valid) + "
        "%d (hidden activations, float32) + 4 (score) + masks" % (K * 4, HIDDEN * 4))
    write("w")


if __name__ == "__main__":
    main()
