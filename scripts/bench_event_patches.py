#!/usr/bin/env python
"""EventPatches.add_run on the rows of one emulator run, for r = 1, 2, 3 in both modes, beside the numpy reference on the host.

Workload: scripts/bench_denoise_sweep.py's -- the rows of 300 frames of moving_dot at 346 x 260 through one Philox-mode emulator
(noisy preset, shot_noise_rate_hz 50) -- and the same rows 32 times over, each copy later in time than the one before.

Everything runs in one process on one GPU.  Each timing starts with the device idle and ends behind a device synchronise (host
clock); a round times `--inner` consecutive add_run calls of every (r, mode), the configurations alternating; median, minimum and
maximum over `--rounds` rounds.  The device's features for r = 3 are compared first with the reference's on the same rows (equal, or
the script stops).

  python scripts/bench_event_patches.py [--rounds 5] [--inner 20] [--out profiles/r17_event_patches.txt]
  python scripts/bench_event_patches.py --alt-lib "row order=OTHER/libv2e_amd.so" [--alt-ablation "no write=..."]   # v2e_patches_features
        of other builds of the library against this one's, on the same sorted keys, alternating (results compared equal first,
        except an ablation's); appended to --out
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_event_patches.py --trace-runs 20 [--long]   # traced
  python scripts/bench_event_patches.py --kernel-stats DIR [--long] [--out FILE]                              # ... summed per add_run (appended)
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

from bench_denoise_sweep import FRAMES, H, W, workload  # noqa: E402

CONFIGS = [(r, mode) for r in (1, 2, 3) for mode in ("age", "linear")]
TAU = 0.01
COPY_RATE = 6.3e12  # bytes per second this chip reaches on a copy
SORT = "torch.sort (rocprim block sort and merge passes, index fill)"
BOOK = "torch bookkeeping (zeroed counters)"


def long_rows(rows, reps):
    import torch
    n = int(rows.shape[0])
    span = float(rows[:, 0].max().item()) + 1e-4
    big = rows.repeat(reps, 1)
    big[:, 0] += torch.arange(reps, device=rows.device, dtype=torch.float32).repeat_interleave(n) * span
    return big


def timed(fn, inner):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def table(say, t):
    say("%-44s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"))
    med = {}
    for name, v in t.items():
        v = np.sort(np.array(v))
        med[name] = float(np.median(v))
        say("%-44s %10.3f %10.3f %10.3f" % (name, med[name], v[0], v[-1]))
    return med


def kernel_stats(d, n_rows, say):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        sys.exit("no kernel_stats.csv under %s" % d)
    feats = [r for r in rows if "k_patches_features" in r["Name"]]
    calls = max(int(r["Calls"]) for r in feats)
    groups = {SORT: [], BOOK: []}
    other = []
    for r in rows:
        name = r["Name"]
        m = re.search(r"k_(patches|denoise)_\w+(<\w+>)?", name)
        if m:
            groups.setdefault(m.group(0), []).append(r)
        elif "rocprim" in name or "fill_reverse_indices" in name or "radix" in name:
            groups[SORT].append(r)
        elif "FillFunctor<long>" in name:
            groups[BOOK].append(r)
        else:
            other.append(r)
    say("")
    say("rocprofv3 --kernel-trace --stats of %d add_run calls per radius (mode linear; a run of its own) on %d rows, kernel time per add_run:"
        % (calls, n_rows))
    say("%-66s %8s %12s" % ("kernel", "calls", "us / add_run"))
    per = {}
    for name, rs in groups.items():
        n = sum(int(r["Calls"]) for r in rs)
        tot = sum(float(r["TotalDurationNs"]) for r in rs)
        shared = 1 if "k_patches_features" in name else 3  # every other kernel runs for all three radii
        per[name] = tot / (calls * shared) / 1e3
        say("%-66s %8d %12.1f" % (name[:66], n, per[name]))
    rest = sum(v for k, v in per.items() if k != SORT and "k_patches_features" not in k)
    for r in (1, 2, 3):
        name = "k_patches_features<%d>" % r
        if name not in per:
            continue
        nbytes = n_rows * 2 * (2 * r + 1) ** 2 * 4
        rate = nbytes / (per[name] * 1e-6)
        say("r = %d: sort %.1f us, features kernel %.1f us, the rest %.1f us, sum %.1f us; the features kernel writes %.4g bytes: %.3g B/s, "
            "%.1f %% of the copy rate (%.1f TB/s)" % (r, per[SORT], per[name], rest, per[SORT] + per[name] + rest, nbytes, rate,
                                                     100.0 * rate / COPY_RATE, COPY_RATE / 1e12))
    say("not part of add_run (the emulator runs and the frames of the workload): %d launches, %.1f us in all"
        % (sum(int(r["Calls"]) for r in other), sum(float(r["TotalDurationNs"]) for r in other) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rate", type=float, default=50.0, help="shot_noise_rate_hz of the emulator run")
    ap.add_argument("--long-copies", type=int, default=32, help="copies of the rows in the long run")
    ap.add_argument("--long", action="store_true", help="--trace-runs / --kernel-stats: the long run's rows")
    ap.add_argument("--trace-runs", type=int, default=0, help="only run add_run this often per radius (for rocprofv3) and exit")
    ap.add_argument("--kernel-stats", help="summarise the kernel_stats.csv of a rocprofv3 run under this directory, appended to --out")
    ap.add_argument("--alt-lib", action="append", default=[], metavar="NAME=PATH",
                    help="another build of the library whose v2e_patches_features is timed against this one's (outputs must be equal)")
    ap.add_argument("--alt-ablation", action="append", default=[], metavar="NAME=PATH",
                    help="the same for a build that leaves a part of the kernel out (outputs not compared)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_event_patches.txt"))
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
        sys.exit("bench_event_patches.py needs a GPU")
    from v2e_amd import EventPatches, _capi
    dev = "cuda:0"
    rows, counts, n_signal, emu_sec = workload(args.rate, dev)
    n = int(rows.shape[0])
    big = long_rows(rows, args.long_copies)
    nb = int(big.shape[0])

    if args.kernel_stats:
        kernel_stats(args.kernel_stats, nb if args.long else n, say)
        write("a")
        return

    def patches(r, mode):
        return EventPatches(H, W, radius=r, mode=mode, tau=TAU, device=dev)

    if args.trace_runs:
        for r in (1, 2, 3):
            ep = patches(r, "linear")
            for _ in range(args.trace_runs):
                ep.add_run(big if args.long else rows)
        torch.cuda.synchronize()
        return

    lib = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def prepared(ev):
        """(sorted keys, seg) of one pass over ev."""
        m = int(ev.shape[0])
        keys = torch.empty((m,), dtype=torch.int64, device=dev)
        seg = torch.empty((H * W + 1,), dtype=torch.int32, device=dev)
        _capi.check(lib.v2e_denoise_keys(C.c_void_p(ev.data_ptr()), m, H, W, C.c_void_p(keys.data_ptr()), None, stream), "v2e_denoise_keys")
        skeys = torch.sort(keys)[0]
        _capi.check(lib.v2e_denoise_segments(C.c_void_p(skeys.data_ptr()), m, H, W, C.c_void_p(seg.data_ptr()), None, stream), "segments")
        return skeys, seg

    if args.alt_lib or args.alt_ablation:
        builds = {"this build": (lib, True)}
        for spec, checked in [(s, True) for s in args.alt_lib] + [(s, False) for s in args.alt_ablation]:
            name, path = spec.split("=", 1)
            alt = C.CDLL(path)
            alt.v2e_patches_features.restype, alt.v2e_patches_features.argtypes = _capi.SIGNATURES["v2e_patches_features"]
            builds[name] = (alt, checked)
        say("")
        say("v2e_patches_features alone (both of its kernels; the keys sorted once, maps empty), this build (threads in sorted, pixel, "
            "order) against other builds of the library, all alternating, %d rounds; outputs compared equal first, except those of "
            "the builds marked (ablation), which leave a part of the kernel out" % args.rounds)
        last_t = torch.full((H, W), -float("inf"), dtype=torch.float32, device=dev)
        last_p = torch.zeros((H, W), dtype=torch.int8, device=dev)
        for ev, inner in ((rows, args.inner), (big, 3)):
            m = int(ev.shape[0])
            skeys, seg = prepared(ev)
            for r in (1, 3):
                P = 2 * r + 1
                outs = [torch.full((m, 2, P, P), float("nan"), device=dev) for _ in range(2)]
                valid = torch.empty((m,), dtype=torch.uint8, device=dev)

                def call(build, out):
                    rc = build.v2e_patches_features(C.c_void_p(ev.data_ptr()), m, H, W, C.c_void_p(skeys.data_ptr()),
                                                    C.c_void_p(seg.data_ptr()), C.c_void_p(last_t.data_ptr()),
                                                    C.c_void_p(last_p.data_ptr()), r, 1, TAU, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(valid.data_ptr()), stream)
                    if rc != 0:
                        sys.exit("v2e_patches_features failed: %d" % rc)
                call(lib, outs[0])
                legs = {}
                for name, (build, checked) in builds.items():
                    call(build, outs[1])
                    if checked and not torch.equal(outs[0], outs[1]):
                        say("MISMATCH between this build and %s at r = %d on %d rows" % (name, r, m))
                        write("a")
                        sys.exit(1)
                    legs[name if checked else name + " (ablation)"] = lambda build=build: call(build, outs[1])
                t = {name: [] for name in legs}
                for rnd in range(-1, args.rounds):
                    for name, fn in legs.items():
                        v = timed(fn, inner)
                        if rnd >= 0:
                            t[name].append(v)
                say("%d rows, r = %d, mode linear, %d consecutive calls per round" % (m, r, inner))
                table(say, t)
                del outs
        write("a")
        return

    say("event patches: (2r+1)^2 ages and polarities per row for r = 1, 2, 3, modes age and linear (tau %g s), on the rows of %d frames "
        "%dx%d of moving_dot (dt 100 us), noisy preset with shot_noise_rate_hz %g" % (TAU, FRAMES, W, H, args.rate))
    say("device: %s" % torch.cuda.get_device_name(0))
    say("rows %d (signal %d); the emulator run that made them: %.2f ms" % (n, int(n_signal.sum()), emu_sec * 1e3))

    # the numpy reference on the host, and the device's features for the same rows
    from patches_ref import patches_serial
    host_rows = rows.cpu().numpy()
    host_sec = {}
    for r, mode in ((3, "age"), (3, "linear"), (1, "linear")):
        t0 = time.perf_counter()
        ref = patches_serial(host_rows, H, W, r, mode, TAU)
        host_sec[r, mode] = time.perf_counter() - t0
        ep = patches(r, mode)
        out = ep.add_run(rows)
        if not (np.array_equal(out["features"].cpu().numpy(), ref[0]) and np.array_equal(ep.last_t.cpu().numpy(), ref[2])
                and np.array_equal(ep.last_p.cpu().numpy(), ref[3])):
            say("MISMATCH between the numpy reference and the device at r = %d, mode %s" % (r, mode))
            sys.exit(1)
        inside = (ref[0][:, 0] > 0) & (ref[0][:, 0] < 1) if mode == "linear" else np.isfinite(ref[0][:, 0])
        say("numpy reference (tests/patches_ref.py, the serial loop) r = %d, mode %s: %.2f s on %d rows, features and maps equal to the "
            "device's; %.1f %% of the entries %s" % (r, mode, host_sec[r, mode], n, 100.0 * inside.mean(),
                                                    "strictly between 0 and 1" if mode == "linear" else "finite"))
        del ref

    legs = {"add_run r = %d, mode %s" % c: (lambda ep=patches(*c): ep.add_run(rows)) for c in CONFIGS}
    t = {name: [] for name in legs}
    for rnd in range(-1, args.rounds):
        for name, fn in legs.items():
            v = timed(fn, args.inner)
            if rnd >= 0:
                t[name].append(v)
    say("")
    say("per call on %d rows, host clock from idle device to device idle; %d rounds alternating, %d consecutive calls each"
        % (n, args.rounds, args.inner))
    med = table(say, t)
    say("rows per second at r = 3, linear: %.3g; add_run / emulator run: %.2f; numpy reference / add_run: %.3g"
        % (n / (med["add_run r = 3, mode linear"] * 1e-3), med["add_run r = 3, mode linear"] * 1e-3 / emu_sec,
           host_sec[3, "linear"] / (med["add_run r = 3, mode linear"] * 1e-3)))

    say("")
    say("long run: the rows %d times over, %d rows in one pass, 3 rounds of 3 calls" % (args.long_copies, nb))
    t = {}
    peak = {}
    for c in CONFIGS:
        ep = patches(*c)
        ep.add_run(big)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ep.add_run(big)
        torch.cuda.synchronize()
        P = 2 * c[0] + 1
        peak[c] = (torch.cuda.max_memory_allocated() - base) / nb - 2 * P * P * 4
        t["add_run r = %d, mode %s" % c] = [timed(lambda: ep.add_run(big), 3) for _ in range(3)]
        del ep
        torch.cuda.empty_cache()
    med = table(say, t)
    say("rows per second at r = 3, linear: %.3g; peak scratch beside the features: %.1f bytes per row; numpy reference scaled to these "
        "rows: %.0f s" % (nb / (med["add_run r = 3, mode linear"] * 1e-3), peak[3, "linear"], host_sec[3, "linear"] * nb / n))
    skeys_keys = torch.empty((nb,), dtype=torch.int64, device=dev)
    _capi.check(lib.v2e_denoise_keys(C.c_void_p(big.data_ptr()), nb, H, W, C.c_void_p(skeys_keys.data_ptr()), None, stream), "v2e_denoise_keys")
    say("torch.sort of its keys alone: median %.3f ms" % float(np.median([timed(lambda: torch.sort(skeys_keys), 1) for _ in range(3)])))
    write("w")


if __name__ == "__main__":
    main()
