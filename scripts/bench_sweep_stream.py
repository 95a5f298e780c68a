#!/usr/bin/env python
"""ThresholdSweep fed chunk by chunk (add_run ... result) against ThresholdSweep.run on the whole clip, and run on this commit
against run on another build of the library (the parent commit's).

Workload: that of profiles/r14_threshold_sweep.txt -- the reference's 95 thresholds (np.arange(1, 0.05, -0.01)) on 300 frames of
moving_dot at 346 x 260, rendered on the device, default model parameters (float32 state), counts inside a central ROI.

  python scripts/bench_sweep_stream.py [--parent-tree DIR] [--rounds 5] [--inner 20] [--repeats 3] [--out profiles/r18_sweep_stream.txt]

1. `run`, this tree against --parent-tree (a checkout of the parent commit with its library built; without it that leg is reported
   as not measured).  Two builds of one library do not share a process, so each leg is a child process that times `--rounds`
   rounds of `--inner` consecutive runs after a warm-up round; the two trees alternate, `--repeats` children each.  The spread
   of one tree's medians from child to child is what a difference between the trees is judged against.  Each child also reports
   v2e_thres_sweep_info of the four default instantiations.
2. In this process: the device-to-device copy rate of a buffer the size of the carried state (T x npx x 4 bytes), `run`, and
   add_run in chunks of 32, 64 and 300 frames followed by result(), alternating round by round.  A chunk reads the state once and
   writes it once, which is what a copy of that buffer does; so the expected time of a chunked sweep is run's plus one such copy
   per chunk, and that expectation is printed beside the measurement.
Every timing starts with the device idle and ends behind the read-back of the counts (host clock).  Counts are compared first.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FRAMES = 260, 346, 300
ROI = ((53, 292), (40, 219))
SEED = 5
CHUNKS = (32, 64, 300)
THRESHOLDS = np.arange(1, 0.05, -0.01)


def _workload(tree):
    sys.path.insert(0, tree)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sweep_stream.py needs a GPU")
    from v2e_amd import ThresholdSweep, _capi
    from v2e_amd.synthetic import moving_dot
    dev = "cuda:0"
    frames, times = moving_dot(W, H, arg_list=["--cycles", "1"], device=dev).frames_block(0, FRAMES)
    times = [float(t) for t in times]
    torch.cuda.synchronize()
    return torch, ThresholdSweep, _capi, dev, frames, times


def _timed(torch, fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def _info(_capi, entry):
    lib = _capi.lib()
    out = {}
    for f64 in (0, 1):
        for scalar in (0, 1):
            cols, vg, occ = C.c_int(0), C.c_int(0), C.c_int(0)
            _capi.check(getattr(lib, entry)(f64, scalar, 0, C.byref(cols), C.byref(vg), C.byref(occ)), entry)
            out["%d%d" % (f64, scalar)] = (cols.value, vg.value, occ.value)
    return out


def child(tree, rounds, inner):
    """One leg of part 1: prints a JSON line {ms: [per round], on, off, info}."""
    torch, ThresholdSweep, _capi, dev, frames, times = _workload(tree)
    sw = ThresholdSweep(H, W, THRESHOLDS, roi=ROI, seed=SEED, device=dev)
    res = sw.run(frames, times)
    ms = [_timed(torch, lambda: sw.run(frames, times), inner) for _ in range(rounds + 1)][1:]
    print(json.dumps(dict(ms=ms, on=res.on.tolist(), off=res.off.tolist(), info=_info(_capi, "v2e_thres_sweep_info"))), flush=True)


def stat(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_sweep_stream.txt"))
    args = ap.parse_args()
    if args.child:
        return child(os.path.abspath(args.child), args.rounds, args.inner)

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # ---- 1. run: this tree against the parent's, alternating child processes (before this process opens the GPU)
    trees = ([("parent commit", os.path.abspath(args.parent_tree))] if args.parent_tree else []) + [("this commit", ROOT)]
    legs = {name: [] for name, _ in trees}
    for _ in range(args.repeats):
        for name, tree in trees:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--rounds", str(args.rounds),
                                  "--inner", str(args.inner)], check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
            legs[name].append(json.loads(out.strip().splitlines()[-1]))

    torch, ThresholdSweep, _capi, dev, frames, times = _workload(ROOT)
    T, npx = len(THRESHOLDS), H * W
    say("streamed threshold sweep: %d thresholds %.2f .. %.2f, %d frames %dx%d of moving_dot (dt %.0f us), ROI x %r y %r, seed %d, default "
        "model parameters (sigma_thres 0.03, leak_rate_hz 0.1, no cutoff: float32 state, no refractory period)"
        % (T, THRESHOLDS[0], THRESHOLDS[-1], len(times), W, H, (times[1] - times[0]) * 1e6, ROI[0], ROI[1], SEED))
    say("device: %s" % torch.cuda.get_device_name(0))
    say("")
    say("1. ThresholdSweep.run, one child process per leg, the trees alternating; per call, host clock from idle device to counts on the "
        "host; %d rounds of %d consecutive calls per child after a warm-up round" % (args.rounds, args.inner))
    say("%-34s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"))
    meds = {}
    for name, _ in trees:
        meds[name] = []
        for k, leg in enumerate(legs[name]):
            m, lo, hi = stat(leg["ms"])
            meds[name].append(m)
            say("%-34s %10.3f %10.3f %10.3f" % ("%s, child %d" % (name, k + 1), m, lo, hi))
    for name, _ in trees:
        say("%s: median of the children's medians %.3f ms, their spread (max - min) %.3f ms"
            % (name, float(np.median(meds[name])), max(meds[name]) - min(meds[name])))
    this = legs["this commit"][0]
    if args.parent_tree:
        par = legs["parent commit"][0]
        same = all(leg["on"] == par["on"] and leg["off"] == par["off"] for name, _ in trees for leg in legs[name])
        say("counts of the two trees: %s" % ("equal" if same else "DIFFERENT"))
        d = float(np.median(meds["this commit"])) - float(np.median(meds["parent commit"]))
        spread = max(max(v) - min(v) for v in meds.values())
        say("this commit - parent commit: %+.3f ms (%+.2f %%); the larger child-to-child spread of one tree: %.3f ms -> %s"
            % (d, 100 * d / float(np.median(meds["parent commit"])), spread,
               "equal within the spread" if abs(d) <= spread else ("this commit is SLOWER" if d > 0 else "this commit is faster")))
        if not same:
            sys.exit(1)
    else:
        say("parent commit: not measured (no --parent-tree)")
    say("")
    say("registers and occupancy of the default instantiations (v2e_thres_sweep_info; cols_per_thread 0 -> 8):")
    names = {"00": "f64_state=0 scalar_thres=0", "01": "f64_state=0 scalar_thres=1", "10": "f64_state=1 scalar_thres=0",
             "11": "f64_state=1 scalar_thres=1"}
    for name, _ in trees:
        for k in sorted(names):
            cols, vg, occ = legs[name][0]["info"][k]
            say("%s: k_sweep %s cols_per_thread=%d: VGPRs %d, workgroups/CU %d" % (name, names[k], cols, vg, occ))
    for k, (cols, vg, occ) in sorted(_info(_capi, "v2e_thres_sweep_chunk_info").items()):
        say("this commit, the carrying instantiation (v2e_thres_sweep_chunk): k_sweep %s cols_per_thread=%d: VGPRs %d, workgroups/CU %d"
            % (names[k], cols, vg, occ))

    # ---- 2. chunked against run, in this process
    sw = ThresholdSweep(H, W, THRESHOLDS, roi=ROI, seed=SEED, device=dev)
    ref = sw.run(frames, times)
    if ref.on.tolist() != this["on"] or ref.off.tolist() != this["off"]:
        say("MISMATCH between this process and its child")
        sys.exit(1)

    def chunked(n):
        sw.reset()
        for a in range(0, len(times), n):
            sw.add_run(frames[a:a + n], times[a:a + n], a)
        return sw.result()

    for n in CHUNKS:
        r = chunked(n)
        if not (np.array_equal(r.on, ref.on) and np.array_equal(r.off, ref.off) and not r.rule_on.any() and sw.host_syncs == 1):
            say("MISMATCH add_run in chunks of %d" % n)
            sys.exit(1)
    say("")
    say("2. counts: add_run in chunks of %s + result() == run; ON %d .. %d, OFF %d .. %d; no read-back before result()"
        % (", ".join(str(n) for n in CHUNKS), ref.on.min(), ref.on.max(), ref.off.min(), ref.off.max()))

    state_bytes = T * npx * 4
    src = torch.empty((state_bytes // 4,), dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    t_copy = []
    for rnd in range(-1, args.rounds):
        ms = _timed(torch, lambda: dst.copy_(src), 200)
        if rnd >= 0:
            t_copy.append(ms)
    copy_ms = stat(t_copy)[0]
    say("the carried state: base [%d][%d] float32 = %.1f MB (and lp, %.2f MB); a device-to-device copy of that size, read + write as a "
        "chunk does: %.1f us median of %d rounds of 200 (%.2f TB/s counting both directions)"
        % (T, npx, state_bytes / 1e6, npx * 4 / 1e6, copy_ms * 1e3, args.rounds, 2 * state_bytes / (copy_ms * 1e-3) / 1e12))

    t_run, t_chunk = [], {n: [] for n in CHUNKS}
    for rnd in range(-1, args.rounds):
        ms = _timed(torch, lambda: sw.run(frames, times), args.inner)
        if rnd >= 0:
            t_run.append(ms)
        for n in CHUNKS:
            ms = _timed(torch, lambda: chunked(n), args.inner)
            if rnd >= 0:
                t_chunk[n].append(ms)
    say("per call, host clock from idle device to counts on the host; %d rounds alternating, %d consecutive calls each" % (args.rounds, args.inner))
    say("%-34s %10s %10s %10s %14s %12s" % ("", "median ms", "min ms", "max ms", "expected ms", "excess"))
    m_run, lo, hi = stat(t_run)
    say("%-34s %10.3f %10.3f %10.3f" % ("run (this commit, this process)", m_run, lo, hi))
    per_frame = m_run / (len(times) - 1)
    for n in CHUNKS:
        nch = -(-len(times) // n)
        m, lo, hi = stat(t_chunk[n])
        exp = m_run + nch * copy_ms
        say("%-34s %10.3f %10.3f %10.3f %14.3f %+11.3f   (%d chunks; %+.1f %% over run, expected %+.1f %%; excess per chunk %.1f us)"
            % ("add_run x %d frames + result" % n, m, lo, hi, exp, m - exp, nch, 100 * (m / m_run - 1), 100 * (exp / m_run - 1),
               (m - exp) / nch * 1e3))
    say("(expected = run + chunks x the copy above; run is %.2f us per frame, so a chunk's state traffic is %.1f frames' worth)"
        % (per_frame * 1e3, copy_ms / per_frame))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
