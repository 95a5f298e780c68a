#!/usr/bin/env python
"""EventFileReader on files of a few million events: the decode kernels alone, read_events end to end, the host baseline, and
what the upload of the same bytes costs.

Files (made here, in --dir): the rows of scripts/bench_denoise_sweep.py's emulator run (300 frames of moving_dot at 346 x 260,
noisy preset), `--copies` times over with later and later time stamps, as an AEDAT-2.0 file (DeviceAEDat2Output's bytes) and as
a text file (DeviceTextOutput's lines); and an RPG-style text file, `%.9f x y p` lines with seeded stamps.

  (a) decode alone   the bytes already on the device as one chunk, v2e_events_unpack_aedat2 / v2e_events_parse_text between two
                     device events; the first calls are warm-up, median of --rounds
  (b) end to end     read_events(path) from the page cache: file read, pinned upload, decode, concatenation; host clock behind a
                     device synchronise, median of --rounds
  (c) host           np.frombuffer + bit operations (tests/event_reader_ref.py decode_aedat2) on the whole AEDAT file; the Python
                     line loop (decode_text) and np.loadtxt on the first --host-lines lines of the text files, scaled to the file
  upload             the same bytes from pinned memory to the device, between two device events

  python scripts/bench_event_reader.py [--copies 32] [--rounds 5] [--out profiles/r19_event_reader.txt]
  rocprofv3 --kernel-trace --stats ... -- python scripts/bench_event_reader.py --trace-runs 5      # the kernels one by one
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_denoise_sweep import H, W, workload  # noqa: E402


def device_ms(fn, rounds, warm=2):
    import torch
    out = []
    for k in range(warm + rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            out.append(a.elapsed_time(b))
    return np.array(out)


def host_ms(fn, rounds, warm=1):
    import torch
    out = []
    for k in range(warm + rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=32)
    ap.add_argument("--rpg-lines", type=int, default=4_000_000)
    ap.add_argument("--host-lines", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-runs", type=int, default=0, help="only decode each file this often (for rocprofv3) and exit")
    ap.add_argument("--dir", default=None, help="where the files are made (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_event_reader.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_event_reader.py needs a GPU")
    from v2e_amd import _capi, read_events
    from v2e_amd._capi import check, ptr, stream_ptr
    from v2e_amd.readers import AEDAT2_LAYOUT
    from v2e_amd.sinks import DeviceAEDat2Output, DeviceTextOutput
    from event_reader_ref import aedat2_header_end, decode_aedat2, decode_text
    lib = _capi.lib()
    dev = torch.device("cuda:0")
    tmp = args.dir or tempfile.mkdtemp(prefix="v2e_reader_bench_")

    rows, counts, n_signal, _ = workload(50.0, "cuda:0")
    n1 = int(rows.shape[0])
    span = float(rows[:, 0].max().item()) + 1e-4
    big = rows.repeat(args.copies, 1)
    big[:, 0] += torch.arange(args.copies, device=dev, dtype=torch.float32).repeat_interleave(n1) * span
    n = int(big.shape[0])
    paths = {"aedat2": os.path.join(tmp, "run.aedat"), "text": os.path.join(tmp, "run.txt"), "rpg": os.path.join(tmp, "rpg.txt")}
    a2, tx = DeviceAEDat2Output(paths["aedat2"], W, H), DeviceTextOutput(paths["text"])
    for k in range(args.copies):  # (one run at a time, as the emulator's sinks get them)
        a2.appendEvents(big[k * n1:(k + 1) * n1])
        tx.appendEvents(big[k * n1:(k + 1) * n1])
    a2.close()
    tx.close()
    rng = np.random.default_rng(19)
    t = np.sort(rng.uniform(0, 600.0, args.rpg_lines))
    x, y, p = rng.integers(0, 240, args.rpg_lines), rng.integers(0, 180, args.rpg_lines), rng.integers(0, 2, args.rpg_lines)
    with open(paths["rpg"], "w") as f:
        for lo in range(0, args.rpg_lines, 500_000):
            f.write("".join("%.9f %d %d %d\n" % r for r in zip(t[lo:lo + 500_000], x[lo:lo + 500_000], y[lo:lo + 500_000], p[lo:lo + 500_000])))
    data = {k: open(v, "rb").read() for k, v in paths.items()}
    nrows = {"aedat2": (len(data["aedat2"]) - aedat2_header_end(data["aedat2"])) // 8, "text": n, "rpg": args.rpg_lines}

    # ---- the decode calls on bytes that are already on the device, one chunk
    calls = {}
    keep = []
    for name, raw in data.items():
        payload = raw[aedat2_header_end(raw):] if name == "aedat2" else raw
        nb = len(payload)
        dbytes = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(dev)
        pinned = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).pin_memory()
        cnt = torch.zeros(8, dtype=torch.int64, device=dev)
        if name == "aedat2":
            nrec = nb // 8
            out = torch.empty((nrec, 4), dtype=torch.float32, device=dev)
            t_us = torch.empty(nrec, dtype=torch.int64, device=dev)
            scratch = torch.empty(int(lib.v2e_events_unpack_aedat2_scratch_bytes(nrec)), dtype=torch.uint8, device=dev)
            xs, ys, ps, fx, fy = AEDAT2_LAYOUT[(W, H)]

            def call(dbytes=dbytes, nrec=nrec, out=out, t_us=t_us, cnt=cnt, scratch=scratch):
                check(lib.v2e_events_unpack_aedat2(ptr(dbytes), nrec, W, H, xs, ys, ps, fx, fy, 0, ptr(out), None, ptr(t_us), ptr(cnt),
                                                   ptr(scratch), stream_ptr(dev)), "v2e_events_unpack_aedat2")
        else:
            cap = nrows[name] + 64
            out = torch.empty((cap, 4), dtype=torch.float32, device=dev)
            fl = torch.empty((4096, 2), dtype=torch.int64, device=dev)
            scratch = torch.empty(int(lib.v2e_events_parse_text_scratch_bytes(nb, cap)), dtype=torch.uint8, device=dev)

            def call(dbytes=dbytes, nb=nb, out=out, cap=cap, cnt=cnt, fl=fl, scratch=scratch):
                check(lib.v2e_events_parse_text(ptr(dbytes), nb, 0, ptr(out), None, cap, ptr(cnt), ptr(fl), 4096, ptr(scratch),
                                                stream_ptr(dev)), "v2e_events_parse_text")
        calls[name] = (call, nb, dbytes, pinned)
        keep.append((out, scratch, cnt))

    if args.trace_runs:
        for name, (call, _, _, _) in calls.items():
            for _ in range(args.trace_runs):
                call()
        torch.cuda.synchronize()
        return

    say("event file readers: AEDAT-2.0 and text files decoded into device rows (v2e_amd/readers.py, v2e_amd/csrc/readers.hip)")
    say("device: %s" % torch.cuda.get_device_name(0))
    say("files: the rows of 300 frames %dx%d of moving_dot (noisy preset, shot noise 50 Hz), %d rows, %d times over = %d rows, written by "
        "DeviceAEDat2Output (%d bytes) and DeviceTextOutput (%d bytes); an RPG-style text file of %d lines '%%.9f x y p' (%d bytes)"
        % (W, H, n1, args.copies, n, len(data["aedat2"]), len(data["text"]), args.rpg_lines, len(data["rpg"])))
    say("")
    say("%-8s %12s %10s | %-28s | %-28s | %-28s | %-22s" % ("file", "bytes", "rows", "(a) decode alone ms  GB/s", "upload alone ms  GB/s",
                                                          "(b) read_events ms  GB/s", "(c) host s  (x of (b))"))
    for name in ("aedat2", "text", "rpg"):
        call, nb, dbytes, pinned = calls[name]
        dec = device_ms(call, args.rounds)
        up = device_ms(lambda: dbytes.copy_(pinned, non_blocking=True), args.rounds)
        kw = dict(width=W, height=H)
        got = read_events(paths[name], **kw)[0]
        assert int(got.shape[0]) == nrows[name], (name, got.shape, nrows[name])
        del got
        e2e = host_ms(lambda: read_events(paths[name], **kw), args.rounds)
        # the host baseline, and the device's rows against it on the part it covers
        if name == "aedat2":
            payload = data[name][aedat2_header_end(data[name]):]
            t0 = time.perf_counter()
            ref = decode_aedat2(payload, W, H)[0]
            host_s, note = time.perf_counter() - t0, "np.frombuffer + bit operations, the whole file"
            same = np.array_equal(read_events(paths[name], **kw)[0].cpu().numpy().view(np.uint32), ref.view(np.uint32))
            extra = ""
        else:
            head = b"\n".join(data[name].split(b"\n", args.host_lines + 16)[:args.host_lines + 16]) + b"\n"
            t0 = time.perf_counter()
            ref = decode_text(head)[0]
            part = time.perf_counter() - t0
            host_s = part * len(data[name]) / len(head)
            t0 = time.perf_counter()
            np.loadtxt(head.decode().splitlines(), dtype=np.float64, comments="#")
            lt = (time.perf_counter() - t0) * len(data[name]) / len(head)
            note = "the Python line loop on the first %d bytes, scaled to the file" % len(head)
            extra = "; np.loadtxt (float64, no checks) likewise: %.1f s" % lt
            same = np.array_equal(read_events(paths[name], **kw)[0][:len(ref)].cpu().numpy().view(np.uint32), ref.view(np.uint32))
        if not same:
            say("MISMATCH between the host baseline and the device on %s" % name)
            sys.exit(1)
        md, mu, me = float(np.median(dec)), float(np.median(up)), float(np.median(e2e))
        say("%-8s %12d %10d | %8.3f (%.3f-%.3f) %6.1f | %8.3f (%.3f-%.3f) %6.1f | %8.1f (%.1f-%.1f) %6.2f | %8.2f  (%.0fx)"
            % (name, nb, nrows[name], md, dec.min(), dec.max(), nb / md / 1e6, mu, up.min(), up.max(), nb / mu / 1e6, me, e2e.min(),
               e2e.max(), nb / me / 1e6, host_s, host_s * 1e3 / me))
        say("         host baseline: %s%s; rows equal to the device's" % (note, extra))
    say("")
    say("(a) and the upload: device events, 2 warm-up calls, median (min-max) of %d; (b): host clock behind a synchronise, files in the "
        "page cache, 1 warm-up, median (min-max) of %d; GB/s = the file's bytes over the time" % (args.rounds, args.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
