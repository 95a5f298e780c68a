"""Event-file sinks on the device-resident path: the headline clip (346x260, 300 frames per run, Philox, the pipelined loop of
bench.py) with no sink, with AEDAT-2.0 and with text, the writers pointed at os.devnull (packing, formatting, PCIe and host work;
no disk); and the per-frame drop-in's frames/s with dvs_text, with the device formatter and with the Python per-row formatting it
replaced (restated below as the "before" path).

    python scripts/sink_rates.py [--steps 20] [--repeats 5]
    python scripts/sink_rates.py --kernel-stats DIR     # the formatter kernels per event, from a rocprofv3 --stats run of
                                                        # `python scripts/sink_rates.py --profile-text` (output in DIR)
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import DEFAULT_KW, DT, FRAMES_PER_STEP, H, W, gen_frames_device  # noqa: E402
from v2e_amd import EventEmulator  # noqa: E402
from v2e_amd.sinks import DeviceAEDat2Output, DeviceTextOutput  # noqa: E402


def make_emu(sink):
    emu = EventEmulator(device="cuda", seed=1, rng_mode="philox", output_width=W, output_height=H, **DEFAULT_KW)
    if sink == "aedat2":
        emu.dvs_aedat2 = DeviceAEDat2Output(os.devnull, output_width=W, output_height=H)
    elif sink == "text":
        emu.dvs_text = DeviceTextOutput(os.devnull)
    return emu


def run_loop(emu, frames, steps, first):
    """bench.py's loop (benchutil.run_steps): run s + 1 enqueued before run s's result() is read; returns (seconds, events)."""
    nclip = (int(frames.shape[0]) - 1) // FRAMES_PER_STEP
    F = FRAMES_PER_STEP

    def enqueue(s):
        lo = 1 + (s % nclip) * F
        return emu.generate_events_batch_async(frames[lo:lo + F], [(1 + s * F + i) * DT for i in range(F)], return_device=True,
                                               use_graph=0, pipelined=True, frames_resident=True)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, pend = 0, None
    for s in range(first, first + steps):
        nxt = enqueue(s)
        if pend is not None:
            n += int(pend.result()[1].sum())
        pend = nxt
    n += int(pend.result()[1].sum())
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def batch_rates(frames, steps, repeats):
    out = {}
    for sink in ("none", "aedat2", "text"):
        emu = make_emu(sink)
        emu.generate_events_batch(frames[:1], [0.0])
        run_loop(emu, frames, 3, 0)  # warm-up (buffers, pinned staging)
        rates, first = [], 3
        for _ in range(repeats):
            sec, n = run_loop(emu, frames, steps, first)
            first += steps
            rates.append(n / sec / 1e6)
        emu.cleanup()
        out[sink] = {"Mevents_per_s_median": round(statistics.median(rates), 1), "min": round(min(rates), 1),
                     "max": round(max(rates), 1), "events_per_run": n // steps, "repeats": repeats, "runs_per_repeat": steps}
    return out


def legacy_text_append(self, events, signnoise_label=None, n_signal=None):
    """DeviceTextOutput.appendEvents before the device formatter: integer columns on the GPU, one Python format per row."""
    from v2e_amd.sinks import pack_h5
    if events is None or len(events) == 0:
        return
    ev = events if torch.is_tensor(events) else torch.from_numpy(events.astype('float32', copy=False)).cuda()
    n = int(ev.shape[0])
    cols = pack_h5(ev).cpu().numpy()
    t = ev[:, 0].double().cpu().numpy()
    lines = '{} {} {} {}\n'
    self.file.write(''.join(lines.format(t[i], cols[i, 1], cols[i, 2], cols[i, 3]) for i in range(n)).encode())
    self.numEventsWritten += n


def frame_api_rates(frames, nframes, repeats):
    host = frames[:nframes + 1].cpu().numpy()
    out = {}
    for name in ("no_sink", "text_python_rows", "text_device"):
        res = []
        for _ in range(repeats):
            emu = make_emu("text" if name != "no_sink" else "none")
            if name == "text_python_rows":
                emu.dvs_text.appendEvents = legacy_text_append.__get__(emu.dvs_text)
            for i in range(11):
                emu.generate_events(host[i], i * DT)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for i in range(11, len(host)):
                e = emu.generate_events(host[i], i * DT)
                n += 0 if e is None else len(e)
            sec = time.perf_counter() - t0
            emu.cleanup()
            res.append(((len(host) - 11) / sec, n / (len(host) - 11)))
        fps = [r[0] for r in res]
        out[name] = {"frames_per_s_median": round(statistics.median(fps), 1), "min": round(min(fps), 1), "max": round(max(fps), 1),
                     "events_per_frame": round(res[0][1])}
    return out


def profile_text(frames):
    emu = make_emu("text")
    emu.generate_events_batch(frames[:1], [0.0])
    sec, n = run_loop(emu, frames, 6, 0)
    emu.cleanup()
    print(json.dumps({"profiled_runs": 6, "events": n}))


def kernel_stats(d):
    """Per-event time of the sink kernels from rocprofv3 --kernel-trace --stats output (kernel_stats.csv) under d."""
    import csv
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    out = {}
    for r in rows:
        name = r.get("Name", "")
        for k in ("k_text_len", "k_text_scan", "k_text_write", "k_pack_aedat2", "k_pack_h5"):
            if k in name:
                out[k] = {"calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"]), "avg_ns": float(r["AverageNs"]),
                          "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])}
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frame-api-frames", type=int, default=300)
    ap.add_argument("--profile-text", action="store_true")
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
        return
    frames = gen_frames_device(1 + 8 * FRAMES_PER_STEP, 7, "cuda")
    torch.cuda.synchronize()
    if a.profile_text:
        profile_text(frames)
        return
    res = {"clip": "%dx%d, %d frames per run, Philox, pipelined async loop" % (W, H, FRAMES_PER_STEP),
           "batch": batch_rates(frames, a.steps, a.repeats),
           "frame_api_dvs_text": frame_api_rates(frames, a.frame_api_frames, 3)}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
