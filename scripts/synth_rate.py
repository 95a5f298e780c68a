"""Frame rates of the device-resident synthetic sources (v2e_amd/synthetic.py) at 346 x 260 with the classes' default arguments
(dt 100 us), for each of moving_dot, particles, gradients and barberpole:

  render      frames/s of frames_block alone (blocks of --block frames, one synchronise at the end)
  pipeline    frames/s of SyntheticToEvents.run (render + emulator, no frame on the host)
  per_frame   frames/s of next_frame() + EventEmulator.generate_events per frame: the drop-in way, the figure to beat

Every path is run once on a short clip first (code objects, allocations, the emulator's stream assignment), then timed with a host
clock around work that ends in a device synchronise.  The emulator parameters are those of BASELINE configs[0].

  python scripts/synth_rate.py [--seconds 0.4] [--block 256] [--out profiles/r12_synthetic.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=300, leak_rate_hz=0.01, shot_noise_rate_hz=0.001,
          refractory_period_s=0.0005)
W, H = 346, 260


def make(name, seconds):
    import v2e_amd
    cls = getattr(v2e_amd, name)
    args = ['--t_total', str(seconds)] if name == "moving_dot" else ['--total_time', str(seconds)]
    kw = dict(rng=np.random.RandomState(1)) if name == "particles" else {}
    return cls(W, H, arg_list=args, parent_args=argparse.Namespace(hdr=False), device="cuda", **kw)


def emulator():
    from v2e_amd import EventEmulator
    return EventEmulator(device="cuda", seed=42, rng_mode="philox", **KW)


def render(name, seconds, block):
    import torch
    src = make(name, seconds)
    n = src.total_frames()
    bufs = [torch.empty((block, H, W), dtype=torch.float32 if name == "particles" else torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b, f0 in enumerate(range(0, n, block)):
        m = min(block, n - f0)
        src.frames_block(f0, m, out=bufs[b & 1][:m])
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), n, 0


def pipeline(name, seconds, block):
    import torch
    from v2e_amd import SyntheticToEvents
    src, emu = make(name, seconds), emulator()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev, counts, n = SyntheticToEvents(src, emu, block_frames=block).run(on_events=lambda e, c, f: None, return_device=True)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), n, int(counts.sum())


def per_frame(name, seconds, block):
    import torch
    src, emu = make(name, seconds), emulator()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = events = 0
    while True:
        f, t = src.next_frame()
        if f is None:
            break
        ev = emu.generate_events(f, float(t))
        events += 0 if ev is None else len(ev)
        n += 1
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), n, events


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.4, help="clip length (dt is 100 us: 10 000 frames per second of clip)")
    ap.add_argument("--per_frame_seconds", type=float, default=0.2)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "synth_rate.py measures on the GPU: there is no CPU path"
    lines = ["synthetic sources at %d x %d, dt 100 us, blocks of %d frames; frames/s, best and median of %d runs (%s)"
             % (W, H, a.block, a.repeats, torch.cuda.get_device_name(0)),
             "%-12s %-10s %8s %10s %12s %12s" % ("source", "path", "frames", "events", "best", "median")]
    for name in ("moving_dot", "particles", "gradients", "barberpole"):
        for path, fn, secs in (("render", render, a.seconds), ("pipeline", pipeline, a.seconds), ("per_frame", per_frame, a.per_frame_seconds)):
            fn(name, 0.03, a.block)  # warm-up: every kernel, buffer size class and stream of the path
            rates = []
            for _ in range(a.repeats):
                r, n, events = fn(name, secs, a.block)
                rates.append(r)
            lines.append("%-12s %-10s %8d %10d %12.0f %12.0f" % (name, path, n, events, max(rates), float(np.median(rates))))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
