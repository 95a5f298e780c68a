"""Frames per second of VideoToEvents(auto_upsample=True) against a fixed upsampling factor.

  python scripts/auto_upsample_rate.py [--out FILE]

1. The samples-per-call curve: interpolated frames/s of ONE ragged interpolation call (k_prep_tab, interpolation UNet,
   k_fuse_tab) against the samples it carries, at the 320x256 network size (time points of U = 10 over 8 pairs).
2. A 346x260 uniform-random clip (seed 2, as bench.py's end-to-end leg) through VideoToEvents: the flow head of the seeded weights
   scaled so that the per-batch factors land near --target-speed (8; the flow is linear in the head: conv3 + leaky ReLU is
   positively homogeneous), auto_upsample with samples-per-call caps (0 = one call per batch, no packing) against fixed U = the auto run's rounded mean
   factor and U = 10; SloMo stage (upsample) and whole run (events included), host read-backs per clip.
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def engine(device, head, conv_math=None):
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import portable_unet_state_dict
    sd_f, sd_i = portable_unet_state_dict(2, 4, 101), portable_unet_state_dict(12, 5, 102)
    sd_f["conv3.weight"] = sd_f["conv3.weight"] * np.float32(head)
    sd_f["conv3.bias"] = sd_f["conv3.bias"] * np.float32(head)
    return SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()}, {k: torch.from_numpy(v) for k, v in sd_i.items()},
                       device, conv_math=conv_math)


def samples_curve(eng, device, sizes, reps):
    from v2e_amd.slomo import time_coefficients
    g = torch.Generator(device=device)
    g.manual_seed(7)
    P, U, h, w = 8, 10, 256, 320
    x = torch.rand((P + 1, 1, h, w), device=device, generator=g) - 0.428
    I0, I1 = x[:P].contiguous(), x[1:].contiguous()
    flow = eng.flow(I0, I1)
    coef = torch.from_numpy(time_coefficients([(k + 0.5) / U for k in range(U)])).to(device)
    out = {}
    for n in sizes:
        tab = torch.tensor([(s % P, (s // P) % U, s) for s in range(n)], dtype=torch.int32, device=device)
        eng.interpolate_table(I0, I1, flow, coef, tab, 0, n)  # warm-up (workspace)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.interpolate_table(I0, I1, flow, coef, tab, 0, n)
        torch.cuda.synchronize(device)
        out[n] = round(n * reps / (time.perf_counter() - t0), 1)
        print("samples/call %4d: %8.1f frames/s" % (n, out[n]), flush=True)
    return out


def clip_rate(eng, src, U, auto, cap, reps, device, run_too=True):
    from v2e_amd import EventEmulator
    from v2e_amd.pipeline import VideoToEvents
    import bench as B
    pipe = VideoToEvents(eng, None, U, batch_size=8, auto_upsample=auto)
    if cap is not None:
        pipe.samples_per_call = cap
    pipe.upsample(src)  # warm-up
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(reps):
        nfr = int(pipe.upsample(src).shape[0])
    torch.cuda.synchronize(device)
    r = {"frames": nfr, "slomo_frames_per_s": round(nfr * reps / (time.perf_counter() - t0), 1)}
    if auto:
        r.update(factors=pipe.upsampling_factors, host_syncs_per_clip=pipe.host_syncs, samples_per_call=pipe.samples_per_call)
    if run_too:
        n_fr, n_ev, t = 0, 0, 0.0
        for i in range(reps + 1):
            pipe.emu = EventEmulator(device=device, seed=2 + i, rng_mode="philox", **B.DEFAULT_KW)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            ev, counts, n = pipe.run(src, 1.0 / 30.0, return_device=True)
            torch.cuda.synchronize(device)
            if i:  # the first run is the warm-up
                t += time.perf_counter() - t0
                n_fr += n
                n_ev += int(counts.sum())
        r.update(run_frames_per_s=round(n_fr / t, 1), Mevents_per_s=round(n_ev / t / 1e6, 1))
    print(("auto cap %s" % cap if auto else "fixed U=%d" % U), r, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-src", type=int, default=97, help="source frames of the clip (96 pairs: two flow chunks)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="8,16,24,32,48,64,80,96,128,160,192,256", help="samples per call of the curve ('': no curve)")
    ap.add_argument("--target-speed", type=float, default=8.0, help="median per-batch flow speed the head is scaled to (factor ~ its ceil)")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(device)}
    eng = engine(device, 1.0)
    if a.sizes:
        res["samples_per_call_curve_320x256"] = samples_curve(eng, device, [int(v) for v in a.sizes.split(",")], a.reps)

    from v2e_amd.pipeline import VideoToEvents
    g = torch.Generator(device=device)
    g.manual_seed(2)
    src = torch.randint(0, 256, (a.n_src, 260, 346), dtype=torch.uint8, device=device, generator=g)
    x, _, _ = VideoToEvents(eng, None, None, auto_upsample=True)._normalised_input(src)
    speeds = [eng.max_speed(eng.flow(x[b0:min(b0 + 8, a.n_src - 1)], x[b0 + 1:min(b0 + 8, a.n_src - 1) + 1]))
              for b0 in range(0, a.n_src - 1, 8)]
    head = a.target_speed / float(np.median(speeds))
    res["flow_head_scale"] = round(head, 4)
    del eng
    eng = engine(device, head)
    caps = [0, 32, 64, 80, 128, 192, 256]
    auto = {str(c): clip_rate(eng, src, None, True, c, a.reps, device, run_too=(c in (0, 128))) for c in caps}
    res["auto"] = auto
    u_mean = int(round(float(np.mean(auto["128"]["factors"]))))
    res["fixed"] = {str(u): clip_rate(eng, src, u, False, None, a.reps, device) for u in sorted({max(2, u_mean), 10})}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
