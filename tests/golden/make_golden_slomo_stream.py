#!/usr/bin/env python
"""Golden vectors for the warp / blend / fusion kernels (k_prep, k_fuse and their _tab twins) at edge shapes, from the
reference's own backWarp and the slomo.py:404-433 sequence (make_golden_slomo.ref_interp) with overridden flow and
interpolation-network outputs.

  slomo_stream_edges.npz   per case (h, w, b, n_t) of slomo_stream_cases.EDGE_CASES: frames, ts, flow, intrp, channels 6-11 of
                           x12, Ft

The flow of a case is random in +-(max(h, w) + 3) px, and on planted pixels chosen so that the sampling position of one warp
lands exactly in one of the classes of slomo_stream_cases.classify (on an integer, on -1 / the last / the first outside
column or row, half a pixel across a border, in a corner with one neighbour inside, 3e4 px outside).  At t = 0.5 the blend is
Ft0 = (F10 - F01) / 4 = -Ft1 and at t = 0.25 Ft0 = (F10 - 3 F01) / 16 = -Ft1 / 3: two flows per pixel set Ft0 of both time rows,
exactly in float32.  The interpolation override is random in +-3; on planted samples its residual flows are target - Ft, with Ft
read from the reference's own x12, kept where float32 adds them back to the target exactly.  Seven pixels per sample carry the
visibility logits 0, +-20, +-90, +-110."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import ref_harness as rh  # noqa: E402
import slomo_stream_cases as sc  # noqa: E402
from make_golden_slomo import ref_interp  # noqa: E402
from v2e_amd.synth import int_gradient_frames  # noqa: E402

REPS = sc.MIN_PER_CLASS
FAR = 3.0e4


def recipes(h, w, rng):
    """name -> a function returning one target position (ix, iy); the first dozen are planted 8 times per warp direction in
    every case, the rest (an axis class beside an inner fractional coordinate of the other axis) while pixels are left"""
    q = lambda: float(rng.choice([0.25, 0.75]))
    fx = lambda: float(rng.integers(0, w - 1)) + q()   # strictly inside, both neighbours inside
    fy = lambda: float(rng.integers(0, h - 1)) + q()
    calls = [0]

    def far():   # (job_list asks for the two directions in turn: the sign changes with every second call)
        s = FAR if (calls[0] // 2) % 2 == 0 else -FAR
        calls[0] += 1
        return (s, fy()) if (calls[0] // 4) % 2 else (fx(), s)

    must = {
        "interior_integer": lambda: (float(rng.integers(0, w - 1)), float(rng.integers(0, h - 1))),
        "x_on_minus_1": lambda: (-1.0, fy()),
        "x_on_size": lambda: (float(w), fy()),
        "y_on_minus_1": lambda: (fx(), -1.0),
        "y_on_size": lambda: (fx(), float(h)),
        "half_across_left, y_on_last": lambda: (-0.5, h - 1.0),
        "x_on_last, half_across_top": lambda: (w - 1.0, -0.5),
        "half_across_right, half_across_bottom": lambda: (w - 0.5, h - 0.5),
        "corner_top_left": lambda: (-q(), -q()),
        "corner_top_right": lambda: (w - 1 + q(), -q()),
        "corner_bottom_left": lambda: (-q(), h - 1 + q()),
        "far": far,
    }
    more = {
        "half_across_left": lambda: (-0.5, fy()),
        "half_across_right": lambda: (w - 0.5, fy()),
        "half_across_top": lambda: (fx(), -0.5),
        "half_across_bottom": lambda: (fx(), h - 0.5),
        "x_on_last": lambda: (w - 1.0, fy()),
        "y_on_last": lambda: (fx(), h - 1.0),
        "corner_bottom_right": lambda: (w - 1 + q(), h - 1 + q()),
    }
    return must, more


def job_list(h, w, rng):
    """[(direction, target, mandatory)]: both directions of a recipe in turn"""
    must, more = recipes(h, w, rng)
    jobs = []
    for group, mandatory in ((must, True), (more, False)):
        for name in group:
            for _ in range(REPS):
                for d in (1, 0):
                    jobs.append((d, group[name](), mandatory))
    return jobs


def planted_flow(rng, case, ts):
    h, w, b, n_t = case
    R = max(h, w) + 3
    flow = sc.rand15(rng, (b, 4, h, w), float(R))
    npx = b * h * w
    half = [int(p) for p in rng.permutation(npx)]                          # pixels whose Ft0 at t = 0.5 is still free
    two_rows = 0.25 in ts
    quarter = [int(p) for p in rng.permutation(npx)] if two_rows else []   # ... at t = 0.25 (direction 0 only: Ft1 = -3 Ft0)
    d_half, d_quarter = {}, {}
    for d, (tx, ty), mandatory in job_list(h, w, rng):
        pool, store = (quarter, d_quarter) if (d == 0 and quarter) else (half, d_half)
        if not pool:
            assert not mandatory, "case %s has too few pixels for the mandatory classes" % (case,)
            continue
        p = pool.pop()
        py, px = (p % (h * w)) // w, p % w
        ft = (tx - px + 0.5, ty - py + 0.5)          # the blended flow that puts this pixel's sample on the target
        store[p] = ft if d == 0 else (-ft[0], -ft[1])  # as Ft0 (t = 0.5: Ft0 = -Ft1)
    free = lambda: tuple(float(v) / 4 for v in rng.integers(-2 * R, 2 * R + 1, 2))   # a multiple of 1/4 in +-R/2
    for p in sorted(set(d_half) | set(d_quarter)):
        d1 = d_half[p] if p in d_half else free()
        d2 = d_quarter[p] if p in d_quarter else free()
        bi, py, px = p // (h * w), (p % (h * w)) // w, p % w
        for a in (0, 1):
            f01 = 2 * d1[a] - 8 * d2[a] if two_rows else -2 * d1[a]
            f10 = f01 + 4 * d1[a]
            assert np.float32(f01) == f01 and np.float32(f10) == f10
            flow[bi, a, py, px], flow[bi, 2 + a, py, px] = f01, f10
    return flow


def planted_intrp(rng, case, x12):
    """[n_t][b][5][h][w]: random in +-3, planted residual flows, special visibility logits"""
    h, w, b, n_t = case
    intrp = sc.rand15(rng, (n_t, b, 5, h, w), 3.0)
    slots = [int(s) for s in rng.permutation(n_t * b * h * w)]
    jobs = job_list(h, w, rng)
    pairs = list(zip([j for j in jobs if j[0] == 0], [j for j in jobs if j[0] == 1]))   # one slot plants both directions
    for j0, j1 in pairs:
        while slots:
            s = slots.pop()
            ti, bi, py, px = s // (b * h * w), (s // (h * w)) % b, (s % (h * w)) // w, s % w
            r = []
            for (d, (tx, ty), _), ch in ((j0, 8), (j1, 6)):     # x12: Ft1 in channels 6, 7, Ft0 in 8, 9
                for a, (t, p) in enumerate(((tx, px), (ty, py))):
                    ft = np.float32(x12[ti, bi, ch + a, py, px])
                    want = np.float32(t - p + 0.5)
                    res = np.float32(want - ft)
                    if abs(t) < 1e4 and np.float32(res + ft) != want:
                        res = None
                    r.append(res)
            if all(v is not None for v in r):
                intrp[ti, bi, 0:4, py, px] = r
                break
        else:
            assert not (j0[2] or j1[2]), "case %s: no sample left for a mandatory class of the fusion" % (case,)
    for ti in range(n_t):
        for bi in range(b):
            where = rng.choice(h * w, len(sc.LOGITS), replace=False)
            intrp[ti, bi, 4].flat[where] = sc.LOGITS
    return intrp


def main():
    model = rh.ref_model()
    torch.set_num_threads(1)
    out = {}
    for k, case in enumerate(sc.EDGE_CASES):
        h, w, b, n_t = case
        ts = sc.EDGE_TS[n_t]
        rng = np.random.Generator(np.random.PCG64(4100 + k))
        fr = int_gradient_frames(b + 1, h, w, seed=40 + k, noise=10, as_array=True)
        I0 = torch.from_numpy(fr[:b].astype(np.float32) / 255.0).unsqueeze(1) - 0.428
        I1 = torch.from_numpy(fr[1:b + 1].astype(np.float32) / 255.0).unsqueeze(1) - 0.428
        warper = model.backWarp(w, h, "cpu")
        flow = planted_flow(rng, case, ts)
        tf = torch.from_numpy(flow)
        with torch.no_grad():
            first = ref_interp(model, None, None, warper, I0, I1, ts, flowOut=tf,
                               intrp_override=[torch.zeros((b, 5, h, w)) for _ in ts])
            intrp = planted_intrp(rng, case, first["x12"].numpy())
            o = ref_interp(model, None, None, warper, I0, I1, ts, flowOut=tf, intrp_override=[torch.from_numpy(v) for v in intrp])
        x12, Ft = o["x12"].numpy(), o["Ft"].numpy()
        assert np.isfinite(x12).all() and np.isfinite(Ft).all(), "the reference's outputs must be finite"
        assert np.array_equal(x12, first["x12"].numpy())
        d = dict(frames=fr, ts=np.asarray(ts), flow=flow, intrp=intrp, x12_tail=x12[:, :, 6:12], Ft=Ft)
        name = sc.case_name(case)
        for key, v in d.items():
            out[name + "_" + key] = v
        dd = dict(d, ts=ts)
        for what, pos in (("prep", sc.prep_positions(dd, case)), ("fuse", sc.fuse_positions(dd, case))):
            cen = sc.census(pos, case)
            print("%-12s %s %s" % (name, what, {k: min(c.values()) for k, c in cen.items()}), sc.census_short(cen))
            assert not sc.census_short(cen)
        print("%-12s Ft range [%.3f, %.3f], |flow| max %.0f" % (name, Ft.min(), Ft.max(), np.abs(flow).max()))
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, sc.EDGE_FIXTURE)
    with zipfile.ZipFile(path, "w") as zf:  # np.savez_compressed, with a fixed date in every entry: reruns give the same bytes
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    print(sc.EDGE_FIXTURE, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
