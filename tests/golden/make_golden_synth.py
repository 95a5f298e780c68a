"""Fixtures for v2e_amd/synthetic.py, recorded from the reference's own classes (scripts/moving_dot.py, particles.py,
gradients.py, barberpole.py) through ref_harness (its numba stub runs fill_dot as plain Python).

Every fixture holds the reference's frames, what the host part must reproduce (times, per-frame dot lists, bump centres, the
final particle_count) and `margin`: the device's exp / sin / tanh may differ from this host's numpy in the last bits, and a stored
pixel can differ only where the value before the store sits on a decision boundary.  So this script recomputes every pre-store
value in float64 and asserts
  (a) its own store equals the reference's frame, and
  (b) every value that went through a transcendental is at a relative distance above MARGIN = 1e-9 from the nearest integer
      (uint8 outputs) and from the v > 1 and v < .01 cuts; the exact-arithmetic values of `gradients` are held to the same.
For `particles` (float32 frames) the boundary is a float32 rounding midpoint.  Midpoints lie one float32 ulp apart (6e-8 .. 1.2e-7
relative), so of the ~2e5 distinct gaussian-tail values of a 200-frame clip some 2 % lie within 1e-9 of one whatever the seed:
that figure cannot be met there.  What the device can move a value by is a few float64 ulps (2.2e-16 relative: exp is within one
ulp on either side, and bg + diff * v adds no more); MARGIN_F32 = 1e-13 leaves two orders of magnitude above that, and the seed
is the first for which it holds.  The smallest margins found are stored; they are what entitles the GPU tests to demand bit equality.

Run from the repository root with the reference tree present: python tests/golden/make_golden_synth.py
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

MARGIN = 1e-9
MARGIN_F32 = 1e-13


def ref_module(name):
    rh.ref_moving_dot()  # installs the stubs (skimage among them)
    return importlib.import_module("scripts." + name)


def record(mod, cls, kw, hook_fill_dot=None, after_frame=None):
    """All frames and times of one reference instance; fill_dot's calls are reported to hook_fill_dot(frame, args)."""
    calls = []
    if hook_fill_dot is not None:
        orig = mod.fill_dot

        def spy(*a):
            calls.append(hook_fill_dot(*a))
            return orig(*a)
        mod.fill_dot = spy
    try:
        g = getattr(mod, cls)(**kw)
        frames, times, offs, extra = [], [], [0], []
        for _ in range(g.total_frames()):
            f, t = g.next_frame()
            frames.append(np.array(f))  # (particles hands out the same array every time)
            times.append(float(t))
            offs.append(len(calls))
            if after_frame is not None:
                extra.append(after_frame(g))
        end = g.next_frame()
        assert end[0] is None and end[1] == g.times[-1]
    finally:
        if hook_fill_dot is not None:
            mod.fill_dot = orig
    return g, np.stack(frames), np.asarray(times), np.asarray(offs, np.int32), calls, extra


def rel_dist_to_integer(v):
    return np.abs(v - np.rint(v)) / np.maximum(np.abs(v), 1e-300)


def rel_dist_to_f32_midpoint(v):
    f = v.astype(np.float32)
    up = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    dn = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(v - up), np.abs(v - dn)) / np.maximum(np.abs(v), 1e-300)


def render_dots(offs, xy, box, n, H, W, bg, fg, sigma, d, peak, low_cut, clip, dtype, clip_boxes):
    """fill_dot recomputed per dot with numpy; returns the frames and the smallest margins of the values that went through exp."""
    frames = np.empty((n, H, W), dtype)
    frames[:] = bg
    m = {"integer": np.inf, "cut_high": np.inf, "cut_low": np.inf, "f32_midpoint": np.inf}
    for f in range(n):
        for k in range(offs[f], offs[f + 1]):
            x, y = xy[k]
            x0, y0 = int(box[k][0]), int(box[k][1])
            xs, ys = np.arange(x0 - d, x0 + d), np.arange(y0 - d, y0 + d)
            if clip_boxes:
                xs, ys = xs[(xs >= 0) & (xs < W)], ys[(ys >= 0) & (ys < H)]
            else:
                assert xs[0] >= 0 and xs[-1] < W and ys[0] >= 0 and ys[-1] < H, "moving_dot box leaves the frame"
            if not len(xs) or not len(ys):
                continue
            ddx, ddy = xs[None, :] - x, ys[:, None] - y
            dist2 = ddx * ddx + ddy * ddy
            v = peak * np.exp(-dist2 / (sigma * sigma))
            m["cut_high"] = min(m["cut_high"], float(np.min(np.abs(v - 1))))
            if low_cut is not None:
                m["cut_low"] = min(m["cut_low"], float(np.min(np.abs(v - low_cut) / low_cut)))
            live = (v <= 1) & ((v >= low_cut) if low_cut is not None else True)
            v = np.where(v > 1, 1.0, v)
            if low_cut is not None:
                v = np.where(v < low_cut, 0.0, v)
            pv = bg + (fg - bg) * v
            if live.any():
                if dtype == np.uint8:
                    m["integer"] = min(m["integer"], float(np.min(rel_dist_to_integer(pv[live]))))
                elif dtype == np.float32:
                    m["f32_midpoint"] = min(m["f32_midpoint"], float(np.min(rel_dist_to_f32_midpoint(pv[live]))))
            if clip:
                pv = np.where(pv > 255, 255.0, np.where(pv < 0, 0.0, pv))
            frames[f][np.ix_(ys, xs)] = pv.astype(dtype)
    return frames, {k: v for k, v in m.items() if np.isfinite(v)}


def save(name, **out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-36s %6.0f KB  margin %s" % (name, os.path.getsize(path) / 1024, out.get("margin")))
    assert os.path.getsize(path) < (1 << 20)


def check_margins(m, f32=False):
    for k, v in m.items():
        need = MARGIN_F32 if k == "f32_midpoint" else MARGIN
        if not v > need:
            return False
    return True


def make_moving_dot(name, W, H, arg_list, store_frames=True):
    mod = ref_module("moving_dot")
    g, frames, times, offs, calls, _ = record(
        mod, "moving_dot", dict(width=W, height=H, preview=False, arg_list=arg_list),
        hook_fill_dot=lambda pix, x, x0, y, y0, d, fg, bg, s: (float(x), float(y), int(x0), int(y0)))
    xy = np.asarray([c[:2] for c in calls], np.float64).reshape(-1, 2)
    box = np.asarray([c[2:] for c in calls], np.int32).reshape(-1, 2)
    assert frames.dtype == np.uint8
    own, m = render_dots(offs, xy, box, len(times), H, W, g.bg, g.fg, g.dot_sigma, g.d, 10, .01, True, np.uint8, False)
    assert np.array_equal(own, frames), name + ": the recomputed frames differ from the reference's"
    assert check_margins(m), (name, m)
    out = dict(arg_list=json.dumps(arg_list), W=W, H=H, times=times, theta=np.asarray(g.theta), dot_offs=offs, dot_xy=xy, dot_box=box,
               bg=g.bg, fg=g.fg, margin=json.dumps(m))
    if store_frames:
        out["frames"] = frames
    save(name, **out)
    return frames


def make_particles(name, W, H, arg_list, hdr):
    mod = ref_module("particles")
    for seed in range(1, 200):
        np.random.seed(seed)
        g, frames, times, offs, calls, counts = record(
            mod, "particles", dict(width=W, height=H, preview=False, arg_list=arg_list, parent_args=argparse.Namespace(hdr=hdr)),
            hook_fill_dot=lambda pix, x, y, fg, bg, r: (float(x), float(y)), after_frame=lambda g: g.particle_count)
        xy = np.asarray(calls, np.float64).reshape(-1, 2)
        box = np.asarray([(round(x), round(y)) for x, y in calls], np.int32).reshape(-1, 2)
        d = int(g.radius * 2) + 1
        own, m = render_dots(offs, xy, box, len(times), H, W, g.bg, g.fg, g.radius, d, 2, None, False, np.float32, True)
        # (with hdr numpy >= 2 promotes the reference's frame to float64, np.log being a float64 scalar; numpy 1.x keeps the float32
        #  frame the reference declares, which is what rounding each stored value to float32 gives)
        assert np.array_equal(own, frames.astype(np.float32)), name + ": the recomputed frames differ from the reference's"
        if check_margins(m):
            break
        print("  %s: seed %d misses the margin %s" % (name, seed, m))
    else:
        raise SystemExit(name + ": no seed meets the margins")
    replaced = int(g.particle_count) - g.num_particles
    assert replaced >= 24, "%s: only %d particles were replaced" % (name, replaced)
    save(name, arg_list=json.dumps(arg_list), W=W, H=H, hdr=hdr, seed=seed, times=times, frames=own, dot_offs=offs, dot_xy=xy,
         dot_box=box, particle_count=np.asarray(counts, np.int64), final_particle_count=int(g.particle_count), bg=float(g.bg),
         fg=float(g.fg), margin=json.dumps(m))


def make_gradients(name, W, H, arg_list):
    mod = ref_module("gradients")
    g, frames, times, _, _, _ = record(mod, "gradients", dict(width=W, height=H, preview=False, arg_list=arg_list))
    low = (g.bg * 2) / (g.contrast + 1)
    high = g.contrast * low
    diff = high - low
    w2 = (g.bump_width * g.w) / 2
    x = np.arange(W).astype(np.float64)
    own = np.empty_like(frames)
    ps, margin = [], np.inf
    for f, t in enumerate(g.times):
        p = w2 + t * g.speed_pps
        p2 = p + w2 * 2
        row = np.full(W, low)
        ind = (x > p - w2) & (x < p)
        row[ind] = high + (-diff / w2) * (p - x[ind])
        ind = (x <= p + w2) & (x >= p)
        row[ind] = high + (-diff / w2) * (x[ind] - p)
        ind = (x > p2) & (x <= p2 + 10)
        row[ind] = high
        margin = min(margin, float(np.min(rel_dist_to_integer(row))))
        own[f] = row.astype(np.uint8)[None, :]
        ps.append(p)
    assert np.array_equal(own, frames), name
    m = {"integer": margin}
    assert check_margins(m), (name, m)
    save(name, arg_list=json.dumps(arg_list), W=W, H=H, times=times, frames=frames, p=np.asarray(ps, np.float64), margin=json.dumps(m))


def make_barberpole(name, W, H, arg_list):
    mod = ref_module("barberpole")
    g, frames, times, _, _, _ = record(mod, "barberpole", dict(width=W, height=H, preview=False, arg_list=arg_list))
    wavelength = (g.bb_width * g.w) / g.num_stripes
    low = (g.bg * 2) / (g.contrast + 1)
    diff = (g.contrast - 1) * low
    tan = np.tan((90 - g.bb_angle) * np.pi / 180)
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    pole = g.pole_mask == 1
    assert pole.any()
    own = np.empty_like(frames)
    margin = np.inf
    for f, t in enumerate(g.times):
        u = low + diff * 0.5 * (1 + np.tanh(10 * np.sin(2 * np.pi * (y - tan * x - t * g.speed_pps) / wavelength)))
        margin = min(margin, float(np.min(rel_dist_to_integer(u[pole]))))
        fr = np.uint8(np.floor(u))
        fr[~pole] = g.bg
        own[f] = fr
    assert np.array_equal(own, frames), name
    m = {"integer": margin}
    assert check_margins(m), (name, m)
    save(name, arg_list=json.dumps(arg_list), W=W, H=H, times=times, frames=frames, pole=np.asarray([g.pole_mask.sum()]),
         margin=json.dumps(m))


def main():
    import logging
    logging.disable(logging.CRITICAL)
    # the clip of philox_moving_dot_64x64.npz (make_golden.py:260-270): its frames are stored there; here its dot table and margins
    fr = make_moving_dot("synth_moving_dot_64x64", 64, 64, ['--radius', '20', '--t_total', '0.05', '--dt', '1e-4', '--num_particles', '3'],
                         store_frames=False)
    assert np.array_equal(fr, np.load(os.path.join(HERE, "philox_moving_dot_64x64.npz"))["frames"])
    make_moving_dot("synth_moving_dot_97x131", 97, 131, ['--radius', '30', '--t_total', '0.02', '--dt', '1e-4', '--num_particles', '5',
                                                         '--contrast', '0.45'])
    # fg = int(5 * 60) = 300: the centre of every dot is clipped to 255 (moving_dot.py:50-51)
    make_moving_dot("synth_moving_dot_clip_64x64", 64, 64, ['--radius', '22', '--t_total', '0.01', '--dt', '1e-4', '--num_particles', '4',
                                                            '--contrast', '60'])
    pa = ['--num_particles', '40', '--dt', '1e-3', '--total_time', '0.2', '--speed_min', '100', '--speed_max', '600']
    make_particles("synth_particles_64x48", 64, 48, pa, hdr=False)
    make_particles("synth_particles_hdr_64x48", 64, 48, pa, hdr=True)
    make_particles("synth_particles_edge_64x48", 64, 48, pa + ['--edge'], hdr=False)
    ta = ['--total_time', '0.15', '--dt', '1e-3']
    make_gradients("synth_gradients_131x97", 131, 97, ta)
    make_gradients("synth_gradients_64x64", 64, 64, ta + ['--contrast', '1.7', '--bump_width', '0.4', '--speed_pps', '250'])
    make_barberpole("synth_barberpole_97x131", 97, 131, ta + ['--bb_angle', '40', '--num_stripes', '4', '--bb_height', '0.5'])
    make_barberpole("synth_barberpole_64x64", 64, 64, ta)


if __name__ == "__main__":
    main()
