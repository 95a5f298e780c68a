"""CPU-only: the host part of v2e_amd/synthetic.py -- times, theta, dot tables, bump centres and the `particles` state machine --
against what tests/golden/make_golden_synth.py recorded from the reference's classes; argument parsing; the refusals."""
import argparse
import json
import os

import numpy as np
import pytest

from fixtures import GOLDEN

MOVING_DOT = ["synth_moving_dot_64x64", "synth_moving_dot_97x131", "synth_moving_dot_clip_64x64"]
PARTICLES = ["synth_particles_64x48", "synth_particles_hdr_64x48", "synth_particles_edge_64x48"]
GRADIENTS = ["synth_gradients_131x97", "synth_gradients_64x64"]
BARBERPOLE = ["synth_barberpole_97x131", "synth_barberpole_64x64"]


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return z, json.loads(str(z["arg_list"])), int(z["W"]), int(z["H"])


def same_table(got, z, lo=None, hi=None):
    offs, xy, box = got
    o = z["dot_offs"]
    lo, hi = (0, len(o) - 1) if lo is None else (lo, hi)
    a, b = int(o[lo]), int(o[hi])
    assert np.array_equal(offs, o[lo:hi + 1] - a)
    assert offs.dtype == np.int32 and xy.dtype == np.float64 and box.dtype == np.int32
    assert np.array_equal(xy.view(np.uint64), z["dot_xy"][a:b].view(np.uint64))  # the float centres bit for bit
    assert np.array_equal(box, z["dot_box"][a:b])


@pytest.mark.parametrize("name", MOVING_DOT)
def test_moving_dot_host_part(name):
    from v2e_amd import moving_dot
    z, args, W, H = load(name)
    g = moving_dot(W, H, arg_list=args)
    assert g.total_frames() == len(z["times"]) and np.array_equal(g.times, z["times"])
    assert np.array_equal(g.theta.view(np.uint64), z["theta"].view(np.uint64))
    assert (g.bg, g.fg) == (int(z["bg"]), int(z["fg"])) and type(g.bg) is int
    same_table(g.dot_table(0, g.total_frames()), z)
    same_table(g.dot_table(37, 50), z, 37, 87)  # random access: any block, any time
    same_table(g.dot_table(0, 1), z, 0, 1)


@pytest.mark.parametrize("name", PARTICLES)
def test_particles_state_sequence(name):
    """Frame by frame: the drawn particles in draw order and particle_count -- the removal-while-iterating skips, the particles
    appended and visited in the same frame, the replaced ones not drawn."""
    from v2e_amd import particles
    z, args, W, H = load(name)
    hdr = bool(z["hdr"])
    g = particles(W, H, arg_list=args, parent_args=argparse.Namespace(hdr=hdr), rng=np.random.RandomState(int(z["seed"])))
    assert np.array_equal(g.times, z["times"])
    assert float(g.bg) == float(z["bg"]) and float(g.fg) == float(z["fg"])
    counts = z["particle_count"]
    assert int(counts[-1]) - g.num_particles >= 24  # dozens of particles leave and are replaced in this clip
    for k in range(g.total_frames()):
        same_table(g.dot_table(k, 1), z, k, k + 1)
        assert g.particle_count == counts[k], "frame %d" % k
    assert g.particle_count == int(z["final_particle_count"])
    # the global np.random module is the default stream, as in the reference; blocks of any size give the same sequence
    np.random.seed(int(z["seed"]))
    g = particles(W, H, arg_list=args, parent_args=argparse.Namespace(hdr=hdr))
    k = 0
    for n in (7, 64, 1, 100, 28):
        same_table(g.dot_table(k, n), z, k, k + n)
        k += n
    assert k == g.total_frames() and g.particle_count == int(z["final_particle_count"])


def test_particles_blocks_out_of_order_raise():
    from v2e_amd import particles
    g = particles(64, 48, arg_list=['--num_particles', '3', '--dt', '1e-3', '--total_time', '0.05'], rng=np.random.RandomState(1))
    with pytest.raises(ValueError):
        g.dot_table(5, 2)
    g.dot_table(0, 4)
    with pytest.raises(ValueError):
        g.dot_table(0, 4)  # a frame cannot be taken twice
    with pytest.raises(ValueError):
        g.dot_table(6, 1)
    g.dot_table(4, 2)
    with pytest.raises(ValueError):
        g.dot_table(6, 100)  # past the end: refused before the state moves
    g.dot_table(6, 44)


def test_moving_dot_box_off_frame_raises():
    from v2e_amd import moving_dot
    # the defaults on a 64 x 64 frame: radius 100 puts every dot outside
    g = moving_dot(64, 64, arg_list=['--t_total', '0.01'])
    with pytest.raises(ValueError):
        g.dot_table(0, 1)
    # a box that touches the edge is fine, one pixel further is not: centre (32 + r, 32), d = 3
    ok = moving_dot(64, 64, arg_list=['--t_total', '0.0002', '--radius', '29', '--num_particles', '1'])
    assert ok.dot_table(0, 1)[2].tolist() == [[61, 32]]
    bad = moving_dot(64, 64, arg_list=['--t_total', '0.0002', '--radius', '30', '--num_particles', '1'])
    with pytest.raises(ValueError):
        bad.dot_table(0, 1)
    with pytest.raises(Exception):
        moving_dot(64, 64, arg_list=[])  # neither --cycles nor --t_total (moving_dot.py:80-81)
    assert moving_dot(64, 64, arg_list=['--t_total', '0.01', '--contrast', '1']).dot_table(0, 5)[0].tolist() == [0] * 6


@pytest.mark.parametrize("name", GRADIENTS)
def test_gradients_host_part(name):
    from v2e_amd import gradients
    z, args, W, H = load(name)
    g = gradients(W, H, arg_list=args)
    assert np.array_equal(g.times, z["times"])
    assert np.array_equal(g.bump_centres(0, g.total_frames()).view(np.uint64), z["p"].view(np.uint64))
    assert np.array_equal(g.bump_centres(11, 5).view(np.uint64), z["p"][11:16].view(np.uint64))


@pytest.mark.parametrize("name", BARBERPOLE)
def test_barberpole_host_part(name):
    from v2e_amd import barberpole
    z, args, W, H = load(name)
    g = barberpole(W, H, arg_list=args)
    assert np.array_equal(g.times, z["times"])
    y, x = np.mgrid[0:H, 0:W]
    pole = (x > g.minx) & (x < g.maxx) & (y > g.miny) & (y < g.maxy)
    assert int(pole.sum()) == int(z["pole"][0])
    assert np.array_equal(z["frames"][0][~pole], np.full(int((~pole).sum()), g.bg, np.uint8))


DEFAULTS = {
    "moving_dot": (['--cycles', '2'], dict(num_dots=5, contrast=10, bg=5, fg=50, radius=100, dt=100e-6, cycles=2.0, d=3, dot_sigma=1,
                                           speed_pps=1000)),
    "particles": ([], dict(num_particles=300, contrast=1.25, bg=127, radius=1, t_total=1, speed_pps_min=3, speed_pps_max=100,
                           dt=100e-6, start_on_edge=False)),
    "gradients": ([], dict(contrast=2, t_total=1, speed_pps=300, dt=100e-6, bump_width=.5, bg=127)),
    "barberpole": ([], dict(num_stripes=6, contrast=1.5, t_total=1, speed_pps=1000, dt=100e-6, bb_width=.8, bb_height=.2,
                            bb_angle=30, bg=127)),
}
FLAGS = {
    "moving_dot": ['--num_particles', '7', '--contrast', '1.5', '--bg', '20', '--radius', '50', '--dt', '2e-4', '--t_total', '0.01'],
    "particles": ['--num_particles', '9', '--contrast', '1.1', '--bg', '60', '--radius', '1.5', '--total_time', '0.01',
                  '--speed_min', '10', '--speed_max', '20', '--dt', '1e-3', '--edge'],
    "gradients": ['--contrast', '3', '--total_time', '0.01', '--speed_pps', '100', '--dt', '1e-3', '--bump_width', '.25'],
    "barberpole": ['--num_stripes', '3', '--contrast', '2', '--total_time', '0.01', '--speed_pps', '500', '--dt', '1e-3',
                   '--bb_width', '.5', '--bb_height', '.4', '--bb_angle', '55'],
}


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_arguments_parse_as_the_reference(name):
    import v2e_amd
    import ref_harness as rh
    cls = getattr(v2e_amd, name)
    args, want = DEFAULTS[name]
    np.random.seed(3)
    g = cls(346, 260, None, False, args, argparse.Namespace(hdr=False))
    for k, v in want.items():
        assert getattr(g, k) == v and type(getattr(g, k)) is type(v), k
    assert g.total_frames() == len(np.arange(0, g.t_total, g.dt)) and g.frame_number == 0
    with pytest.raises(SystemExit):
        cls(346, 260, arg_list=['--no_such_flag', '1'])
    if rh.reference_available():  # attribute by attribute against an instance of the reference's class, defaults and every flag
        import importlib
        import logging
        rh.ref_moving_dot()
        ref_cls = getattr(importlib.import_module("scripts." + name), name)
        logging.disable(logging.CRITICAL)
        try:
            for al in (args, FLAGS[name]):
                kw = dict(width=346, height=260, preview=False, arg_list=al)
                if name == "particles":
                    kw["parent_args"] = argparse.Namespace(hdr=False)
                np.random.seed(3)
                r = ref_cls(**kw)
                np.random.seed(3)
                g = cls(346, 260, arg_list=al, parent_args=argparse.Namespace(hdr=False))
                keys = [k for k, v in vars(g).items() if not k.startswith("_") and hasattr(r, k)
                        and isinstance(v, (int, float, bool, np.floating)) and k not in ("preview",)]
                assert len(keys) >= 6
                for k in keys:
                    assert getattr(g, k) == getattr(r, k), k
                assert np.array_equal(g.times, r.times)
        finally:
            logging.disable(logging.NOTSET)


def test_c_symbols_exported_and_declared():
    import ctypes
    from v2e_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "v2e_amd.h")).read()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("v2e_synth_dots", "v2e_synth_gradients", "v2e_synth_barberpole"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and ("int %s(" % name) in header
    assert "synth.o" in open(os.path.join(root, "v2e_amd", "csrc", "Makefile")).read()
