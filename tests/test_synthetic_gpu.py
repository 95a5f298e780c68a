"""GPU: v2e_amd/synthetic.py.  The frames of every fixture of tests/golden/make_golden_synth.py (recorded from the reference's
classes, every value measured to lie clear of a decision boundary) bit for bit from `frames_block`, whole and cut at awkward places,
into buffers with sentinel bands; the last dot of a list wins; next_frame(); and `SyntheticToEvents` against the reference events of
philox_moving_dot_64x64.npz and against per-frame generate_events."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest

from fixtures import GOLDEN, PhiloxFixture

pytestmark = pytest.mark.gpu

U8 = ["synth_moving_dot_64x64", "synth_moving_dot_97x131", "synth_moving_dot_clip_64x64", "synth_gradients_131x97",
      "synth_gradients_64x64", "synth_barberpole_97x131", "synth_barberpole_64x64"]
F32 = ["synth_particles_64x48", "synth_particles_hdr_64x48", "synth_particles_edge_64x48"]
_cache = {}


def load(name):
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        d = {k: z[k] for k in z.files}
        if "frames" not in d:  # the clip of BASELINE configs[0]: its frames are in the emulator's fixture
            d["frames"] = PhiloxFixture("philox_moving_dot_64x64").frames
        _cache[name] = d
    return _cache[name]


def source(name):
    import v2e_amd
    z = load(name)
    cls = getattr(v2e_amd, name.split("_")[1] if "moving_dot" not in name else "moving_dot")
    kw = {}
    if cls is v2e_amd.particles:
        kw = dict(parent_args=argparse.Namespace(hdr=bool(z["hdr"])), rng=np.random.RandomState(int(z["seed"])))
    return cls(int(z["W"]), int(z["H"]), arg_list=json.loads(str(z["arg_list"])), device="cuda", **kw), z


def banded(n, H, W, dtype, band):
    """A buffer with `band` sentinel elements before and after the [n, H, W] block; returns (whole, block view, check)."""
    import torch
    tdt = torch.uint8 if dtype == np.uint8 else torch.float32
    whole = torch.empty(n * H * W + 2 * band, dtype=tdt, device="cuda")
    whole.view(torch.uint8).fill_(0xA5)  # (as float32: -1.8e-16 in every element, a value no source produces)
    out = whole[band:band + n * H * W].view(n, H, W)

    def bands_intact():
        b = whole.view(torch.uint8).cpu().numpy()
        e = whole.element_size()
        return bool((b[:band * e] == 0xA5).all() and (b[(band + n * H * W) * e:] == 0xA5).all())
    return whole, out, bands_intact


@pytest.mark.parametrize("name", U8 + F32)
def test_frames_block_matches_reference_frames(name):
    """Bit equality, whole and in blocks of 1, 7, 64 and the remainder; the block starts 16 elements (aligned: full vector stores
    wherever H * W allows) and 13 elements (every frame starts off a 4-element boundary: ragged head and tail) into the buffer."""
    src, z = source(name)
    ref = z["frames"]
    n, H, W = ref.shape
    assert (src.h, src.w) == (H, W) and src.total_frames() == n
    whole, out, intact = banded(n, H, W, ref.dtype, 16)
    fr, t = src.frames_block(0, n, out=out)
    assert fr.data_ptr() == out.data_ptr() and np.array_equal(t, z["times"])
    got = out.cpu().numpy()
    assert got.dtype == ref.dtype and np.array_equal(got.view(np.uint8), ref.view(np.uint8))
    assert intact()
    src, _ = source(name)
    whole, out, intact = banded(n, H, W, ref.dtype, 13)
    k = 0
    for m in (1, 7, 64, n - 72):
        fr, t = src.frames_block(k, m, out=out[k:k + m])
        assert np.array_equal(t, z["times"][k:k + m])
        k += m
    assert k == n and np.array_equal(out.cpu().numpy().view(np.uint8), ref.view(np.uint8))
    assert intact()
    # without out=: a tensor of its own
    if "particles" not in name:
        fr, _ = src.frames_block(n - 5, 5)
        assert np.array_equal(fr.cpu().numpy(), ref[n - 5:])


def paint(offs, xy, box, n, H, W, bg, fg, sigma, d, peak):
    """fill_dot in list order with numpy (float64, no store conversion); also the number of boxes over every pixel."""
    fr = np.full((n, H, W), bg, np.float64)
    cover = np.zeros((n, H, W), np.int32)
    for f in range(n):
        for k in range(offs[f], offs[f + 1]):
            x0, y0 = box[k]
            for yy in range(max(0, y0 - d), min(H, y0 + d)):
                for xx in range(max(0, x0 - d), min(W, x0 + d)):
                    ddx, ddy = xx - xy[k][0], yy - xy[k][1]
                    v = min(1.0, peak * np.exp(-(ddx * ddx + ddy * ddy) / (sigma * sigma)))
                    fr[f, yy, xx] = bg + (fg - bg) * v
                    cover[f, yy, xx] += 1
    return fr, cover


def test_moving_dot_with_a_float_bg_renders_float64():
    """--bg on the command line is a float (argparse), and numpy then makes the reference's frame float64 (moving_dot.py:156): the
    same doubles without the uint8 store, so truncating them gives the uint8 clip of the same arguments."""
    src, z = source("synth_moving_dot_clip_64x64")
    from v2e_amd import moving_dot
    f64 = moving_dot(64, 64, arg_list=json.loads(str(z["arg_list"])) + ['--bg', '5'], device="cuda")
    assert type(f64.bg) is float and f64.fg == src.fg
    fr, _ = f64.frames_block(10, 33)
    got = fr.cpu().numpy()
    assert got.dtype == np.float64 and got.max() == 255.0 and (got != np.floor(got)).any()
    assert np.array_equal(got.astype(np.uint8), z["frames"][10:43])


@pytest.mark.parametrize("case", ["three_overlapping", "long_list"])
def test_last_dot_of_the_list_wins(case):
    """v2e_synth_dots on a hand-built table, float64 output.  three_overlapping: three boxes over one another (and one clipped at
    the corner, one wholly outside); every covered pixel has the value of the last dot that covers it, which differs from the
    other candidates' by far more than the comparison's 1e-12 (exp's last bits).  long_list: 1100 dots in one frame, more than
    one LDS chunk of the gather."""
    import torch
    from v2e_amd import _capi
    H, W, d, sigma, peak, bg, fg = 37, 45, 4, 3.0, 0.9, 10.0, 200.0
    if case == "three_overlapping":
        xy = np.array([[20.3, 18.6], [22.7, 19.2], [21.1, 21.4], [0.4, 0.2], [-30.0, 80.0], [10.5, 30.5]])
        offs = np.array([0, 5, 5, 6], np.int32)  # frame 1 has no dots
    else:
        r = np.random.RandomState(5)
        xy = np.stack([r.uniform(-3, W + 3, 1100), r.uniform(-3, H + 3, 1100)], axis=1)
        offs = np.array([0, 1100], np.int32)
    box = np.array([[round(x), round(y)] for x, y in xy], np.int32)
    n = len(offs) - 1
    want, cover = paint(offs, xy, box, n, H, W, bg, fg, sigma, d, peak)
    if case == "three_overlapping":
        assert cover[0].max() == 3 and (cover[1] == 0).all()
        tri = cover[0] == 3  # where all three overlap the first two dots' values are far from the third's
        first, _ = paint(np.array([0, 2], np.int32), xy, box, 1, H, W, bg, fg, sigma, d, peak)
        assert np.abs(first[0][tri] - want[0][tri]).min() > 1e-3
    else:
        assert cover.max() > 8
    out = torch.full((n, H, W), -7.0, dtype=torch.float64, device="cuda")
    dxy, dbox, doffs = (torch.from_numpy(a).cuda() for a in (xy, box, offs))
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(_capi.lib().v2e_synth_dots(p(dxy), p(dbox), p(doffs), n, H, W, p(out), _capi.DT_F64, bg, fg, sigma, d, peak, -1.0, 0,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "v2e_synth_dots")
    got = out.cpu().numpy()
    assert np.array_equal(got[cover == 0], want[cover == 0])  # bg exactly
    assert np.max(np.abs(got - want) / want) < 1e-12


@pytest.mark.parametrize("name", ["synth_moving_dot_clip_64x64", "synth_particles_edge_64x48"])
def test_next_frame_hands_out_the_same_frames(name):
    src, z = source(name)
    src.NEXT_FRAME_BLOCK = 48  # (100 and 200 frames: whole blocks and a remainder)
    for k in range(len(z["times"])):
        f, t = src.next_frame()
        assert isinstance(f, np.ndarray) and f.dtype == z["frames"].dtype and t == z["times"][k]
        assert np.array_equal(f.view(np.uint8), z["frames"][k].view(np.uint8)), "frame %d" % k
    assert src.frame_number == len(z["times"])
    for _ in range(2):
        f, t = src.next_frame()
        assert f is None and t == z["times"][-1]
    src.cleanup()


def text_body(path):
    lines = open(path, "rb").read().split(b"\n")
    k = 0
    while lines[k].startswith(b"#"):
        k += 1
    return b"\n".join(lines[k:])


@pytest.fixture(scope="module")
def moving_dot_twin(tmp_path_factory):
    """Per-frame generate_events on the fixture's frames with the text sink open: the drop-in way."""
    from v2e_amd import EventEmulator
    fx = PhiloxFixture("philox_moving_dot_64x64")
    tmp = tmp_path_factory.mktemp("twin")
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", output_folder=str(tmp), dvs_text="twin", **fx.kw)
    for f, t in zip(fx.frames, fx.times):
        emu.generate_events(f, float(t))
    emu.cleanup()
    return fx, text_body(str(tmp / "twin.txt"))


@pytest.mark.parametrize("block_frames", [500, 64, 37])
def test_synthetic_to_events_is_baseline_config0(block_frames, moving_dot_twin, tmp_path):
    """BASELINE configs[0] with no frame on the host: the reference's events, order and counts, and the text file of the per-frame run."""
    from v2e_amd import EventEmulator, SyntheticToEvents
    fx, twin_text = moving_dot_twin
    src, _ = source("synth_moving_dot_64x64")
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", output_folder=str(tmp_path), dvs_text="run", **fx.kw)
    ev, counts, n = SyntheticToEvents(src, emu, block_frames=block_frames).run()
    emu.cleanup()
    assert n == 500 and list(counts) == list(fx.n_events)
    want = np.concatenate([e for e in fx.events if len(e)])
    assert ev.dtype == np.float32 and np.array_equal(ev.view(np.uint32), want.view(np.uint32))
    assert [emu.num_events_total, emu.num_events_on, emu.num_events_off] == list(fx.counters)
    assert text_body(str(tmp_path / "run.txt")) == twin_text and twin_text.count(b"\n") == len(want)


def test_synthetic_to_events_on_events_and_device_rows():
    """on_events gets every block once, in order; return_device gives the same rows as device tensors."""
    import torch
    from v2e_amd import EventEmulator, SyntheticToEvents
    fx = PhiloxFixture("philox_moving_dot_64x64")
    want = np.concatenate([e for e in fx.events if len(e)])
    got, firsts = [], []

    def on_events(ev, cnt, frame0):
        firsts.append((frame0, len(cnt)))
        if ev is not None:
            assert torch.is_tensor(ev) and int(np.sum(cnt)) == ev.shape[0]
            got.append(ev.cpu().numpy())
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **fx.kw)
    ev, counts, n = SyntheticToEvents(source("synth_moving_dot_64x64")[0], emu, block_frames=128).run(on_events, return_device=True)
    assert ev is None and n == 500 and list(counts) == list(fx.n_events)
    assert firsts == [(0, 128), (128, 128), (256, 128), (384, 116)]
    assert np.array_equal(np.concatenate(got).view(np.uint32), want.view(np.uint32))
    emu = EventEmulator(device="cuda", seed=fx.seed, rng_mode="philox", **fx.kw)
    ev, counts, n = SyntheticToEvents(source("synth_moving_dot_64x64")[0], emu, block_frames=200).run(return_device=True)
    assert torch.is_tensor(ev) and np.array_equal(ev.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_particles_take_the_float32_path():
    """float32 frames in HBM -> the emulator's f32 input path: the events of per-frame generate_events on the fixture's frames."""
    from v2e_amd import EventEmulator, SyntheticToEvents
    kw = dict(pos_thres=0.1, neg_thres=0.1, sigma_thres=0.02, cutoff_hz=200, leak_rate_hz=0.1, shot_noise_rate_hz=1.0,
              refractory_period_s=0.0)
    src, z = source("synth_particles_64x48")
    assert z["frames"].dtype == np.float32
    twin = EventEmulator(device="cuda", seed=3, rng_mode="philox", **kw)
    per = [twin.generate_events(f, float(t)) for f, t in zip(z["frames"], z["times"])]
    want = np.concatenate([e for e in per if e is not None])
    assert len(want) > 1000
    emu = EventEmulator(device="cuda", seed=3, rng_mode="philox", **kw)
    ev, counts, n = SyntheticToEvents(src, emu, block_frames=64).run()
    assert n == 200 and list(counts) == [0 if e is None else len(e) for e in per]
    assert np.array_equal(ev.view(np.uint32), want.view(np.uint32))
    assert src.particle_count == int(z["final_particle_count"])
