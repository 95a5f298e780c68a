"""The DVS frame renderer's window kernels (v2e_amd/csrc/render.hip) on the MI355X, on crafted edge packets: the reference's
own results (tests/golden/renderer_edges.npz, recorded by tests/golden/make_golden_renderer_edges.py) and, beyond the fixture,
seeded packets against the sequential model tests/renderer_ref.py, which tests/test_renderer_edges.py pins to the same fixture.
Every comparison is exact: frames are integers over 2 * full scale in float64, everything else integers or sums of grid stamps.

  per-packet path   EventRenderer.render_events_to_frames, host array and device tensor: frames, currentFrame, area_counts and
                    currentFrameStartTime after every packet
  whole-run path    render_run + flush_run on the same clips cut into emulator frames and runs in three ways: frames, bytes,
                    frame times, numFramesWritten and the state left behind
  EventFrameAccumulator on the histogram-rule packets

Mutants of render.hip these tests were checked against (each built into the library and run once; "before": also caught by
test_sinks.py / test_render_run_gpu.py / test_video_render_gpu.py as they stood):
  pos = end -> end + 1                          caught (108 tests; before: yes)
  end >= n - 1 -> end >= n                      caught (56; before: yes)
  k1 line removed, k_render_hist / k_run_hist   caught (9 / 9; before: only as a difference between the two paths)
  !(t_sl > nxt) -> !(t_sl >= nxt), host too     caught (12; before: no)
  e.w == 1.0f -> e.w > 0.f                      caught (24; before: no)
  fi < bins_y -> fi <= bins_y                   caught (8, run on the hist_first_window cases only; before: not run)
  last = (m & gt) == 0ull -> true               NOT caught, by no test: every lane of a cell then stores its count to the same
                                                LDS word in one instruction and the hardware keeps the highest lane's, which
                                                is the right one (area1_c65_n66 ... need 64 such lanes to agree); the
                                                predicate guards an order the language does not promise
"""
import os

import numpy as np
import pytest
import torch

from renderer_ref import RendererModel, clip_packets, histogram, load_fixture, random_packets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, NUMPY_VERSION, F32_TIME = load_fixture(os.path.join(ROOT, "tests", "golden", "renderer_edges.npz"))
F32_HERE = type(np.float32(0) + 0.5) is np.float32
MODES = ("duration", "count", "area_count", "source")
H, W = 24, 32


def same(a, b):
    """None where None, else equal shape, float64 and bits."""
    if a is None or b is None:
        return a is None and b is None
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = np.asarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b) and \
        np.array_equal(a.view(np.int64), b.view(np.int64))


def renderer(mode, value, full_scale_count, area_dimension):
    from v2e_amd.renderer import EventRenderer, ExposureMode
    return EventRenderer(full_scale_count=full_scale_count, exposure_mode=ExposureMode[mode.upper()],
                         exposure_value=value if value is not None else 1 / 300.0, area_dimension=area_dimension)


def needs_the_fixtures_numpy(c):
    if c.family == "duration_offgrid" and F32_HERE != F32_TIME:
        pytest.skip("off the binary grid the frames depend on numpy's promotion of float32 + float: the fixture was recorded "
                    "with numpy %s (float32 kept: %s), this numpy %s gives %s" % (NUMPY_VERSION, F32_TIME, np.__version__, F32_HERE))


def check_state(r, mode, cur, ac, start, where):
    assert same(r.currentFrame, cur), where
    if mode == "area_count":
        assert np.array_equal(r.area_counts.cpu().numpy(), ac), where
    if mode == "duration":
        assert float(r.currentFrameStartTime) == float(start), where


# ------------------------------------------------------------------------------------------------------- per-packet path
@pytest.mark.parametrize("name", sorted(CASES))
def test_per_packet_call_equals_the_reference(name):
    c = CASES[name]
    needs_the_fixtures_numpy(c)
    for as_tensor in (False, True):
        r = renderer(c.mode, c.value, c.full_scale_count, c.area_dimension)
        for k, pk in enumerate(c.packets):
            fr = r.render_events_to_frames(torch.from_numpy(pk.copy()).cuda() if as_tensor else pk.copy(), c.h, c.w, return_frames=True)
            assert same(fr, c.frames[k]), (name, as_tensor, k)
            check_state(r, c.mode, c.cur[k], None if c.ac is None else c.ac[k], None if c.start is None else c.start[k],
                        (name, as_tensor, k))


@pytest.mark.parametrize("mode", MODES)
def test_per_packet_call_equals_the_model_on_generated_packets(mode):
    for seed in range(24):
        kw, packets = random_packets(mode, seed)
        m = RendererModel(f32_time=F32_HERE, **kw)
        r = renderer(mode, kw.get("value"), kw["full_scale_count"], kw.get("area_dimension"))
        for k, pk in enumerate(packets):
            want = m.render(pk, H, W)
            fr = r.render_events_to_frames(torch.from_numpy(pk).cuda() if (seed + k) % 2 else pk, H, W, return_frames=True)
            assert same(fr, want), (mode, seed, k)
            check_state(r, mode, m.currentFrame, m.area_counts, m.currentFrameStartTime, (mode, seed, k))


# -------------------------------------------------------------------------------------------------------- whole-run path
def one_frame_per_packet(lens):
    """(counts, batch_size, cuts): every packet is one emulator frame, flushed at once; one run."""
    return list(lens), 1, [0, len(lens)]


def a_run_per_few_frames(lens):
    """The same frames, rendered in runs of one, two and more frames."""
    P = len(lens)
    return list(lens), 1, sorted({0, 1, 3, P // 2, P - 1, P} & set(range(P + 1)))


def three_frames_per_packet(lens):
    """batch_size 3 behind an empty frame 0: every packet is spread over three emulator frames (the first two may be empty),
    the last over two, so that it is left to flush_run; the runs are cut inside packets, so rows stay pending between them."""
    counts = [0]
    for n in lens[:-1]:
        a = (n - 1) // 2
        counts += [a, n - 1 - a, 1]
    counts += [lens[-1] // 2, lens[-1] - lens[-1] // 2]
    F = len(counts)
    return counts, 3, sorted({0, 2, 5, F // 2, F} & set(range(F + 1)))


WAYS = (one_frame_per_packet, a_run_per_few_frames, three_frames_per_packet)


def render_clip(r, packets, h, w, way, **kw):
    """render_run over the runs of `way`, then flush_run: (frames, times) on the host, None without frames."""
    lens = [len(p) for p in packets]
    rows = torch.from_numpy(np.concatenate(packets)).cuda()
    counts, bs, cuts = way(lens)
    assert sum(counts) == len(rows)
    off = np.concatenate(([0], np.cumsum(counts)))
    assert [e for _, e in clip_packets(counts, bs)] == list(np.cumsum(lens)), way.__name__  # this way forms the clip's own packets
    frames, times = [], []
    for a, b in zip(cuts, cuts[1:]):
        fr, t = r.render_run(rows[off[a]:off[b]], counts[a:b], h, w, frame0=a, batch_size=bs, **kw)
        assert (fr is None) == (t is None)
        if fr is not None:
            assert len(fr) == len(t) and t.dtype == torch.float64
            frames.append(fr)
            times.append(t)
    fr, t = r.flush_run(h, w, **kw)
    assert (fr is None) == (t is None)
    if fr is not None:
        frames.append(fr)
        times.append(t)
    assert r.flush_run(h, w, **kw) == (None, None)
    if not frames:
        return None, np.zeros(0)
    return torch.cat(frames).cpu().numpy(), torch.cat(times).cpu().numpy()


def check_clip(make, packets, h, w, mode, want_frames, want_times, cur, ac, start, where):
    for way in WAYS:
        for as_u8 in (False, True):
            r = make()
            frames, times = render_clip(r, packets, h, w, way, as_u8=as_u8)
            tag = (where, way.__name__, as_u8)
            if len(want_frames) == 0:
                assert frames is None, tag
            elif as_u8:
                want = (want_frames * 255).astype(np.uint8)  # the bytes the reference hands its AVI writer
                assert frames.dtype == np.uint8 and frames.shape == want.shape and np.array_equal(frames, want), tag
            else:
                assert same(frames, want_frames), tag
            assert times.dtype == np.float64 and np.array_equal(times.view(np.int64), np.asarray(want_times).view(np.int64)), tag
            assert r.numFramesWritten == len(want_frames), tag
            check_state(r, mode, cur, ac, start, tag)


@pytest.mark.parametrize("name", sorted(CASES))
def test_whole_run_equals_the_reference(name):
    c = CASES[name]
    needs_the_fixtures_numpy(c)
    check_clip(lambda: renderer(c.mode, c.value, c.full_scale_count, c.area_dimension), c.packets, c.h, c.w, c.mode, c.all_frames,
               c.times, c.cur[-1], None if c.ac is None else c.ac[-1], None if c.start is None else c.start[-1], name)


def test_the_long_clips_pass_the_run_kernels_block_of_64_packets():
    """What the two long fixture clips are for: more than 64 packets in one launch, with DURATION packets whose second-to-last
    stamp sits on the next boundary on both sides of the refill, and AREA_COUNT counters that fire on a packet's event 0."""
    c = CASES["dur_grid_long"]
    on = [k for k, pk in enumerate(c.packets) if len(pk) >= 2 and k and pk[-2, 0] == c.start[k] + c.value]
    assert len(c.packets) > 64 and min(on) < 64 <= max(on)
    c = CASES["area_carry_long"]
    fired = [k for k in range(1, len(c.packets)) if c.frames[k] is not None and np.all(c.frames[k][0] == 0.5)
             and c.ac[k - 1].max() == c.value - 1]
    assert len(c.packets) > 64 and len(fired) >= 3


@pytest.mark.parametrize("mode", MODES)
def test_whole_run_equals_the_model_on_generated_clips(mode):
    """Seeded clips of a few packets of up to 300 events, and of 80 short packets."""
    for seed, kwargs in [(s, {}) for s in range(100, 108)] + [(s, dict(n_max=12, n_packets=80)) for s in (200, 201)]:
        kw, packets = random_packets(mode, seed, **kwargs)
        m = RendererModel(f32_time=F32_HERE, **kw)
        frames = [m.render(pk, H, W) for pk in packets]
        frames = [f for f in frames if f is not None]
        want = np.concatenate(frames) if frames else np.zeros((0, H, W))
        check_clip(lambda: renderer(mode, kw.get("value"), kw["full_scale_count"], kw.get("area_dimension")), packets, H, W, mode,
                   want, np.array(m.frame_times, dtype=np.float64), m.currentFrame, m.area_counts, m.currentFrameStartTime,
                   (mode, seed))


# ------------------------------------------------------------------------------------------------- EventFrameAccumulator
@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.family == "hist" and n.startswith("hist_source")))
def test_event_frame_accumulator_equals_the_model(name):
    """The histogram rule k_hist_events shares with the renderer: the packet accumulated twice into one running frame (the clip
    acts between the two), into bins of the output size and, from a 24x32 sensor, into the case's bins."""
    from v2e_amd.sinks import EventFrameAccumulator
    c = CASES[name]
    pk = c.packets[0]
    for sensor in (None, (H, W)):
        ranges = None if sensor is None else ((0, sensor[0]), (0, sensor[1]))
        acc = EventFrameAccumulator(c.h, c.w, c.full_scale_count, device="cuda")
        cur = np.zeros((c.h, c.w))
        for part in (pk, pk[:30], pk[30:], pk[:0]):
            got = acc.accumulate(torch.from_numpy(part.copy()).cuda(), *(sensor or (None, None)))
            cur = np.clip(cur + histogram(part, c.h, c.w, ranges), -c.full_scale_count, c.full_scale_count)
            assert same(got, cur), (name, sensor, len(part))
