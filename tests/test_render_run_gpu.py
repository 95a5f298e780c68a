"""EventRenderer.render_run / flush_run on the MI355X against the reference's own DVS video (tests/golden/render_run.npz,
recorded by tests/golden/make_golden_render_run.py from v2ecore's EventRenderer driven by v2e.py's loop): frames, the frame
left behind and the frame-times file, bit for bit and byte for byte, as one run and split into runs at arbitrary frames; and
at sensor size against a loop of the per-packet call, which tests/test_sinks.py pins to the reference."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_run.npz")
VIDEO = "dvs-video.avi"
SPLITS = {1: [0, 120], 2: [0, 47, 120], 5: [0, 1, 26, 64, 65, 120]}  # 64 flushes a packet at batch 8, 65 at batch 5


def _cases():
    z = np.load(GOLDEN)
    return sorted(k[:-len("_packets")] for k in z.keys() if k.endswith("_packets"))


def _renderer(case):
    from v2e_amd.renderer import EventRenderer, ExposureMode
    m = re.match(r"(duration|count|source|area_count)_(\w+?)_b(\d+)_(\d+)x(\d+)$", case)
    mode, val, bs, h, w = m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))
    em = {"duration": ExposureMode.DURATION, "count": ExposureMode.COUNT, "source": ExposureMode.SOURCE,
          "area_count": ExposureMode.AREA_COUNT}[mode]
    value = {"0p0003": 300e-6, "0p001": 1e-3, "50": 50, "6": 6, "none": 1 / 300.0}[val]
    r = EventRenderer(full_scale_count=3, exposure_mode=em, exposure_value=value, area_dimension=16 if mode == "area_count" else None)
    return r, bs, h, w


def _golden_frames(z, case):
    n = len(z[case + "_packets"])
    return np.concatenate([z[case + "_p%d" % k] for k in range(n) if case + "_p%d" % k in z])


def _render_clip(r, rows, counts, h, w, bs, cuts, **kw):
    """render_run over the runs [cuts[k], cuts[k + 1]) of emulator frames, then flush_run: (frames, times) on the host."""
    off = np.concatenate(([0], np.cumsum(counts)))
    frames, times = [], []
    for a, b in zip(cuts, cuts[1:]):
        fr, t = r.render_run(rows[off[a]:off[b]], counts[a:b], h, w, frame0=a, batch_size=bs, **kw)
        assert (fr is None) == (t is None)
        if fr is not None:
            assert fr.is_cuda and t.is_cuda and t.dtype == torch.float64 and len(fr) == len(t)
            frames.append(fr)
            times.append(t)
    fr, t = r.flush_run(h, w, **kw)
    if fr is not None:
        frames.append(fr)
        times.append(t)
    assert r.flush_run(h, w, **kw) == (None, None)  # nothing pending any more
    return torch.cat(frames).cpu().numpy(), torch.cat(times).cpu().numpy()


@pytest.mark.parametrize("n_runs", sorted(SPLITS))
@pytest.mark.parametrize("case", _cases())
def test_render_run_equals_the_reference_video(case, n_runs):
    from v2e_amd.renderer import frame_times_text
    z = np.load(GOLDEN)
    counts, rows = z["counts"], torch.from_numpy(z["rows"]).cuda()
    want = _golden_frames(z, case)
    r, bs, h, w = _renderer(case)
    frames, times = _render_clip(r, rows, counts, h, w, bs, SPLITS[n_runs])
    assert frames.dtype == np.float64 and frames.shape == want.shape
    assert np.array_equal(frames.view(np.int64), want.view(np.int64))
    assert r.numFramesWritten == len(want)
    if case + "_cur" in z:
        cur = r.currentFrame.cpu().numpy()
        assert cur.dtype == np.float64 and np.array_equal(cur.view(np.int64), z[case + "_cur"].view(np.int64))
    else:
        assert r.currentFrame is None
    assert frame_times_text(VIDEO, times).encode() == z[case + "_txt"].tobytes()
    assert np.array_equal(times.view(np.int64), z[case + "_times"].view(np.int64))  # (and the value behind every line)


@pytest.mark.parametrize("case", _cases())
def test_u8_frames_are_the_bytes_of_the_avi_writer(case):
    z = np.load(GOLDEN)
    counts, rows = z["counts"], torch.from_numpy(z["rows"]).cuda()
    want = (_golden_frames(z, case) * 255).astype(np.uint8)  # renderer.py:339
    r, bs, h, w = _renderer(case)
    frames, _ = _render_clip(r, rows, counts, h, w, bs, SPLITS[2], as_u8=True)
    assert frames.dtype == np.uint8 and np.array_equal(frames, want)


@pytest.mark.parametrize("case", _cases())
def test_without_frames_the_state_still_advances(case):
    """return_frames=False: no frames, the same times, frame count and frame left behind."""
    z = np.load(GOLDEN)
    counts, rows = z["counts"], torch.from_numpy(z["rows"]).cuda()
    off = np.concatenate(([0], np.cumsum(counts)))
    r, bs, h, w = _renderer(case)
    times = []
    for a, b in zip(SPLITS[2], SPLITS[2][1:]):
        fr, t = r.render_run(rows[off[a]:off[b]], counts[a:b], h, w, frame0=a, batch_size=bs, return_frames=False)
        assert fr is None
        times += [] if t is None else [t]
    fr, t = r.flush_run(h, w, return_frames=False)
    assert fr is None
    times += [] if t is None else [t]
    assert np.array_equal(torch.cat(times).cpu().numpy().view(np.int64), z[case + "_times"].view(np.int64))
    assert r.numFramesWritten == len(z[case + "_times"])
    if case + "_cur" in z:
        assert np.array_equal(r.currentFrame.cpu().numpy(), z[case + "_cur"])


class _ReadBacks:
    """Counts the device-to-host reads torch offers (.item / .tolist / .cpu / .numpy on device tensors) while active."""

    def __enter__(self):
        self.n, self.saved = 0, {}
        for name in ("item", "tolist", "cpu", "numpy"):
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def wrapped(t, *a, _orig=orig, **k):
                if t.is_cuda:
                    self.n += 1
                return _orig(t, *a, **k)

            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


@pytest.mark.parametrize("case", [c for c in _cases() if c.endswith("_b8_64x64")])
def test_at_most_one_read_back_per_run(case):
    z = np.load(GOLDEN)
    counts, rows = z["counts"], torch.from_numpy(z["rows"]).cuda()
    off = np.concatenate(([0], np.cumsum(counts)))
    r, bs, h, w = _renderer(case)
    cuts = SPLITS[5]
    for a, b in zip(cuts, cuts[1:]):
        before = r.host_syncs
        with _ReadBacks() as rb:
            r.render_run(rows[off[a]:off[b]], counts[a:b], h, w, frame0=a, batch_size=bs)
        assert rb.n <= 1 and r.host_syncs - before == rb.n, (case, a, b, rb.n)
        if case.startswith(("count", "source")):
            assert rb.n == 0
    with _ReadBacks() as rb:
        r.flush_run(h, w)
    assert rb.n <= 1


def test_duration_that_does_not_advance_is_refused():
    """Time stamps near 4e6 s: a 1 us exposure is below half a float32 ulp there.  Where numpy keeps `currentFrameStartTime`
    float32 the frame time cannot advance and the run is refused, as the per-packet call refuses it; nothing is committed.
    An instance that renders runs refuses per-packet calls."""
    from v2e_amd.renderer import EventRenderer, ExposureMode
    ev = np.zeros((6, 4), np.float32)
    ev[:, 0] = np.float32(4e6) + np.arange(6, dtype=np.float32) * np.float32(1e-5)  # (all the same float32)
    ev[4:, 0] = np.float32(4e6) + np.float32(1)
    ev[:, 3] = 1
    r = EventRenderer(exposure_mode=ExposureMode.DURATION, exposure_value=1e-6)
    dev = torch.from_numpy(ev).cuda()
    assert r.render_run(dev[:2], [0, 2], 8, 8, frame0=0, batch_size=8) == (None, None)  # frame 1 does not flush: two rows pending
    with pytest.raises(RuntimeError, match="pending"):
        r.render_events_to_frames(ev, 8, 8)
    if type(np.float32(0) + 0.5) is np.float32:
        with pytest.raises(ValueError, match="does not advance"):
            r.render_run(dev[2:], [0, 0, 0, 0, 0, 0, 4], 8, 8, frame0=2, batch_size=8)  # frame 8 flushes all six rows
        assert r.numFramesWritten == 0 and float(r._time_state[1].item()) == 0.0 and r.currentFrameStartTime is None
        assert r._pend_rows is not None and torch.equal(r._pend_rows, dev[:2])  # the refused run consumed nothing
        return
    fr, t = r.render_run(dev[2:], [0, 0, 0, 0, 0, 0, 4], 8, 8, frame0=2, batch_size=8, return_frames=False)
    assert r.numFramesWritten == len(t) > 0  # this numpy promotes the frame start time to float64: the exposure advances it


@pytest.mark.parametrize("case", [c for c in _cases() if c.endswith("_b8_64x64") and not c.startswith("count")])  # (no packet holds 50 events)
def test_more_packets_than_one_block_of_the_window_kernel(case):
    """batch_size 1 on the 120-frame fixture: 115 packets, so the DURATION window kernel refills its 64-packet LDS block; against
    the per-packet loop over the same packets.  The per-packet call then follows the run on the same instance."""
    from v2e_amd.renderer import run_packets
    z = np.load(GOLDEN)
    counts, rows = z["counts"], torch.from_numpy(z["rows"]).cuda()
    packets, pending = run_packets(counts, 0, 1)
    assert len(packets) == 115 and pending == 0 and int(packets[-1, 1]) == len(rows)
    loop, _, h, w = _renderer(case)
    want = [loop.render_events_to_frames(rows[a:b], h, w, return_frames=True) for a, b in packets.tolist()]
    want = np.concatenate([f for f in want if f is not None])
    run, _, _, _ = _renderer(case)
    frames, times = _render_clip(run, rows, counts, h, w, 1, [0, 120])
    assert len(want) >= 10 and frames.shape == want.shape and np.array_equal(frames.view(np.int64), want.view(np.int64))
    assert len(times) == len(want)
    if case.startswith("duration"):
        assert type(run.currentFrameStartTime) is type(loop.currentFrameStartTime)
        assert float(run.currentFrameStartTime) == float(loop.currentFrameStartTime)
    # one more packet through the per-packet call on both instances: the run left the state the loop left
    extra = rows[:60].clone()
    extra[:, 0] += 0.02
    a = run.render_events_to_frames(extra, h, w, return_frames=True)
    b = loop.render_events_to_frames(extra, h, w, return_frames=True)
    assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    assert (run.currentFrame is None) == (loop.currentFrame is None)
    if run.currentFrame is not None:
        assert torch.equal(run.currentFrame, loop.currentFrame)


KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=300, leak_rate_hz=0.01, shot_noise_rate_hz=0.001,
          refractory_period_s=0.0005)


@pytest.fixture(scope="module")
def sensor_run():
    """346x260, Philox, the `noisy` preset, 84 frames at 1/300 s (about 13 k events a frame): device rows and per-frame counts."""
    from v2e_amd import EventEmulator
    from v2e_amd.synth import int_gradient_frames
    frames = int_gradient_frames(84, 260, 346, seed=1, noise=10, as_array=True)
    emu = EventEmulator(device="cuda", seed=8, rng_mode="philox", **KW)
    emu.set_dvs_params("noisy")
    ev, counts = emu.generate_events_batch(frames, [i / 300 for i in range(84)], return_device=True)
    return ev.clone(), np.asarray(counts)


@pytest.mark.parametrize("mode,value,area", [("DURATION", 1 / 300.0, None), ("DURATION", 2.5e-3, None), ("COUNT", 20000, None),
                                             ("SOURCE", None, None), ("AREA_COUNT", 400, 32)])
def test_sensor_size_run_equals_the_per_packet_loop(sensor_run, mode, value, area):
    from v2e_amd.renderer import EventRenderer, ExposureMode, run_packets
    ev, counts = sensor_run
    assert int(counts.sum()) >= 1_000_000, int(counts.sum())
    kw = dict(full_scale_count=3, exposure_mode=ExposureMode[mode], exposure_value=value if value is not None else 1 / 300.0,
              area_dimension=area)
    h, w, bs = 260, 346, 8
    packets, _ = run_packets(counts, 0, bs)
    ranges = [tuple(p) for p in packets.tolist()] + [(int(packets[-1, 1]), int(counts.sum()))]
    loop = EventRenderer(**kw)
    want = [loop.render_events_to_frames(ev[a:b], h, w, return_frames=True) for a, b in ranges if b > a]
    want = np.concatenate([f for f in want if f is not None])
    run = EventRenderer(**kw)
    frames, times = _render_clip(run, ev, counts, h, w, bs, [0, 23, 84])
    print("%s: %d events, %d packets, %d frames" % (mode, int(counts.sum()), len(ranges), len(want)))
    assert len(want) >= 5 and frames.shape == want.shape and np.array_equal(frames.view(np.int64), want.view(np.int64))
    assert len(times) == len(want) and np.all(np.diff(times) >= 0)
    cur, cur_loop = run.currentFrame, loop.currentFrame
    assert (cur is None) == (cur_loop is None)
    if cur is not None:
        assert torch.equal(cur, cur_loop)
    if mode == "AREA_COUNT":
        assert torch.equal(run.area_counts, loop.area_counts)
    if mode == "DURATION":  # the start time carried on the device is the one the per-packet class holds on the host
        assert float(run._time_state[0].item()) == float(loop.currentFrameStartTime)
