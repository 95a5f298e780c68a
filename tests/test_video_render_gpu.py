"""The DVS video from the device-resident video pipeline on the MI355X: VideoToEvents.run(renderer=) and
run_stream(renderer=, chunk_pairs=) give the same frames and frame times as each other and as EventRenderer.render_run on the
events of `run`, in every exposure mode; events and counts are what they are without a renderer; on_dvs_frames gets the chunks'
frames in order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(pos_thres=0.15, neg_thres=0.15, sigma_thres=0.03, cutoff_hz=200, leak_rate_hz=0.1, shot_noise_rate_hz=2.0,
          refractory_period_s=0.001)
DT = 1 / 30.0
BS = 8  # flow chunks of 64 pairs
U = 3
H, W = 64, 96
MODES = [("DURATION", 0.05, None), ("COUNT", 3, None), ("SOURCE", None, None), ("AREA_COUNT", 12, 16)]  # COUNT / AREA_COUNT: packet / value


@pytest.fixture(scope="module")
def eng():
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import portable_unet_state_dict
    sd_f, sd_i = portable_unet_state_dict(2, 4, 401), portable_unet_state_dict(12, 5, 402)
    return SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()}, {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda")


@pytest.fixture(scope="module")
def clip():
    from v2e_amd.synth import int_gradient_frames
    return torch.from_numpy(int_gradient_frames(151, H, W, seed=3, noise=10, as_array=True)).cuda()


def _pipe(engine):
    from v2e_amd import EventEmulator
    from v2e_amd.pipeline import VideoToEvents
    return VideoToEvents(engine, EventEmulator(device="cuda", seed=5, rng_mode="philox", **KW), U, batch_size=BS)


def _renderer(mode, value, area):
    from v2e_amd.renderer import EventRenderer, ExposureMode
    return EventRenderer(full_scale_count=3, exposure_mode=ExposureMode[mode], exposure_value=value if value is not None else 1 / 300.0,
                         area_dimension=area)


def _host(ev):
    if ev is None:
        return np.zeros((0, 4), np.float32)
    return ev.cpu().numpy() if torch.is_tensor(ev) else ev


def _same(a, b):
    a, b = _host(a), _host(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope="module")
def plain(eng, clip):
    """The clip without a renderer: host events, counts, n."""
    return _pipe(eng).run(clip, DT)


@pytest.mark.parametrize("mode,value,area", MODES)
def test_run_and_run_stream_give_the_same_dvs_video(eng, clip, plain, mode, value, area):
    ref_ev, ref_counts, ref_n = plain
    assert ref_n == 450 and int(ref_counts.sum()) > 1000
    if mode in ("COUNT", "AREA_COUNT"):  # a fraction of the typical packet of BS frames, so that most packets complete frames
        value = max(2, int(np.median(ref_counts[2:].reshape(-1, BS).sum(axis=1))) // value)
    pipe = _pipe(eng)
    r_run = _renderer(mode, value, area)
    ev, counts, n = pipe.run(clip, DT, renderer=r_run)
    assert not torch.is_tensor(ev) and n == ref_n and np.array_equal(counts, ref_counts) and _same(ev, ref_ev)
    frames, times = pipe.dvs_frames, pipe.dvs_frame_times
    assert frames.is_cuda and frames.dtype == torch.float64 and tuple(frames.shape[1:]) == (H, W)
    assert len(frames) == len(times) == r_run.numFramesWritten >= 10
    print("%s: %d events, %d DVS frames" % (mode, int(ref_counts.sum()), len(frames)))

    # render_run on the events of run
    r = _renderer(mode, value, area)
    rows = torch.from_numpy(ref_ev).cuda()
    a = r.render_run(rows, ref_counts, H, W, frame0=0, batch_size=BS)
    b = r.flush_run(H, W)
    parts = [p for p in (a, b) if p[0] is not None]
    assert torch.equal(torch.cat([p[0] for p in parts]), frames) and torch.equal(torch.cat([p[1] for p in parts]), times)

    for cp, rd in ((64, False), (128, True)):
        pipe = _pipe(eng)
        rs = _renderer(mode, value, area)
        ev, counts, n = pipe.run_stream(clip, DT, chunk_pairs=cp, renderer=rs, return_device=rd)
        assert torch.is_tensor(ev) == rd and n == ref_n and np.array_equal(counts, ref_counts) and _same(ev, ref_ev)
        assert torch.equal(pipe.dvs_frames, frames) and torch.equal(pipe.dvs_frame_times, times), "chunk_pairs=%d" % cp
        assert rs.numFramesWritten == len(frames)
        assert pipe.host_syncs == rs.host_syncs <= len(range(0, 150, cp)) + 1  # at most one per chunk and one for the flush
        cur, cur_run = rs.currentFrame, r_run.currentFrame
        assert (cur is None) == (cur_run is None) and (cur is None or torch.equal(cur, cur_run))


def test_u8_video_and_the_callback(eng, clip, plain):
    ref_ev, ref_counts, ref_n = plain
    pipe = _pipe(eng)
    ev, counts, n = pipe.run(clip, DT, renderer=_renderer("DURATION", 0.05, None), dvs_u8=True, return_device=True)
    assert torch.is_tensor(ev) and _same(ev, ref_ev)
    want8, times = pipe.dvs_frames, pipe.dvs_frame_times
    assert want8.dtype == torch.uint8
    pipe = _pipe(eng)
    pipe.run(clip, DT, renderer=_renderer("DURATION", 0.05, None))
    assert torch.equal((pipe.dvs_frames * 255).to(torch.uint8), want8)

    calls = []

    def on_dvs_frames(frames, frame_times, first):
        assert frames.is_cuda and frames.dtype == torch.uint8 and len(frames) == len(frame_times) > 0
        calls.append((first, frames.clone(), frame_times.clone()))

    pipe = _pipe(eng)
    ev, counts, n = pipe.run_stream(clip, DT, chunk_pairs=64, renderer=_renderer("DURATION", 0.05, None), on_dvs_frames=on_dvs_frames,
                                    dvs_u8=True)
    torch.cuda.synchronize()
    assert _same(ev, ref_ev) and np.array_equal(counts, ref_counts)
    assert pipe.dvs_frames is None and len(calls) >= 2
    nxt = 0
    for first, fr, _ in calls:  # in order, consecutive first_frame_index
        assert first == nxt
        nxt += len(fr)
    assert nxt == len(want8)
    assert torch.equal(torch.cat([c[1] for c in calls]), want8) and torch.equal(torch.cat([c[2] for c in calls]), times)


def test_renderer_and_group_are_refused(eng, clip):
    with pytest.raises(NotImplementedError, match="multi-rank"):
        _pipe(eng).run(clip, DT, renderer=_renderer("SOURCE", None, None), group=object())


def _body(path):
    lines = open(path, "rb").read().split(b"\n")
    k = 0
    while lines[k].startswith(b"#"):
        k += 1
    return b"\n".join(lines[k:])


def test_event_files_are_unchanged_by_the_renderer(eng, tmp_path):
    """dvs_text and dvs_aedat2 sinks open (346x260, the AEDAT-2.0 layout): run and run_stream with a renderer write the bytes run
    writes without one."""
    from v2e_amd import EventEmulator
    from v2e_amd.pipeline import VideoToEvents
    from v2e_amd.synth import int_gradient_frames
    clip = torch.from_numpy(int_gradient_frames(71, 260, 346, seed=8, noise=10, as_array=True)).cuda()
    out = {}
    for name in ("plain", "run", "stream"):
        emu = EventEmulator(device="cuda", seed=5, rng_mode="philox", output_folder=str(tmp_path), dvs_aedat2=name, dvs_text=name,
                            output_width=346, output_height=260, **KW)
        pipe = VideoToEvents(eng, emu, U, batch_size=BS)
        kw = {} if name == "plain" else dict(renderer=_renderer("DURATION", 0.05, None))
        out[name] = pipe.run_stream(clip, DT, chunk_pairs=64, **kw) if name == "stream" else pipe.run(clip, DT, **kw)
        emu.cleanup()
        if name != "plain":
            assert len(pipe.dvs_frames) >= 10 and tuple(pipe.dvs_frames.shape[1:]) == (260, 346)
    n_ev = int(out["plain"][1].sum())
    for name in ("run", "stream"):
        assert np.array_equal(out[name][1], out["plain"][1]) and _same(out[name][0], out["plain"][0])
        for ext in (".aedat", ".txt"):
            a, b = _body(str(tmp_path / ("plain" + ext))), _body(str(tmp_path / (name + ext)))
            assert len(a) > 0 and a == b, (name, ext)
    assert _body(str(tmp_path / "plain.txt")).count(b"\n") == n_ev
