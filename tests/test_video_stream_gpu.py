"""VideoToEvents.run_stream on the MI355X: the clip in chunks, SloMo of the next chunk on a side stream beside the emulator's run of
the current one -- the same events, counts, frames, times and event files as VideoToEvents.run on the same clip with the same fresh
emulator, for fixed and automatic upsampling factors, device and host source frames, gathered rows and per-chunk callbacks; device
memory bounded by the chunk."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(pos_thres=0.15, neg_thres=0.15, sigma_thres=0.03, cutoff_hz=200, leak_rate_hz=0.1, shot_noise_rate_hz=2.0,
          refractory_period_s=0.001)
DT = 1 / 30.0
BS = 8  # flow chunks of 64 pairs


def _engine(head=1.0):
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import portable_unet_state_dict
    sd_f, sd_i = portable_unet_state_dict(2, 4, 401), portable_unet_state_dict(12, 5, 402)
    sd_f["conv3.weight"] = sd_f["conv3.weight"] * np.float32(head)
    sd_f["conv3.bias"] = sd_f["conv3.bias"] * np.float32(head)
    return SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()}, {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda")


@pytest.fixture(scope="module")
def eng():
    return _engine()


@pytest.fixture(scope="module")
def eng_auto():
    return _engine(25.0)


def _emu(**kw):
    from v2e_amd import EventEmulator
    return EventEmulator(device="cuda", seed=5, rng_mode="philox", **dict(KW, **kw))


def _pipe(engine, U, auto=False, **kw):
    from v2e_amd.pipeline import VideoToEvents
    return VideoToEvents(engine, _emu(**kw), U, batch_size=BS, auto_upsample=auto)


def _clip(n, H=64, W=96, seed=3):
    from v2e_amd.synth import int_gradient_frames
    return int_gradient_frames(n, H, W, seed=seed, noise=10, as_array=True)


def _host(ev):
    if ev is None:
        return np.zeros((0, 4), np.float32)
    return ev.cpu().numpy() if torch.is_tensor(ev) else ev


def _same(a, b):
    a, b = _host(a), _host(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _reference(engine, frames, U, auto=False, return_device=False):
    pipe = _pipe(engine, U, auto)
    ev, counts, n = pipe.run(torch.from_numpy(frames).cuda(), DT, return_device=return_device)
    attrs = (pipe.upsampling_factors, None if pipe.interpTimes is None else np.array(pipe.interpTimes), pipe.avg_upsampling_factor)
    return ev, counts, n, attrs


@pytest.mark.parametrize("return_device", [False, True])
def test_fixed_u_equals_run(eng, return_device):
    """150 pairs (a short last batch), U = 3: one chunk, chunks of 64 and of 128 pairs (neither divides the clip)."""
    frames = _clip(151)
    ref_ev, ref_counts, ref_n, _ = _reference(eng, frames, 3, return_device=return_device)
    assert ref_n == 450 and int(ref_counts.sum()) > 1000
    dev = torch.from_numpy(frames).cuda()
    for cp in (None, 64, 128):
        pipe = _pipe(eng, 3)
        ev, counts, n = pipe.run_stream(dev, DT, chunk_pairs=cp, return_device=return_device)
        assert torch.is_tensor(ev) == return_device
        assert n == ref_n and np.array_equal(counts, ref_counts) and _same(ev, ref_ev), "chunk_pairs=%s" % cp
        assert pipe.host_syncs == 0


def test_auto_upsample_equals_run(eng_auto):
    """The last (short) batch gets a factor of its own -- its source frames are flat grey, the flow head is scaled by 25 -- so a
    time normalisation from any other batch's factor would show in every event time."""
    frames = _clip(151)
    frames[-7:] = 128
    ref_ev, ref_counts, ref_n, (ref_f, ref_t, ref_avg) = _reference(eng_auto, frames, 2, auto=True)
    assert len(ref_f) == 19 and ref_f[-1] not in ref_f[:-1], ref_f
    print("auto factors", ref_f)
    dev = torch.from_numpy(frames).cuda()
    for cp in (None, 64, 128):
        for rd in (False, True):
            pipe = _pipe(eng_auto, 2, auto=True)
            ev, counts, n = pipe.run_stream(dev, DT, chunk_pairs=cp, return_device=rd)
            assert pipe.upsampling_factors == ref_f and pipe.avg_upsampling_factor == ref_avg
            assert np.array_equal(pipe.interpTimes.view(np.int64), ref_t.view(np.int64))
            assert n == ref_n and np.array_equal(counts, ref_counts) and _same(ev, ref_ev), "chunk_pairs=%s" % cp
            nflow = 3  # one factor read-back per flow chunk, and the last flow chunk's once more before the first run
            assert pipe.host_syncs == (nflow if cp is None else nflow + 1)


@pytest.mark.parametrize("auto", [False, True])
def test_host_frames_equal_device_frames(eng, eng_auto, auto):
    frames = _clip(151, seed=6)
    engine = eng_auto if auto else eng
    ref = _pipe(engine, 3, auto).run_stream(torch.from_numpy(frames).cuda(), DT, chunk_pairs=64)
    for src in (frames, torch.from_numpy(frames), torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 2, 1))).transpose(1, 2)):
        pipe = _pipe(engine, 3, auto)
        ev, counts, n = pipe.run_stream(src, DT, chunk_pairs=64)
        assert n == ref[2] and np.array_equal(counts, ref[1]) and _same(ev, ref[0])


@pytest.mark.parametrize("return_device", [False, True])
def test_callback_chunks_concatenate_to_run(eng, return_device):
    frames = _clip(151, seed=7)
    ref_ev, ref_counts, ref_n, _ = _reference(eng, frames, 3)
    ref_ev = _host(ref_ev)
    off = np.concatenate(([0], np.cumsum(ref_counts)))
    calls = []

    def on_events(ev, counts, frame0):
        assert torch.is_tensor(ev) == return_device or ev is None
        k = len(counts)
        rows = _host(ev).copy()  # (device rows read while the callback runs: the buffer set is reused afterwards)
        assert np.array_equal(rows.view(np.int32), ref_ev[off[frame0]:off[frame0 + k]].view(np.int32))
        calls.append((frame0, k, rows, np.array(counts)))

    pipe = _pipe(eng, 3)
    ev, counts, n = pipe.run_stream(torch.from_numpy(frames).cuda(), DT, chunk_pairs=64, on_events=on_events,
                                    return_device=return_device)
    assert ev is None and n == ref_n and np.array_equal(counts, ref_counts)
    assert [c[0] for c in calls] == [0, 192, 384] and [c[1] for c in calls] == [192, 192, 66]
    assert np.array_equal(np.concatenate([c[2] for c in calls]), ref_ev)
    assert np.array_equal(np.concatenate([c[3] for c in calls]), ref_counts)


def _renderer():
    from v2e_amd.renderer import EventRenderer, ExposureMode
    return EventRenderer(full_scale_count=3, exposure_mode=ExposureMode.DURATION, exposure_value=0.05)


@pytest.mark.parametrize("first", ["host_rows", "device_rows_rendered"])
def test_two_calls_on_one_pipeline_equal_fresh_pipelines(eng, first):
    """One VideoToEvents object, two run_stream calls that need different streams (host numpy frames and rows on the host: the
    copy-out stream; device frames, a renderer and device rows: the render stream), in either order: each call gives what it gives
    on a fresh pipeline -- the streams are created on first need and reused.  Every call gets a fresh emulator of the same seed."""
    frames = _clip(151, seed=12)
    dev = torch.from_numpy(frames).cuda()

    def host_rows(pipe):
        return pipe.run_stream(frames, DT, chunk_pairs=64), None, None

    def device_rows_rendered(pipe):
        r = pipe.run_stream(dev, DT, chunk_pairs=64, renderer=_renderer(), return_device=True)
        return r, pipe.dvs_frames, pipe.dvs_frame_times

    calls = [host_rows, device_rows_rendered] if first == "host_rows" else [device_rows_rendered, host_rows]
    one = _pipe(eng, 3)
    for call in calls:
        one.emu = _emu()
        (ev, counts, n), dvs, dvs_t = call(one)
        (ref_ev, ref_counts, ref_n), ref_dvs, ref_dvs_t = call(_pipe(eng, 3))
        assert ref_n == 450 and int(ref_counts.sum()) > 1000
        assert torch.is_tensor(ev) == torch.is_tensor(ref_ev) == (call is device_rows_rendered)
        assert n == ref_n and np.array_equal(counts, ref_counts) and _same(ev, ref_ev), call.__name__
        if call is device_rows_rendered:
            assert len(ref_dvs) == len(ref_dvs_t) >= 10
            assert torch.equal(dvs, ref_dvs) and torch.equal(dvs_t, ref_dvs_t)
        else:
            assert one.dvs_frames is None and one.dvs_frame_times is None


def _body(path, text):
    data = open(path, "rb").read()
    if text:
        lines = data.split(b"\n")
        k = 0
        while lines[k].startswith(b"#"):
            k += 1
        return b"\n".join(lines[k:])
    pos = 0
    while data[pos:pos + 1] == b"#":
        pos = data.index(b"\r\n", pos) + 2
    return data[pos:]


def test_event_files_equal_run(eng, tmp_path):
    frames = _clip(71, 260, 346, seed=8)
    out = {}
    for name in ("run", "stream"):
        pipe = _pipe(eng, 2, output_folder=str(tmp_path), dvs_aedat2=name, dvs_text=name, output_width=346, output_height=260)
        dev = torch.from_numpy(frames).cuda()
        r = pipe.run(dev, DT) if name == "run" else pipe.run_stream(dev, DT, chunk_pairs=64)
        pipe.emu.cleanup()
        out[name] = r
    assert np.array_equal(out["run"][1], out["stream"][1]) and _same(out["run"][0], out["stream"][0])
    n_ev = int(out["run"][1].sum())
    assert n_ev > 1000
    for text, ext in ((False, ".aedat"), (True, ".txt")):
        a, b = _body(str(tmp_path / ("run" + ext)), text), _body(str(tmp_path / ("stream" + ext)), text)
        assert len(a) > 0 and a == b
    assert _body(str(tmp_path / "run.txt"), True).count(b"\n") == n_ev


def test_h5_file_equals_run(eng, tmp_path):
    h5py = pytest.importorskip("h5py")
    frames = _clip(71, seed=9)
    for name in ("run", "stream"):
        pipe = _pipe(eng, 2, output_folder=str(tmp_path), dvs_h5=name)
        dev = torch.from_numpy(frames).cuda()
        pipe.run(dev, DT) if name == "run" else pipe.run_stream(dev, DT, chunk_pairs=64)
        pipe.emu.cleanup()
    with h5py.File(str(tmp_path / "run.h5"), "r") as a, h5py.File(str(tmp_path / "stream.h5"), "r") as b:
        assert sorted(a.keys()) == sorted(b.keys())
        for k in a.keys():
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def _peak(fn):
    import gc
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_device_memory_is_bounded_by_the_chunk(eng):
    """Host source frames, host rows: 2 and 8 chunks of 64 pairs at the same chunk size use the same device memory; run() grows."""
    short, long_ = _clip(129, seed=10), _clip(513, seed=10)
    _pipe(eng, 2).run_stream(short, DT, chunk_pairs=64)  # warm-up: workspaces, resampler tables

    def stream(frames):
        pipe = _pipe(eng, 2)
        _, counts, n = pipe.run_stream(frames, DT, chunk_pairs=64)
        assert n == 2 * (len(frames) - 1)
        del pipe

    p2, p8 = _peak(lambda: stream(short)), _peak(lambda: stream(long_))
    p_run = _peak(lambda: _pipe(eng, 2).run(torch.from_numpy(long_).cuda(), DT))
    print("peak device memory: run_stream 2 chunks %.1f MB, 8 chunks %.1f MB; run 8 chunks' clip %.1f MB"
          % (p2 / 1e6, p8 / 1e6, p_run / 1e6))
    assert p8 <= 1.1 * p2
    assert p_run > p8


def test_clip_beyond_the_run_capacity(eng):
    """cap below the clip's events but above every chunk's: run() on the whole clip raises the capacity error, run_stream completes
    with the events of a run() with the emulator's own capacity."""
    from v2e_amd._capi import V2EAmdError
    frames = _clip(151, seed=11)
    ref_ev, ref_counts, ref_n, _ = _reference(eng, frames, 3)
    per_chunk = [int(ref_counts[a * 3:b * 3].sum()) for a, b in ((0, 64), (64, 128), (128, 150))]
    cap = max(per_chunk) + 16
    assert int(ref_counts.sum()) > max(cap, 1024)
    small = _pipe(eng, 3)
    batch = small.emu.generate_events_batch
    small.emu.generate_events_batch = lambda f, t, **k: batch(f, t, cap=cap, **k)
    with pytest.raises(V2EAmdError, match="capacity"):
        small.run(torch.from_numpy(frames).cuda(), DT)
    pipe = _pipe(eng, 3)
    ev, counts, n = pipe.run_stream(torch.from_numpy(frames).cuda(), DT, chunk_pairs=64, cap=cap)
    assert n == ref_n and np.array_equal(counts, ref_counts) and _same(ev, ref_ev)
