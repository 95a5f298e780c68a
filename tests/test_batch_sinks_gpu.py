"""GPU: device-resident runs (generate_events_batch, generate_events_batch_async, VideoToEvents.run) feed the emulator's open
event files -- the same bytes after the header as a twin emulator fed the same frames through per-frame generate_events, the
path tests/test_sinks.py pins to the reference's writers."""
import os

import numpy as np
import pytest

KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=200, leak_rate_hz=0.1, shot_noise_rate_hz=5.0,
          refractory_period_s=0.0005, output_width=346, output_height=260)


def clip(n=13, seed=4):
    from v2e_amd.synth import int_gradient_frames
    return int_gradient_frames(n, 260, 346, seed=seed, noise=10, as_array=True), [i / 300 for i in range(n)]


class RecordingWriter:
    """A caller-supplied dvs_aedat4 writer object: records what it is given."""

    def __init__(self):
        self.rows, self.labels, self.closed = [], [], 0

    def appendEvents(self, events, signnoise_label=None):
        self.rows.append(np.array(events, copy=True))
        self.labels.append(None if signnoise_label is None else np.array(signnoise_label, copy=True))

    def close(self):
        self.closed += 1

    def all(self):
        rows = np.concatenate(self.rows) if self.rows else np.zeros((0, 4), np.float32)
        labs = [l for l in self.labels if l is not None]
        return rows, (np.concatenate(labs) if labs else None), len(labs) == len(self.labels)


def body(path, text):
    data = open(path, "rb").read()
    if text:
        lines = data.split(b"\n")
        k = 0
        while lines[k].startswith(b"#"):
            k += 1
        return b"\n".join(lines[k:])
    # AEDAT-2.0: header lines start with '#' and end in CRLF; the first event never starts with '#' (the writer drops those)
    pos = 0
    while data[pos:pos + 1] == b"#":
        pos = data.index(b"\r\n", pos) + 2
    return data[pos:]


def emulator(tmp, name, label, aedat4=None):
    from v2e_amd import EventEmulator
    return EventEmulator(device="cuda", seed=7, rng_mode="philox", output_folder=str(tmp), dvs_aedat2=name, dvs_text=name,
                         dvs_aedat4=aedat4, label_signal_noise=label, **KW)


def twin_files(tmp, frames, times, label):
    w = RecordingWriter()
    emu = emulator(tmp, "twin", label, w)
    evs = [emu.generate_events(f, t) for f, t in zip(frames, times)]
    counters = (emu.dvs_aedat2.numEventsWritten, emu.dvs_aedat2.numOnEvents, emu.dvs_aedat2.numOffEvents,
                emu.dvs_text.numEventsWritten)
    emu.cleanup()
    allev = np.concatenate([e for e in evs if e is not None])
    return allev, body(str(tmp / "twin.aedat"), False), body(str(tmp / "twin.txt"), True), w, counters


def assert_same_files(tmp, name, twin, w=None, counters=None):
    allev, aed, txt, tw, tcount = twin
    assert len(aed) == 8 * len(allev) or len(aed) < 8 * len(allev)  # (leading '#' events dropped, as the writer does)
    assert body(str(tmp / (name + ".aedat")), False) == aed
    assert body(str(tmp / (name + ".txt")), True) == txt
    assert txt.count(b"\n") == len(allev)
    if counters is not None:
        assert counters == tcount
    if w is not None:
        r0, l0, all0 = tw.all()
        r1, l1, all1 = w.all()
        assert np.array_equal(r0, r1) and all0 == all1
        assert (l0 is None and l1 is None) or np.array_equal(l0, l1)


@pytest.mark.gpu
@pytest.mark.parametrize("label", [True, False])
def test_batch_runs_write_the_files_of_the_per_frame_path(tmp_path, label):
    frames, times = clip()
    twin = twin_files(tmp_path, frames, times, label)
    w = RecordingWriter()
    emu = emulator(tmp_path, "batch", label, w)
    got = []
    for a, b in ((0, 5), (5, 9), (9, 13)):  # three runs, the first one with the initial frame
        ev, _ = emu.generate_events_batch(frames[a:b], times[a:b])
        if ev is not None:
            got.append(ev)
    counters = (emu.dvs_aedat2.numEventsWritten, emu.dvs_aedat2.numOnEvents, emu.dvs_aedat2.numOffEvents,
                emu.dvs_text.numEventsWritten)
    emu.cleanup()
    assert np.array_equal(np.concatenate(got), twin[0])
    assert_same_files(tmp_path, "batch", twin, w, counters)
    assert w.closed == 1


@pytest.mark.gpu
@pytest.mark.parametrize("label", [True, False])
def test_pipelined_runs_out_of_order_and_dropped_reach_the_files_in_order(tmp_path, label):
    """generate_events_batch_async in the pipelined mode: results read out of order, one handle dropped unread (its buffer set
    reused by a later run), the last ones left to cleanup()."""
    frames, times = clip(17)
    twin = twin_files(tmp_path, frames, times, label)
    w = RecordingWriter()
    emu = emulator(tmp_path, "pipe", label, w)
    cuts = [(0, 4), (4, 7), (7, 10), (10, 13), (13, 15), (15, 17)]
    h = [emu.generate_events_batch_async(frames[a:b], times[a:b], use_graph=0) for a, b in cuts[:2]]
    r1 = h[1].result()  # out of order: run 0 is written first
    r0 = h[0].result()
    h2 = emu.generate_events_batch_async(frames[7:10], times[7:10], use_graph=0)
    del h2  # dropped unread: held for the files
    h3 = emu.generate_events_batch_async(frames[10:13], times[10:13], use_graph=0)
    h4 = emu.generate_events_batch_async(frames[13:15], times[13:15], use_graph=0)  # reuses run 2's buffer set: writes it
    h5 = emu.generate_events_batch_async(frames[15:17], times[15:17], use_graph=0)
    r4 = h4.result()
    del h3, h5  # left to cleanup()
    emu.cleanup()
    assert r0[0] is not None and r1[0] is not None and r4[0] is not None
    assert_same_files(tmp_path, "pipe", twin, w)


@pytest.mark.gpu
def test_no_sink_no_held_runs():
    from v2e_amd import EventEmulator
    frames, times = clip(6)
    emu = EventEmulator(device="cuda", seed=7, rng_mode="philox", **KW)
    h = emu.generate_events_batch_async(frames[:3], times[:3], use_graph=0)
    assert not emu.__dict__.get("_sink_runs")
    h.result()
    emu.cleanup()


@pytest.mark.gpu
def test_video_to_events_writes_the_events_it_returns(tmp_path):
    import torch
    from v2e_amd import EventEmulator
    from v2e_amd.pipeline import VideoToEvents
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import int_gradient_frames, portable_unet_state_dict
    sd_f, sd_i = portable_unet_state_dict(2, 4, 201), portable_unet_state_dict(12, 5, 202)
    eng = SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()}, {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda:0")
    emu = EventEmulator(device="cuda", seed=5, rng_mode="philox", output_folder=str(tmp_path), dvs_text="v2e", dvs_aedat2="v2e",
                        label_signal_noise=True, **KW)
    pipe = VideoToEvents(eng, emu, 3, batch_size=2)
    fr = int_gradient_frames(4, 260, 346, seed=9, noise=8, as_array=True)
    ev, counts, n = pipe.run(torch.from_numpy(fr).cuda(), 1 / 30)
    emu.cleanup()
    assert ev is not None and len(ev) > 1000 and int(counts.sum()) == len(ev)
    rows = body(str(tmp_path / "v2e.txt"), True).split(b"\n")[:-1]
    assert len(rows) == len(ev)
    for i in np.linspace(0, len(ev) - 1, 200).astype(int):
        t, x, y, p, _ = rows[i].split()
        assert t.decode() == '{}'.format(np.float64(ev[i, 0])) and int(x) == int(ev[i, 1]) and int(y) == int(ev[i, 2])
        assert int(p) == int((ev[i, 3] + 1) / 2)
    words = np.frombuffer(body(str(tmp_path / "v2e.aedat"), False), dtype=">i4").reshape(-1, 2)
    tail = min(len(words), len(ev))
    assert np.array_equal(words[-tail:, 1], (np.float32(1e6) * ev[-tail:, 0]).astype(np.int32))


@pytest.mark.gpu
def test_hdf5_rows_and_frame_index_of_batch_runs(tmp_path):
    h5py = pytest.importorskip("h5py")
    frames, times = clip(9)
    from v2e_amd import EventEmulator
    out = {}
    for name, batch in (("pf", False), ("bt", True)):
        emu = EventEmulator(device="cuda", seed=7, rng_mode="philox", output_folder=str(tmp_path), dvs_h5=name, **KW)
        emu.prepare_storage(len(frames), times)
        if batch:
            emu.generate_events_batch(frames[:4], times[:4])
            emu.generate_events_batch(frames[4:], times[4:])
        else:
            for f, t in zip(frames, times):
                emu.generate_events(f, t)
        emu.cleanup()
        with h5py.File(str(tmp_path / (name + ".h5")), "r") as f:
            out[name] = {k: f[k][()] for k in ("events", "frame_idx", "frame", "frame_ts")}
    for k in out["pf"]:
        assert np.array_equal(out["pf"][k], out["bt"][k]), k


def small_clip(n, H, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, size=(n, H, W)).astype(np.uint8), [i / 300 for i in range(n)]


def text_emulator(tmp, name, **kw):
    from v2e_amd import EventEmulator
    kw = dict({k: v for k, v in KW.items() if not k.startswith("output_")}, **kw)
    return EventEmulator(device="cuda", seed=7, rng_mode="philox", output_folder=str(tmp), dvs_text=name, **kw)


@pytest.mark.gpu
def test_cleanup_drops_the_held_runs_of_a_failed_instance(tmp_path, caplog):
    """Three runs left to cleanup() with a text file open, the second one with too small an event buffer: the first run's rows
    reach the file (what the per-frame path writes for its frames), the failed run and the one after it are dropped with one
    error line, the file is closed, and the instance refuses frames until reset()."""
    from v2e_amd import V2EAmdError
    frames, times = small_clip(8, 37, 91, seed=3)
    twin = text_emulator(tmp_path, "twin")
    for f, t in zip(frames[:4], times[:4]):
        twin.generate_events(f, t)
    twin.cleanup()
    emu = text_emulator(tmp_path, "fail")
    emu.generate_events_batch_async(frames[:4], times[:4], use_graph=0, pipelined=False)
    emu.generate_events_batch_async(frames[4:6], times[4:6], use_graph=0, pipelined=False, cap=1024)  # a fresh buffer set: 1 024 rows
    emu.generate_events_batch_async(frames[6:], times[6:], use_graph=0, pipelined=False)  # (reuses the first run's set: written)
    assert len(emu.__dict__["_sink_runs"]) == 2
    text = emu.dvs_text
    emu.cleanup()
    errors = [r.getMessage() for r in caplog.records if r.levelname == "ERROR"]
    assert len(errors) == 1 and "2 enqueued run(s) not written to the event files" in errors[0] and "capacity" in errors[0]
    assert emu.dvs_text is None and not emu.__dict__["_sink_runs"] and text.file is None
    want = body(str(tmp_path / "twin.txt"), True)
    assert want.count(b"\n") > 1024 and body(str(tmp_path / "fail.txt"), True) == want
    with pytest.raises(V2EAmdError, match="reset"):
        emu.generate_events(frames[-1], times[-1] + 0.01)


@pytest.mark.gpu
def test_cleanup_twice_does_the_work_once(tmp_path, caplog):
    """A centre-surround run left to cleanup(): the first call writes it, reports the CSDVS step statistics and closes the file
    (the per-frame path's file); the second call logs nothing and touches no file."""
    import logging
    from v2e_amd.synth import int_gradient_frames
    frames, times = int_gradient_frames(7, 8, 70, seed=71, noise=8, as_array=True), [i / 250 for i in range(7)]
    cs = dict(cutoff_hz=300, cs_lambda_pixels=2.5, cs_tau_p_ms=3.0)
    twin = text_emulator(tmp_path, "twin", **cs)
    for f, t in zip(frames, times):
        twin.generate_events(f, t)
    twin.cleanup()
    emu = text_emulator(tmp_path, "cs", **cs)
    emu.generate_events_batch_async(frames, times, use_graph=0, pipelined=False)
    path = str(tmp_path / "cs.txt")
    with caplog.at_level(logging.INFO, logger="v2e_amd.emulator"):
        emu.cleanup()
        first, stamp, logged = open(path, "rb").read(), os.stat(path).st_mtime_ns, len(caplog.records)
        emu.cleanup()
    assert len(caplog.records) == logged and os.stat(path).st_mtime_ns == stamp and open(path, "rb").read() == first
    assert sum("CSDVS steps statistics" in r.getMessage() for r in caplog.records) == 1
    assert body(path, True) == body(str(tmp_path / "twin.txt"), True) and body(path, True).count(b"\n") > 0
