"""Event-sink integer formats: the HIP packers against bytes produced by the
reference's own AEDAT-2.0 writer and its HDF5 conversion lines (tests/golden/make_golden_sinks.py)."""
import os

import numpy as np
import pytest

from fixtures import GOLDEN


def test_golden_is_consistent_with_documented_rules():
    """CPU: restate aedat2_output.py:155-173 / emulator.py:957-960 in numpy and compare with the recorded bytes."""
    z = np.load(os.path.join(GOLDEN, "sinks.npz"))
    for (w, h, xs, ys, ps) in ((346, 260, 12, 22, 11), (640, 480, 1, 11, 0)):
        ev = z["ev_%dx%d" % (w, h)]
        t = (1e6 * ev[:, 0]).astype(np.int32)
        x = (w - 1) - ev[:, 1].astype(np.int32)
        y = (h - 1) - ev[:, 2].astype(np.int32)
        p = ((ev[:, 3] + 1) / 2).astype(np.int32)
        a = (x << xs | y << ys | p << ps)
        a[4000:] |= 1 << 10
        out = np.empty(2 * len(ev), np.int32)
        out[0::2], out[1::2] = a, t
        assert np.array_equal(np.frombuffer(out.byteswap().tobytes(), np.uint8), z["aedat2_%dx%d" % (w, h)])


@pytest.mark.gpu
def test_hip_packers_match_reference_writer_bytes():
    import torch
    from v2e_amd.sinks import pack_aedat2, pack_h5
    z = np.load(os.path.join(GOLDEN, "sinks.npz"))
    for (w, h) in ((346, 260), (640, 480)):
        ev = torch.from_numpy(z["ev_%dx%d" % (w, h)]).cuda()
        got = pack_aedat2(ev, w, h, noise_from=4000).cpu().numpy()
        assert np.array_equal(got, z["aedat2_%dx%d" % (w, h)])
        h5 = pack_h5(ev).cpu().numpy().view(np.uint32)
        assert np.array_equal(h5, z["h5_%dx%d" % (w, h)])
    with pytest.raises(ValueError):
        pack_aedat2(ev, 100, 100)


@pytest.mark.gpu
def test_event_frame_accumulator_matches_renderer_math():
    """renderer.py:368-400 restated with numpy (hist2d_numba_seq semantics), incl. down-scaled output bins."""
    import torch
    from v2e_amd.sinks import EventFrameAccumulator
    z = np.load(os.path.join(GOLDEN, "sinks.npz"))
    ev = z["ev_346x260"]
    for (bh, bw) in ((260, 346), (130, 173)):
        acc = EventFrameAccumulator(bh, bw, full_scale_count=3, device="cuda")
        cur = np.zeros((bh, bw))
        for sl in (slice(0, 2000), slice(2000, 5000)):
            e = ev[sl]
            got = acc.accumulate(torch.from_numpy(e).cuda(), 260, 346).cpu().numpy()
            on = e[:, 3] == 1
            H = np.zeros((bh, bw))
            for pol, sgn in ((on, 1), (~on, -1)):
                i = (e[pol, 2].astype(np.float64) - 0) * (1 / ((260 - 0) / bh))
                j = (e[pol, 1].astype(np.float64) - 0) * (1 / ((346 - 0) / bw))
                ok = (i >= 0) & (i < bh) & (j >= 0) & (j < bw)
                np.add.at(H, (i[ok].astype(int), j[ok].astype(int)), sgn)
            cur = np.clip(cur + H, -3, 3)
            assert np.array_equal(got, cur)


RENDER_CASES = [("duration", 0.5, None), ("duration", 2.0, None), ("count", 700, None), ("source", None, None), ("area_count", 40, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("as_tensor", [False, True])
@pytest.mark.parametrize("case", RENDER_CASES)
def test_event_renderer_matches_reference(case, as_tensor):
    """v2e_amd.EventRenderer against frames produced by the reference's EventRenderer.render_events_to_frames
    (tests/golden/make_golden_renderer.py): three packets, every exposure mode, sensor resolution and down-scaled;
    float64 frames bit-equal, as is the accumulator left behind after each run."""
    import torch
    from v2e_amd.renderer import EventRenderer, ExposureMode
    mode, val, area = case
    modes = {"duration": ExposureMode.DURATION, "count": ExposureMode.COUNT, "source": ExposureMode.SOURCE,
             "area_count": ExposureMode.AREA_COUNT}
    z = np.load(os.path.join(GOLDEN, "renderer.npz"))
    ev = np.load(os.path.join(GOLDEN, "sinks.npz"))["ev_346x260"]
    for (h, w) in ((260, 346), (130, 173)):
        if mode == "area_count" and (h, w) != (260, 346):
            continue
        r = EventRenderer(full_scale_count=3, exposure_mode=modes[mode], exposure_value=val if val is not None else 1 / 300.0,
                          area_dimension=area)
        key = "%s_%s_%dx%d" % (mode, str(val).replace(".", "p"), h, w)
        for k, (a, b) in enumerate(((0, 1800), (1800, 1801), (1801, 5000))):
            pkt = ev[a:b].copy()
            fr = r.render_events_to_frames(torch.from_numpy(pkt).cuda() if as_tensor else pkt, height=h, width=w, return_frames=True)
            name = key + "_p%d" % k
            if name in z.files:
                assert fr is not None and fr.dtype == np.float64 and np.array_equal(fr, z[name]), name
            else:
                assert fr is None, name
        if key + "_cur" in z.files:
            assert np.array_equal(r.currentFrame.cpu().numpy(), z[key + "_cur"])
        else:
            assert r.currentFrame is None


@pytest.mark.gpu
def test_emulator_file_sinks_are_fed_from_the_device(tmp_path):
    """dvs_aedat2 / dvs_text of the drop-in: the bytes after the header are what the reference's AEDat2Output wrote for
    the same events (golden, label_signal_noise on), frame packets appended one after the other; the text file's rows are
    `repr(float64(t)) x y p label`."""
    import torch
    from v2e_amd.sinks import DeviceAEDat2Output, DeviceTextOutput
    z = np.load(os.path.join(GOLDEN, "sinks.npz"))
    ev = z["ev_346x260"]
    path = str(tmp_path / "x.aedat")
    wr = DeviceAEDat2Output(path, output_width=346, output_height=260, label_signal_noise=True)
    wr.file.flush()
    hdr = os.path.getsize(path)
    head = open(path, "rb").read()
    assert head.startswith(b"#!AER-DAT2.0\r\n") and head.count(b"\r\n") == 8
    dev = torch.from_numpy(ev).cuda()
    wr.appendEvents(dev[:4000], n_signal=4000)          # a packet of signal events only
    label = np.zeros(1000, bool)
    wr.appendEvents(ev[4000:], signnoise_label=label)   # host rows, the reference's label array: all noise
    wr.close()
    assert np.array_equal(np.frombuffer(open(path, "rb").read()[hdr:], dtype=np.uint8), z["aedat2_346x260"])
    assert wr.numEventsWritten == 5000 and wr.numOnEvents == int((ev[:, 3] > 0).sum())
    tp = str(tmp_path / "x.txt")
    tw = DeviceTextOutput(tp, label_signal_noise=True)
    tw.appendEvents(dev[:300], n_signal=250)
    tw.close()
    rows = [l for l in open(tp).read().splitlines() if not l.startswith("#")]
    assert len(rows) == 300
    for i in (0, 17, 249, 250, 299):
        t, x, y, p, lab = rows[i].split()
        assert t == repr(float(np.float64(ev[i, 0]))) and int(x) == int(ev[i, 1]) and int(y) == int(ev[i, 2])
        assert int(p) == (1 if ev[i, 3] > 0 else 0) and int(lab) == (1 if i < 250 else 0)


@pytest.mark.gpu
def test_emulator_writes_aedat2_while_generating(tmp_path):
    """EventEmulator(dvs_aedat2=..., dvs_text=...): the files hold exactly the events generate_events returned."""
    from v2e_amd import EventEmulator
    from v2e_amd.synth import int_gradient_frames
    frames = int_gradient_frames(5, 260, 346, seed=2, noise=6)
    emu = EventEmulator(device="cuda", seed=3, rng_mode="philox", output_folder=str(tmp_path), dvs_aedat2="ev", dvs_text="ev",
                        output_width=346, output_height=260, shot_noise_rate_hz=5.0, leak_rate_hz=0.1, cutoff_hz=200)
    evs = [emu.generate_events(f, i / 300) for i, f in enumerate(frames)]
    emu.cleanup()
    allev = np.concatenate([e for e in evs if e is not None])
    data = open(str(tmp_path / "ev.aedat"), "rb").read()
    pos = 0
    for _ in range(7):  # seven header lines, each ending in CRLF (no signal/noise comment line)
        pos = data.index(b"\r\n", pos) + 2
    body = data[pos:]
    words = np.frombuffer(body, dtype=">i4").reshape(-1, 2)
    assert len(words) == len(allev)
    assert np.array_equal(words[:, 1], (np.float32(1e6) * allev[:, 0]).astype(np.int32))
    x = 345 - allev[:, 1].astype(np.int32)
    y = 259 - allev[:, 2].astype(np.int32)
    p = ((allev[:, 3] + 1) / 2).astype(np.int32)
    assert np.array_equal(words[:, 0], (x << 12) | (y << 22) | (p << 11))
    rows = [l for l in open(str(tmp_path / "ev.txt")).read().splitlines() if not l.startswith("#")]
    assert len(rows) == len(allev)


class _FakeDv:
    """A stand-in for the third-party `dv_processing` package (absent from this image and from the reference tree) that RECORDS what
    a writer does with it: EventStore.push_back refuses a time stamp that goes backwards, as the real store does."""

    class EventStore:
        def __init__(self):
            self.rows = []

        def push_back(self, t, x, y, p):
            assert all(type(v) is int for v in (t, x, y, p)), "the store takes Python ints"
            if self.rows and t < self.rows[-1][0]:
                raise RuntimeError("timestamp %d is lower than the last one" % t)
            self.rows.append((t, x, y, p))

    class io:
        class MonoCameraWriter:
            instances = []

            @staticmethod
            def EventOnlyConfig(name, resolution):
                return ("event-only", name, tuple(resolution))

            def __init__(self, path, config):
                self.path, self.config, self.written = path, config, []
                type(self).instances.append(self)

            def writeEvents(self, store):
                self.written.append(list(store.rows))


def aedat4_case_events():
    """5000 events in several packets' worth, with time stamps that go backwards (refused by the store)."""
    rng = np.random.default_rng(11)
    n = 5000
    t = np.sort(rng.uniform(0.0, 3.0, n)).astype(np.float32)
    t[100], t[2500], t[2501] = t[50], 0.0, t[2400]
    return np.stack([t, rng.integers(0, 346, n).astype(np.float32), rng.integers(0, 260, n).astype(np.float32),
                     rng.choice([-1.0, 1.0], n).astype(np.float32)], axis=1)


def test_aedat4_sink_drives_dv_processing_like_the_reference_writer(tmp_path, monkeypatch):
    """SURVEY 8(f-2), AEDAT-4 (aedat4_output.py:17-99): the file container is dv_processing's and that package is not here, so the sink
    cannot be compared byte for byte; what CAN be pinned is everything the writer class itself does -- the conversions (microsecond
    time stamps in the precision numpy gives `float32 * 1e6`, polarity 0 / 1, no flips), the events the store refuses (logged and
    skipped, still counted), the counters, the writer configuration and the single write at close() -- against what the REFERENCE's
    class did with the same recording stand-in for dv_processing (tests/golden/make_golden_reference_cases.py: reference_cases.npz)."""
    import json
    import sys
    from test_oracle_vs_reference import reference_cases
    ref = reference_cases()
    monkeypatch.setitem(sys.modules, "dv_processing", _FakeDv)
    from v2e_amd.sinks import HostAEDat4Output
    ev = aedat4_case_events()
    n = len(ev)
    _FakeDv.io.MonoCameraWriter.instances.clear()
    ours = HostAEDat4Output(str(tmp_path / "ours.aedat4"), output_width=346, output_height=260)
    for lo in range(0, n, 1300):                                      # several packets, an empty one in between
        ours.appendEvents(ev[lo:lo + 1300])
        ours.appendEvents(ev[:0])
    rows = [tuple(int(v) for v in r) for r in ref["aedat4_rows"]]
    assert len(ours.store.rows) == len(rows) < n and ours.store.rows == rows
    assert [ours.numEventsWritten, ours.numOnEvents, ours.numOffEvents] == ref["aedat4_counters"].tolist() \
        and ours.numEventsWritten == n
    ours.close(); ours.close()                                        # close() twice: one write
    (wo,) = _FakeDv.io.MonoCameraWriter.instances
    written = ref["aedat4_written"]
    assert json.loads(json.dumps(wo.config)) == json.loads(str(ref["aedat4_config"]))
    assert len(wo.written) == len(written) == 1 and wo.written[0] == [tuple(int(v) for v in r) for r in written[0]]
    ours.appendEvents(ev[:10])                                        # after close(): ignored, as the reference does
    assert ours.numEventsWritten == n
