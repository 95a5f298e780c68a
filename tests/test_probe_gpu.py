"""Single-pixel model states in device-resident runs (v2e_emu_set_probes, csrc/probe.hip) on the MI355X: an emulator built with
record_single_pixel_states fed through generate_events_batch records what the same emulator fed through generate_events frame by
frame records -- every one of the ten series, exactly, NaN padding included -- and `probe_pixels` gives the same series for up to 64
pixels of a run.

The per-frame recorder is pinned to the reference by tests/golden/single_pixel.npz (test_emulator_gpu.py, tape mode); nobody can
drive the batch path in tape mode, so the per-frame recorder in Philox mode is the reference here.  A probed run takes the same
kernels as the per-frame API, so every comparison is exact equality of float64 arrays.

Cases (each checked on the CPU with the oracle: the pixel with the most signal events fires ON and OFF):
  defaults, hdr, photoreceptor noise: the fixtures philox_moving_dot_64x64, philox_hdr_97x131, philox_pnoise_97x131;
  scidvs (float64 and float32 state): the parameters of philox_scidvs_97x131 / philox_scidvs_f32_97x131 on the frames of
      philox_probe_flicker_97x131 -- in those two fixtures, and with their parameters on the frames of every other small Philox
      fixture, the busiest pixel fires OFF only (52 OFF / 0 ON): see tests/golden/make_golden_probe.py;
  centre-surround: philox_csdvs_f32_346x260 (6 ON / 5 OFF; the busiest pixels of philox_csdvs_97x131 and philox_csdvs_346x260
      fire OFF only, 28 and 26 times);
  refractory: the first 20 frames of philox_refractory_346x260 (13 ON / 5 OFF, two events in one frame; within its first 12
      frames the busiest pixel fires 13 ON / 0 OFF, and philox_refractory_1280x720 has no pixel with two events in a frame)."""
import os
import pickle

import numpy as np
import pytest
import torch

from fixtures import GOLDEN, PhiloxFixture

pytestmark = pytest.mark.gpu

SERIES = ("time", "new_frame", "base_log_frame", "lp_log_frame", "log_new_frame", "pos_thres", "neg_thres", "diff_frame",
          "final_neg_evts_frame", "final_pos_evts_frame")


class Case:
    def __init__(self, name):
        kw_from, frames_from, n = {
            "defaults": ("philox_moving_dot_64x64", None, None),
            "hdr": ("philox_hdr_97x131", None, None),
            "pnoise": ("philox_pnoise_97x131", None, None),
            "scidvs": ("philox_scidvs_97x131", "philox_probe_flicker_97x131", None),
            "scidvs_f32": ("philox_scidvs_f32_97x131", "philox_probe_flicker_97x131", None),
            "csdvs": ("philox_csdvs_f32_346x260", None, None),
            "refractory": ("philox_refractory_346x260", None, 20),
        }[name]
        fx = PhiloxFixture(kw_from)
        self.name, self.kw, self.preset, self.seed = name, fx.kw, fx.preset, fx.seed
        self.frames, self.times = fx.frames, [float(t) for t in fx.times]
        if frames_from:
            z = np.load(os.path.join(GOLDEN, frames_from + ".npz"))
            self.frames, self.times, self.seed = z["frames"], [float(t) for t in z["times"]], int(z["seed"])
        if n:
            self.frames, self.times = self.frames[:n], self.times[:n]

    def emu(self, **extra):
        from v2e_amd import EventEmulator
        e = EventEmulator(device="cuda", seed=self.seed, rng_mode="philox", **self.kw, **extra)
        if self.preset:
            e.set_dvs_params(self.preset)
        return e

    def cuts(self):
        """Uneven runs: (first frame + 1), 5, the rest."""
        F = len(self.frames)
        return [(0, 2), (2, 7), (7, F)]


def _rows(ev):
    return np.zeros((0, 4), np.float32) if ev is None else ev


def _signal_counts(rows, counts, n_signal, H, W):
    """ON / OFF signal events per frame and pixel from a run's rows: [F, H, W] each."""
    on, off = np.zeros((len(counts), H, W), np.int64), np.zeros((len(counts), H, W), np.int64)
    row = 0
    for f, (n, ns) in enumerate(zip(counts, n_signal)):
        s = rows[row:row + int(ns)]
        y, x = s[:, 2].astype(np.int64), s[:, 1].astype(np.int64)
        np.add.at(on[f], (y[s[:, 3] > 0], x[s[:, 3] > 0]), 1)
        np.add.at(off[f], (y[s[:, 3] < 0], x[s[:, 3] < 0]), 1)
        row += int(n)
    return on, off


_PLAIN = {}


def _plain(name):
    """The case's clip as one unprobed device-resident run, once per module: rows, counts, n_signal per frame, counters, final
    planes, the pipeline it took, and the pixel with the most signal events."""
    if name not in _PLAIN:
        c = Case(name)
        emu = c.emu()
        p = emu.generate_events_batch_async(c.frames, c.times, use_graph=0, pipelined=False)
        ev, counts = p.result()
        ns = np.concatenate([[0], p.rec_host["n_signal"]])
        H, W = c.frames.shape[1:]
        on, off = _signal_counts(_rows(ev), counts, ns, H, W)
        tot = (on + off).sum(0)
        ij = tuple(int(v) for v in np.unravel_index(np.argmax(tot), tot.shape))
        _PLAIN[name] = dict(ev=_rows(ev), counts=counts, n_signal=ns, on=on, off=off, ij=ij, kind=_kind(emu),
                            counters=(emu.num_events_total, emu.num_events_on, emu.num_events_off),
                            lp=emu.lp_log_frame.cpu().numpy(), base=emu.base_log_frame.cpu().numpy())
        emu.cleanup()
    return _PLAIN[name]


def _kind(emu):
    import ctypes as C
    k, a, b = C.c_int(), C.c_int(), C.c_int()
    assert emu._engine.lib.v2e_emu_last_pipeline(emu._engine._h, C.byref(k), C.byref(a), C.byref(b)) == 0
    return k.value


def _same_series(a, b):
    assert sorted(a) == sorted(b) == sorted(SERIES)
    for k in SERIES:
        assert a[k].dtype == np.float64 == b[k].dtype
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, a[k][:12], b[k][:12])


@pytest.mark.parametrize("name", ["defaults", "hdr", "pnoise", "scidvs", "scidvs_f32", "csdvs", "refractory"])
def test_batch_recorder_equals_per_frame_recorder(name, tmp_path, monkeypatch):
    """The same frames, seed and Philox streams through generate_events per frame and through generate_events_batch in uneven
    runs: all ten series, the sample count and the pickled files are equal.  The probed pixel is the one with the most signal
    events, and it fires ON and OFF (for the refractory case twice in one frame): a zero would leave the event columns untested."""
    monkeypatch.chdir(tmp_path)  # SINGLE_PIXEL_STATES_FILENAME is relative, as in the reference
    c = Case(name)
    ij = _plain(name)["ij"]
    ref = c.emu(record_single_pixel_states=ij)
    for f, t in zip(c.frames, c.times):
        ref.generate_events(f, t)
    n = ref.single_pixel_sample_count
    st = ref.single_pixel_states
    print(name, "pixel", ij, "ON", np.nansum(st["final_pos_evts_frame"]), "OFF", np.nansum(st["final_neg_evts_frame"]),
          "most in a frame", np.nanmax(st["final_pos_evts_frame"] + st["final_neg_evts_frame"]))
    assert n == len(c.frames) - 1
    assert np.nansum(st["final_pos_evts_frame"]) >= 1 and np.nansum(st["final_neg_evts_frame"]) >= 1
    if name == "refractory":
        assert np.nanmax(st["final_pos_evts_frame"] + st["final_neg_evts_frame"]) >= 2
    ref.cleanup()
    with open(ref.SINGLE_PIXEL_STATES_FILENAME, "rb") as f:
        d_ref = pickle.load(f)
    os.remove(ref.SINGLE_PIXEL_STATES_FILENAME)

    emu = c.emu(record_single_pixel_states=ij)
    for lo, hi in c.cuts():
        emu.generate_events_batch(c.frames[lo:hi], c.times[lo:hi])
        assert _kind(emu) == 0
    assert emu.single_pixel_sample_count == n
    _same_series(emu.single_pixel_states, st)
    emu.cleanup()
    with open(emu.SINGLE_PIXEL_STATES_FILENAME, "rb") as f:
        d = pickle.load(f)
    _same_series(d, d_ref)
    _same_series(d, st)


@pytest.mark.parametrize("name", ["defaults", "hdr", "refractory"])
def test_probing_does_not_change_the_run(name):
    """Events, counts, counters and the final planes of a probed run (per-frame kernels) equal those of the unprobed run (k_chain), and
    the last sample of base_log_frame / lp_log_frame is the plane's element after the run."""
    c = Case(name)
    plain = _plain(name)
    assert plain["kind"] in (3, 4)
    ij = plain["ij"]
    emu = c.emu()
    p = emu.generate_events_batch_async(c.frames, c.times, use_graph=0, probe_pixels=[ij])
    ev, counts = p.result()
    assert _kind(emu) == 0
    assert np.array_equal(counts, plain["counts"]) and np.array_equal(_rows(ev).view(np.int32), plain["ev"].view(np.int32))
    assert (emu.num_events_total, emu.num_events_on, emu.num_events_off) == plain["counters"]
    lp, base = emu.lp_log_frame.cpu().numpy(), emu.base_log_frame.cpu().numpy()
    assert np.array_equal(lp, plain["lp"]) and np.array_equal(base, plain["base"])
    pr = p.probes
    assert sorted(pr) == sorted(SERIES) and all(v.shape == (len(c.frames) - 1, 1) and v.dtype == np.float64 for v in pr.values())
    assert pr["base_log_frame"][-1, 0] == float(base[ij]) and pr["lp_log_frame"][-1, 0] == float(lp[ij])
    assert np.array_equal(pr["time"][:, 0], np.asarray(c.times[1:]))
    assert np.array_equal(pr["final_pos_evts_frame"][:, 0], plain["on"][1:, ij[0], ij[1]])
    assert np.array_equal(pr["final_neg_evts_frame"][:, 0], plain["off"][1:, ij[0], ij[1]])


def test_64_probes_at_97x131():
    """64 probes at a width that is no multiple of the wave: the four corners, one pixel twice, the busiest pixel.  Every column
    equals the single-probe run of its pixel; the ON / OFF columns equal counts made on the host from the rows and n_signal."""
    c = Case("hdr")
    plain = _plain("hdr")
    H, W = c.frames.shape[1:]
    assert (H, W) == (97, 131)
    rng = np.random.default_rng(64)
    px = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), plain["ij"], plain["ij"]]
    tot = (plain["on"] + plain["off"]).sum(0)
    px += [tuple(int(v) for v in np.unravel_index(i, tot.shape)) for i in np.argsort(tot, axis=None)[-27:-1]]  # the next 26 busiest
    px += [(int(a), int(b)) for a, b in zip(rng.integers(0, H, 32), rng.integers(0, W, 32))]
    assert len(px) == 64
    emu = c.emu()
    ev, counts = emu.generate_events_batch(c.frames, c.times, probe_pixels=px)
    assert np.array_equal(_rows(ev).view(np.int32), plain["ev"].view(np.int32))
    pr = emu.last_probes
    assert all(pr[k].shape == (len(c.frames) - 1, 64) for k in SERIES)
    on = np.stack([plain["on"][1:, a, b] for a, b in px], axis=1)
    off = np.stack([plain["off"][1:, a, b] for a, b in px], axis=1)
    assert on.sum() > 50 and off.sum() > 50
    assert np.array_equal(pr["final_pos_evts_frame"], on) and np.array_equal(pr["final_neg_evts_frame"], off)
    single = {}
    for j, ab in enumerate(px):
        if ab not in single:
            e1 = c.emu()
            e1.generate_events_batch(c.frames, c.times, probe_pixels=[ab])
            single[ab] = e1.last_probes
        for k in SERIES:
            assert np.array_equal(pr[k][:, j], single[ab][k][:, 0]), (k, ab)


def test_run_modes_give_the_same_series(tmp_path, monkeypatch):
    """Graph runs (the second run of a length replays the captured graph), plain launches, and the asynchronous API with three
    runs enqueued before any result is read and one handle dropped unread: the per-frame recorder's series, in order."""
    monkeypatch.chdir(tmp_path)
    c = Case("defaults")
    c.frames, c.times = c.frames[:41], c.times[:41]
    ij = _plain("defaults")["ij"]
    ref = c.emu(record_single_pixel_states=ij)
    for f, t in zip(c.frames, c.times):
        ref.generate_events(f, t)
    st, n = ref.single_pixel_states, ref.single_pixel_sample_count
    assert n == 40 and np.nansum(st["final_pos_evts_frame"]) + np.nansum(st["final_neg_evts_frame"]) >= 1
    cuts = [(0, 9)] + [(lo, lo + 8) for lo in range(9, 41, 8)]  # runs of 8 frames: the graph of that length is taken from the second on

    for use_graph in (True, 0):
        emu = c.emu(record_single_pixel_states=ij)
        for lo, hi in cuts:
            emu.generate_events_batch(c.frames[lo:hi], c.times[lo:hi], use_graph=use_graph)
        assert emu.single_pixel_sample_count == n
        _same_series(emu.single_pixel_states, st)
        emu.record_single_pixel_states = None

    emu = c.emu(record_single_pixel_states=ij)
    frames = torch.from_numpy(np.ascontiguousarray(c.frames)).cuda()
    pend = [emu.generate_events_batch_async(frames[lo:hi], c.times[lo:hi], use_graph=0, return_device=True) for lo, hi in cuts[:3]]
    # (no result() called: the third call took the first run's buffer set and collected that run, as it does for the event files)
    assert emu.single_pixel_sample_count == 8
    del pend[1]  # dropped unread: collected, in order, by the run that reuses its buffers
    pend.append(emu.generate_events_batch_async(frames[cuts[3][0]:cuts[3][1]], c.times[cuts[3][0]:cuts[3][1]], use_graph=0,
                                                return_device=True))
    pend.append(emu.generate_events_batch_async(frames[cuts[4][0]:cuts[4][1]], c.times[cuts[4][0]:cuts[4][1]], use_graph=0,
                                                return_device=True))
    pend[-1].result()
    assert emu.single_pixel_sample_count == n
    _same_series(emu.single_pixel_states, st)
    del pend
    emu.cleanup()
    with open(emu.SINGLE_PIXEL_STATES_FILENAME, "rb") as f:
        _same_series(pickle.load(f), st)
    ref.record_single_pixel_states = None


def test_path_selection_and_the_sample_cap(tmp_path, monkeypatch):
    """An unprobed run takes k_chain as before, a probed one the per-frame kernels; once SINGLE_PIXEL_MAX_SAMPLES is reached the
    file is saved, the recording ends as in the per-frame path and the next run takes the chain again."""
    from v2e_amd import EventEmulator
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(EventEmulator, "SINGLE_PIXEL_MAX_SAMPLES", 7)
    c = Case("defaults")
    plain = _plain("defaults")
    assert plain["kind"] in (3, 4)
    ij = plain["ij"]
    ref = c.emu(record_single_pixel_states=ij)
    for f, t in zip(c.frames[:16], c.times[:16]):
        ref.generate_events(f, t)
    assert ref.single_pixel_sample_count == 7 and ref.record_single_pixel_states is None and ref.single_pixel_states["time"].shape == (7,)
    with open(ref.SINGLE_PIXEL_STATES_FILENAME, "rb") as f:
        d_ref = pickle.load(f)
    os.remove(ref.SINGLE_PIXEL_STATES_FILENAME)

    emu = c.emu(record_single_pixel_states=ij)
    emu.generate_events_batch(c.frames[:6], c.times[:6])
    assert _kind(emu) == 0 and emu.single_pixel_sample_count == 5
    emu.generate_events_batch(c.frames[6:11], c.times[6:11])  # two samples fit; the third frame finds the series full
    assert _kind(emu) == 0 and emu.single_pixel_sample_count == 7 and emu.record_single_pixel_states is None
    assert os.path.isfile(emu.SINGLE_PIXEL_STATES_FILENAME)
    emu.generate_events_batch(c.frames[11:16], c.times[11:16])
    assert _kind(emu) in (3, 4)
    _same_series(emu.single_pixel_states, ref.single_pixel_states)
    with open(emu.SINGLE_PIXEL_STATES_FILENAME, "rb") as f:
        _same_series(pickle.load(f), d_ref)

    # the series exactly full at the end of a run: the next run's first frame saves and ends the recording, and takes the chain
    os.remove(emu.SINGLE_PIXEL_STATES_FILENAME)
    emu = c.emu(record_single_pixel_states=ij)
    emu.generate_events_batch(c.frames[:8], c.times[:8])
    assert emu.single_pixel_sample_count == 7 and emu.record_single_pixel_states == ij and not os.path.exists(emu.SINGLE_PIXEL_STATES_FILENAME)
    emu.generate_events_batch(c.frames[8:16], c.times[8:16])
    assert _kind(emu) in (3, 4) and emu.record_single_pixel_states is None and os.path.isfile(emu.SINGLE_PIXEL_STATES_FILENAME)
    _same_series(emu.single_pixel_states, ref.single_pixel_states)


def test_refusals():
    from v2e_amd._capi import RUN_GRAPH, RUN_REQUIRE_CHAIN, V2EAmdError
    c = Case("hdr")
    H, W = c.frames.shape[1:]
    emu = c.emu(show_dvs_model_state=["all"])
    with pytest.raises(ValueError, match="show_dvs_model_state"):
        emu.generate_events_batch(c.frames, c.times)
    emu.cleanup()
    emu = c.emu()
    with pytest.raises(ValueError, match="at most 64"):
        emu.generate_events_batch(c.frames, c.times, probe_pixels=[(0, k) for k in range(65)])
    for bad in [(H, 0), (0, W), (-1, 0), (0.5, 1)]:
        with pytest.raises(ValueError):
            emu.generate_events_batch(c.frames, c.times, probe_pixels=[bad])
    assert not emu._initialized  # refused before anything ran
    with pytest.raises(V2EAmdError, match="v2e_emu_set_probes"):
        emu.generate_events_batch(c.frames, c.times, use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH, probe_pixels=[(1, 1)])
    # the library's own checks (the Python layer validates first; these guard other callers of the C ABI)
    import ctypes as C
    eng = emu._engine
    out = torch.empty((4, 65, 9), dtype=torch.float64, device="cuda")
    assert eng.lib.v2e_emu_set_probes(eng._h, (C.c_int32 * 65)(), 65, out.data_ptr()) != 0
    assert eng.lib.v2e_emu_set_probes(eng._h, (C.c_int32 * 1)(H * W), 1, out.data_ptr()) != 0
    assert eng.lib.v2e_emu_set_probes(eng._h, (C.c_int32 * 1)(-1), 1, out.data_ptr()) != 0
    assert eng.lib.v2e_emu_set_probes(eng._h, None, 0, None) == 0


def test_video_to_events_records_across_runs_and_chunks(tmp_path, monkeypatch):
    """VideoToEvents.run and run_stream (chunks of one flow chunk) with a recording emulator: equal single_pixel_states, the sample
    index running on across the chunk boundaries, both equal to generate_events per frame over the pipeline's interpolated frames
    and times; cleanup() writes the file."""
    from v2e_amd import EventEmulator
    from v2e_amd.pipeline import VideoToEvents, flow_chunk_pairs, interp_frame_times
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import int_gradient_frames, portable_unet_state_dict
    monkeypatch.chdir(tmp_path)
    sd_f, sd_i = portable_unet_state_dict(2, 4, 401), portable_unet_state_dict(12, 5, 402)
    eng = SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()}, {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda")
    kw = dict(pos_thres=0.15, neg_thres=0.15, sigma_thres=0.03, cutoff_hz=200, leak_rate_hz=0.1, shot_noise_rate_hz=2.0,
              refractory_period_s=0.001)
    U, bs, dt = 2, 8, 1 / 30.0
    fc = flow_chunk_pairs(bs)
    src = int_gradient_frames(fc + 17, 64, 96, seed=3, noise=10, as_array=True)  # two chunks, the second one short
    dev = torch.from_numpy(src).cuda()

    def emu(**extra):
        return EventEmulator(device="cuda", seed=5, rng_mode="philox", **kw, **extra)

    pipe = VideoToEvents(eng, emu(), U, batch_size=bs)
    ev, counts, n = pipe.run(dev, dt)
    up = pipe.upsample(dev).cpu().numpy()
    times = [float(t) for t in interp_frame_times(len(src), U, dt, bs)]
    assert n == len(up) == len(times) == (len(src) - 1) * U
    tot = np.zeros((64, 96), np.int64)
    np.add.at(tot, (ev[:, 2].astype(np.int64), ev[:, 1].astype(np.int64)), 1)
    ij = tuple(int(v) for v in np.unravel_index(np.argmax(tot), tot.shape))

    ref = emu(record_single_pixel_states=ij)
    for f, t in zip(up, times):
        ref.generate_events(f, t)
    st = ref.single_pixel_states
    assert ref.single_pixel_sample_count == n - 1
    assert np.nansum(st["final_pos_evts_frame"]) + np.nansum(st["final_neg_evts_frame"]) >= 1
    ref.record_single_pixel_states = None

    a = VideoToEvents(eng, emu(record_single_pixel_states=ij), U, batch_size=bs)
    ev_a, counts_a, _ = a.run(dev, dt)
    b = VideoToEvents(eng, emu(record_single_pixel_states=ij), U, batch_size=bs)
    ev_b, counts_b, _ = b.run_stream(dev, dt, chunk_pairs=fc)
    assert np.array_equal(counts_a, counts) and np.array_equal(counts_b, counts)
    assert np.array_equal(ev_a.view(np.int32), ev.view(np.int32)) and np.array_equal(ev_b.view(np.int32), ev.view(np.int32))
    for p in (a, b):
        assert p.emu.single_pixel_sample_count == n - 1
        _same_series(p.emu.single_pixel_states, st)
    a.emu.record_single_pixel_states = None
    b.emu.cleanup()
    with open(b.emu.SINGLE_PIXEL_STATES_FILENAME, "rb") as f:
        _same_series(pickle.load(f), st)


def test_a_first_call_with_the_first_frame_alone_is_an_empty_run():
    """The clip's first frame only initialises the state: a call that carries nothing else returns the empty handle -- no rows
    (a [0, 4] device tensor with return_device), zero counts, the ten series with no sample of every probed pixel -- and the
    clip goes on from there as if the frame had come with the next run."""
    c = Case("defaults")
    whole = c.emu()
    ev, counts = whole.generate_events_batch(c.frames[:8], c.times[:8], probe_pixels=[(1, 2), (3, 4), (5, 6)])
    emu = c.emu()
    ev0, counts0 = emu.generate_events_batch(c.frames[:1], c.times[:1], probe_pixels=[(1, 2), (3, 4), (5, 6)])
    assert ev0 is None and list(counts0) == [0] and (emu.num_events_total, emu.frame_counter) == (0, 1)
    assert tuple(emu.last_probes) == SERIES and all(emu.last_probes[k].shape == (0, 3) for k in SERIES)
    ev1, counts1 = emu.generate_events_batch(c.frames[1:8], c.times[1:8], probe_pixels=[(1, 2), (3, 4), (5, 6)])
    assert np.array_equal(_rows(ev1), _rows(ev)) and list(counts1) == list(counts[1:])
    for k in SERIES:
        assert np.array_equal(emu.last_probes[k], whole.last_probes[k], equal_nan=True), k
    h = c.emu().generate_events_batch_async(c.frames[:1], c.times[:1], return_device=True)
    rows, counts2 = h.result()
    assert torch.is_tensor(rows) and rows.is_cuda and tuple(rows.shape) == (0, 4) and list(counts2) == [0]
    assert h.done is None and h.probes is None
