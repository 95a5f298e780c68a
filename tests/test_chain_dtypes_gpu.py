"""k_chain's float-frame and float32-state instantiations (v2e_amd/csrc/emu_chain.h: k_chain<double, float>, <float, float>,
<double, double>, <float, double>, all with the records built inside the chain) against the CPU oracle fed the same frames, bit
for bit: event rows, per-frame counts, the state planes and the three event counters.  The inputs come from
tests/chain_dtypes.py; tests/test_chain_dtypes.py shows on the CPU that they hold what these tests rely on (the edge values of
frame_record_table's float branch; quotients of frame_body's floor division that the reciprocal estimate misses by one, in both
directions, and quotients that are exact integers).

Every test asserts which kernel ran: the pipeline and its frames per launch from last_pipeline(), the state type from the dtype
of lp_log_frame, the frame type from the dtype of the array it passed in (chain_fn() in emu_chain_host.h picks the instantiation by
exactly these)."""
import numpy as np
import pytest
import torch

import chain_dtypes as cd
from v2e_amd._capi import RUN_GRAPH, RUN_ONE_FRAME_PER_LAUNCH, RUN_REQUIRE_CHAIN, V2EAmdError

pytestmark = pytest.mark.gpu

FUSED = "k_chain(fused records)"  # float frames: the chain always builds its records itself (chain_fused_records)
MODES = {"chain_graph": RUN_REQUIRE_CHAIN | RUN_GRAPH, "chain_plain": RUN_REQUIRE_CHAIN,
         "one_frame_graph": RUN_ONE_FRAME_PER_LAUNCH | RUN_GRAPH}
# (mode, V2E_AMD_CHAIN_K or None, frames per launch expected)
LAUNCHES = [("chain_graph", 8, 8), ("chain_graph", 32, 32), ("chain_plain", 8, 8), ("chain_plain", 32, 32), ("one_frame_graph", None, 1)]
TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}

_CACHE = {}


def _cached(key, make, keep=3):
    """The clip and the oracle's run of it, computed once and shared by the cases that follow one another (never changed)."""
    if key not in _CACHE:
        while len(_CACHE) >= keep:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = make()
    return _CACHE[key]


def _case(orc, row, shape, variant, n=cd.N_FRAMES):
    def make():
        frames, times = cd.case_clip(row, shape, n)
        kw = cd.case_kw(row, variant)
        ref = cd.oracle_run(orc, kw, frames, times)
        assert ref["events"].shape[0] > 0
        return frames, times, kw, ref
    return _cached((row, shape, variant, n), make)


_LIVE = []


def _emulator(kw, seed=cd.SEED):
    from v2e_amd import EventEmulator
    emu = EventEmulator(device="cuda", seed=seed, rng_mode="philox", max_iters=cd.MAX_ITERS, **kw)
    _LIVE.append(emu)
    return emu


@pytest.fixture(autouse=True)
def _close_engines():
    """A failed test's traceback keeps its emulator alive: its device handle (streams, scratch, graphs) is closed here all the
    same, so that hundreds of failing cases do not pile up hundreds of handles."""
    yield
    while _LIVE:
        obj = _LIVE.pop()  # an emulator (its engine, if it has made one) or an engine
        eng = obj if hasattr(obj, "close") else getattr(obj, "_engine", None)
        if eng is not None:
            eng.close()


def _ran(emu, frames, frame_dtype, state, kind=FUSED, fpl=None):
    """Which k_chain instantiation the last run launched: chain_fn(f64 state, frame dtype, fused records).  `frames` is what the
    run was fed (a host array or a device tensor)."""
    got = TORCH_DT.get(np.dtype(frame_dtype), torch.uint8) if torch.is_tensor(frames) else np.dtype(frame_dtype)
    assert frames.dtype == got
    got_kind, got_fpl, fpb = emu._engine.last_pipeline()
    assert got_kind == kind
    if fpl is not None:
        assert got_fpl == fpl
    assert emu.lp_log_frame.dtype == emu.base_log_frame.dtype == TORCH_DT[np.dtype(state)]
    return fpb


def _equal(emu, ev, counts, ref, kw, tag=""):
    assert list(counts) == list(ref["counts"]), tag
    ev = np.zeros((0, 4), np.float32) if ev is None else ev
    assert ev.shape == ref["events"].shape and np.array_equal(ev, ref["events"]), tag
    assert np.array_equal(emu.base_log_frame.cpu().numpy(), ref["base"]), tag
    assert np.array_equal(emu.lp_log_frame.cpu().numpy(), ref["lp"]), tag
    if kw.get("refractory_period_s", 0) > 0:
        assert np.array_equal(emu.timestamp_mem.cpu().numpy(), ref["ts"]), tag
    assert (emu.num_events_total, emu.num_events_on, emu.num_events_off) == tuple(ref["counters"]), tag


def _feed(frames, as_tensor):
    if not as_tensor:
        return frames
    t = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    assert t.dtype == TORCH_DT[frames.dtype]
    return t


# row x shape x variant x (mode, frames per launch) x feed (host array / device tensor)
CASES = [(row, shape, variant, li, as_tensor)
         for row in cd.ROWS for shape in cd.SHAPES for variant in cd.VARIANTS for li in range(len(LAUNCHES)) for as_tensor in (False, True)]


def _case_id(c):
    row, shape, variant, li, as_tensor = c
    mode, K, _ = LAUNCHES[li]
    return "-".join([row, shape, variant, mode] + (["k%d" % K] if K else []) + ["tensor" if as_tensor else "host"])


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_float_frame_chain_matches_oracle(case, oracle_lib, monkeypatch):
    """75 frames (two full 32-frame launches and a partial one; at 8 frames per launch nine and a partial one) at a ragged size."""
    row, shape, variant, li, as_tensor = case
    mode, K, fpl = LAUNCHES[li]
    frames, times, kw, ref = _case(oracle_lib, row, shape, variant)
    if K is not None:
        monkeypatch.setenv("V2E_AMD_CHAIN_K", str(K))
    emu = _emulator(kw)
    fed = _feed(frames, as_tensor)
    ev, counts = emu.generate_events_batch(fed, times, use_graph=MODES[mode])
    _ran(emu, fed, cd.ROWS[row]["frames"], cd.ROWS[row]["state"], fpl=fpl)
    _equal(emu, ev, counts, ref, kw)


@pytest.mark.parametrize("row", ["f64state_f32frames", "f64state_f64frames"])
def test_float_frame_chain_runs_longer_than_the_ring(row, oracle_lib):
    """259 run frames in one run: the ring of frame slots (three emission batches of 64 frames) wraps once."""
    frames, times, kw, ref = _case(oracle_lib, row, "33x37", "all_on", n=cd.N_WRAP)
    emu = _emulator(kw)
    ev, counts = emu.generate_events_batch(frames, times, use_graph=MODES["chain_graph"])
    fpb = _ran(emu, frames, cd.ROWS[row]["frames"], cd.ROWS[row]["state"], fpl=32)
    assert fpb == 64 and 3 * fpb < len(frames) - 1
    _equal(emu, ev, counts, ref, kw)


@pytest.mark.parametrize("api", ["runs", "pipelined"])
@pytest.mark.parametrize("chunk", [24, 9])
@pytest.mark.parametrize("row", list(cd.ROWS))
def test_float_frame_clip_in_runs_equals_whole_clip(row, chunk, api, oracle_lib):
    """The 75-frame clip in runs of 24 and of 9 frames through the carried state, blocking (one hipGraph per run) and pipelined
    (generate_events_batch_async, every run enqueued before the result of the run before it is read; frames resident and not):
    the whole clip's rows -- the oracle's -- and its final state."""
    frames, times, kw, ref = _case(oracle_lib, row, "33x37", "refractory_mixed")
    ftype, state = cd.ROWS[row]["frames"], cd.ROWS[row]["state"]
    if api == "runs":
        emu = _emulator(kw)
        evs, cnts = [], []
        for lo in range(0, len(frames), chunk):
            ev, c = emu.generate_events_batch(frames[lo:lo + chunk], times[lo:lo + chunk], use_graph=MODES["chain_graph"])
            _ran(emu, frames[lo:lo + chunk], ftype, state)
            if ev is not None:
                evs.append(ev)
            cnts += list(c)
        _equal(emu, np.concatenate(evs), cnts, ref, kw)
        return
    dev = _feed(frames, True)
    torch.cuda.synchronize()
    for resident in (True, False):
        emu = _emulator(kw)
        pend, evs, cnts = [], [], []
        for lo in range(0, len(frames), chunk):
            pend.append(emu.generate_events_batch_async(dev[lo:lo + chunk], times[lo:lo + chunk], use_graph=0, return_device=True,
                                                        frames_resident=resident))
            if len(pend) > 1:
                ev, c = pend.pop(0).result()
                evs.append(ev.cpu().numpy()); cnts += list(c)
        ev, c = pend.pop(0).result()
        evs.append(ev.cpu().numpy()); cnts += list(c)
        _ran(emu, dev, ftype, state)
        _equal(emu, np.concatenate(evs), cnts, ref, kw, "resident" if resident else "not resident")


# ---------------------------------------------------------------- the reciprocal floor division of frame_body
def _built(orc, kw, built):
    """(frames, times, hits or None, the oracle's run) of a clip built by cd.fixup_frames / _rounded / _u8"""
    frames, times = built[0], built[1]
    ref = cd.oracle_run(orc, kw, frames, times, seed=3)
    assert ref["events"].shape[0] > 0
    return frames, times, (built[2] if len(built) > 2 else None), ref


FIXUPS = {"estimate_too_large": cd.FIXUP_KW, "estimate_too_small": cd.FIXUP_KW_DOWN}


@pytest.mark.parametrize("K", [2, 32], ids=["k2", "k32"])
@pytest.mark.parametrize("mode", ["chain_plain", "chain_graph"])
@pytest.mark.parametrize("which", list(FIXUPS))
def test_fixup_arms_of_the_floor_division_float32_state(which, mode, K, oracle_lib, monkeypatch):
    """k_chain<float, float>: on most pixels of every frame the estimate q0 = floor(am * (1 / theta)) is one too large (thresholds
    0.2 / 0.15: the `r0 < 0` arm), one too small with r0 == theta exactly (55 / 256 and 355 / 2048: the `r0 >= bt` arm and its
    equality), or right with r0 == 0 (tests/test_chain_dtypes.py counts them)."""
    kw = FIXUPS[which]
    frames, times, hits, ref = _cached(("fixup", which), lambda: _built(oracle_lib, kw, cd.fixup_frames(oracle_lib, kw, 33, 37, 3)))
    want = -1 if which == "estimate_too_small" else 1
    assert all(int((h == want).sum()) >= 400 for h in hits) and ref["events"].shape[0] > 0
    monkeypatch.setenv("V2E_AMD_CHAIN_K", str(K))
    emu = _emulator(kw, seed=3)
    ev, counts = emu.generate_events_batch(frames, times, use_graph=MODES[mode])
    _ran(emu, frames, np.float32, np.float32, fpl=K)
    _equal(emu, ev, counts, ref, kw)


@pytest.mark.parametrize("fused", [False, True], ids=["ahead_records", "fused_records"])
@pytest.mark.parametrize("mode", ["chain_plain", "chain_graph"])
@pytest.mark.parametrize("source", ["rounded", "searched"])
def test_fixup_arms_of_the_floor_division_uint8_frames(source, mode, fused, oracle_lib, monkeypatch):
    """k_chain<float, uint8_t, *>: grey levels whose quotient the estimate misses by one or divides exactly -- fixup_frames rounded
    to bytes (8 pixel-frames keep a hit) and the byte search of fixup_frames_u8 (131); tests/test_chain_dtypes.py counts both."""
    kw = cd.FIXUP_KW
    build = cd.fixup_frames_rounded if source == "rounded" else cd.fixup_frames_u8
    frames, times, hits, ref = _cached(("fixup_u8", source), lambda: _built(oracle_lib, kw, build(oracle_lib, kw, 33, 37, 3)))
    if hits is not None:
        assert int((hits != 0).sum()) >= 20 and int((hits == 1).sum()) >= 1
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "1" if fused else "0")
    monkeypatch.setenv("V2E_AMD_CHAIN_K", "2" if source == "rounded" else "4")
    emu = _emulator(kw, seed=3)
    ev, counts = emu.generate_events_batch(frames, times, use_graph=MODES[mode])
    _ran(emu, frames, np.uint8, np.float32, kind=FUSED if fused else "k_chain", fpl=2 if source == "rounded" else 4)
    _equal(emu, ev, counts, ref, kw)


@pytest.mark.parametrize("mode", ["chain_plain", "chain_graph"])
def test_exact_multiples_in_float64_state(mode, oracle_lib):
    """k_chain<double, float> with hdr: L is the pixel value, every quotient of frames 1-19 an exact integer (r0 == 0: 15 699
    pixel-frames with an event); leak and shot noise are off in those frames and on from frame 20 (the emulator's attributes,
    changed between runs)."""
    frames, times = cd.exact_multiple_clip(40, 33, 37, 5)
    noisy = {k: cd.EXACT_KW_NOISY[k] for k in ("leak_rate_hz", "shot_noise_rate_hz")}
    quiet = {k: 0.0 for k in noisy}
    ref = _cached(("exact",), lambda: cd.oracle_run(oracle_lib, cd.EXACT_KW_NOISY, frames, times, phases=[(1, quiet), (20, noisy)]))
    emu = _emulator(cd.EXACT_KW_NOISY)
    evs, cnts = [], []
    for lo, hi, attrs in ((0, 1, {}), (1, 20, quiet), (20, 40, noisy)):
        for k, v in attrs.items():
            setattr(emu, k, v)
        ev, c = emu.generate_events_batch(frames[lo:hi], times[lo:hi], use_graph=MODES[mode])
        if hi > 1:
            _ran(emu, frames[lo:hi], np.float32, np.float64)
        if ev is not None:
            evs.append(ev)
        cnts += list(c)
    _equal(emu, np.concatenate(evs), cnts, ref, cd.EXACT_KW_NOISY)


# ---------------------------------------------------------------- several clips, and the configuration the chain refuses
@pytest.mark.parametrize("cutoff_hz", [300, 0], ids=["f64state", "f32state"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32frames", "f64frames"])
def test_float_frames_of_several_clips(dtype, cutoff_hz, oracle_lib):
    """Three clips of 60x100 in one engine (frames [F][3][H][W]: the frame index of clip c is clip * npx + p), each with frame
    times of its own; every clip equals the oracle's clip stream c."""
    from v2e_amd.emulator import EventEmulator
    from v2e_amd.engine import EmuEngine
    clips, times, kw = cd.multi_clip_case(dtype, cutoff_hz)  # times [F][NC]
    (F, H, W), NC = clips[0].shape, len(clips)
    proto = EventEmulator(device="cuda", seed=cd.MULTI_SEED, rng_mode="philox", **kw)
    _LIVE.append(proto)
    proto._thres_scalar = (0.2, 0.2)
    proto._thres_is_scalar = False
    P = proto._params()
    eng = EmuEngine(H, W, n_clips=NC, device="cuda", max_iters=cd.MAX_ITERS)
    _LIVE.append(eng)
    eng.alloc_state(cutoff_hz > 0)
    frames = torch.from_numpy(np.stack(clips, axis=1)).cuda()  # [F][NC][H][W]
    assert frames.dtype == TORCH_DT[np.dtype(dtype)]
    eng.init_state(P, frames[0].contiguous(), 0.0)
    cap = 16 * H * W * F
    ev = eng.event_buffer(cap)
    recs = eng.alloc_recs(F - 1)
    t_prev = np.concatenate([np.zeros((1, NC)), times[1:F - 1]])
    eng.run(P, frames[1:].contiguous(), t_prev, times[1:], 1, ev, recs, use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    assert eng.last_pipeline()[0] == FUSED
    assert eng.lp.dtype == (torch.float64 if cutoff_hz > 0 else torch.float32)
    r = eng.recs_to_numpy(recs)
    assert not r["flags"].any()
    for c in range(NC):
        ref = cd.oracle_run(oracle_lib, kw, clips[c], [0.0] + list(times[1:, c]), seed=cd.MULTI_SEED, clip=c)
        n = int(r["n_events"][:, c].sum())
        assert n == len(ref["events"]) > 0, "clip %d" % c
        assert list(r["n_events"][:, c]) == ref["counts"][1:], "clip %d" % c
        assert np.array_equal(ev[c, :n].cpu().numpy(), ref["events"]), "clip %d" % c
        assert np.array_equal(eng.plane(eng.base, c).cpu().numpy(), ref["base"]), "clip %d" % c
        assert np.array_equal(eng.plane(eng.lp, c).cpu().numpy(), ref["lp"]), "clip %d" % c
        assert np.array_equal(eng.plane(eng.ts_mem, c).cpu().numpy(), ref["ts"]), "clip %d" % c
        assert (int(r["n_events"][:, c].sum()), int(r["n_on"][:, c].sum()), int(r["n_off"][:, c].sum())) == tuple(ref["counters"])


@pytest.mark.parametrize("use_graph", [True, 0, RUN_GRAPH], ids=["default", "plain", "graph"])
def test_float64_log_frames_fall_back_to_the_per_frame_kernels(use_graph, oracle_lib):
    """float64 frames with hdr: the chain's record carries the lin-log value as float32, which would round a float64 log
    intensity, so chain_eligible() sends the run to the per-frame kernels (equal to the oracle) and RUN_REQUIRE_CHAIN is refused."""
    frames, times, kw = cd.fallback_case()
    assert frames.dtype == np.float64 and np.mean(frames != frames.astype(np.float32)) > 0.9
    ref = _cached(("fallback",), lambda: cd.oracle_run(oracle_lib, kw, frames, times))
    assert ref["events"].shape[0] > 0
    emu = _emulator(kw)
    ev, counts = emu.generate_events_batch(frames, times, use_graph=use_graph)
    assert emu._engine.last_pipeline() == ("k_count/k_rank/k_scan/k_emit", 1, 1)
    assert emu.lp_log_frame.dtype == torch.float64
    _equal(emu, ev, counts, ref, kw)
    with pytest.raises(V2EAmdError):
        emu.generate_events_batch(frames[-2:], [times[-1] + 0.01, times[-1] + 0.02], use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    # float32 frames of the same emulator: the chain takes them
    f32 = frames[-2:].astype(np.float32)
    emu.generate_events_batch(f32, [times[-1] + 0.01, times[-1] + 0.02], use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    _ran(emu, f32, np.float32, np.float64)
