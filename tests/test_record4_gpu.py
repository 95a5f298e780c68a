"""GPU parity of the chain that reads k_ahead's 4-byte records (V2E_AMD_CHAIN_FUSED=0: the leak step as a record, the shot
decisions as per-wave ballot masks, the pixel byte from the frame itself) against the CPU oracle and against the chain that
builds its records itself (=1): events, counts and planes, bit for bit.

33x37 = 1221 pixels throughout: 19 full waves, one wave of 5 pixels (1216 .. 1220), and a last workgroup that is mostly
padding.  Frame intervals are not uniform (a dt_over_tau per frame), as in test_record8_gpu.py.  Every precondition is
asserted from the oracle's own output."""
import numpy as np
import pytest
import torch

from v2e_amd._capi import RUN_GRAPH, RUN_REQUIRE_CHAIN

pytestmark = pytest.mark.gpu

H, W = 33, 37
NPX = H * W
LAST_WAVE = NPX // 64 * 64  # 1216: first pixel of the partial wave
SUB = 8  # frames of a chain sub-pass (CHAIN_SUB): launches are multiples of it long, so sub-passes are frames [8 s, 8 s + 8) of a run

ALL_ON = dict(pos_thres=.2, neg_thres=.15, sigma_thres=.03, cutoff_hz=300, leak_rate_hz=.3, shot_noise_rate_hz=3.0,
              leak_jitter_fraction=0.1, refractory_period_s=0.0005)


def _clip(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 256, size=(H, W))
    frames = []
    for i in range(n):
        if i % 7 == 3:
            base = rng.integers(0, 256, size=(H, W))  # large jumps: many events per pixel, the refractory rule on
        else:
            base = np.clip(base + rng.integers(-14, 15, size=(H, W)), 0, 255)
        f = base.astype(np.uint8)
        f[:, 0] = 0
        f[:, 1] = 255
        f[:, 2] = 255 if i % 2 else 0
        f[-1, 3:] |= 1  # the last row is non-zero right up to pixel npx - 1
        frames.append(f)
    dts = rng.uniform(0.0004, 0.006, size=n)
    times = list(np.cumsum(dts) + 0.001)
    return np.stack(frames), times


def _oracle(oracle_lib, kw, frames, times, seed=7, clip=0):
    """events per frame, planes, and the shot decisions of the run's frames as [frame][pixel] arrays (ON, OFF)"""
    ora = oracle_lib.OracleEmulator(seed=seed, rng_mode="philox", clip=clip, **kw)
    oev, son, soff = [], [], []
    for f, t in zip(frames, times):
        oev.append(ora.generate_events(f, t))
        if ora.last:
            son.append(ora.last["shot_on"].reshape(-1).copy())
            soff.append(ora.last["shot_off"].reshape(-1).copy())
    return ora, oev, np.stack(son) != 0, np.stack(soff) != 0


def _hip(kw, frames, times, fused, monkeypatch, seed=7):
    from v2e_amd import EventEmulator
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "1" if fused else "0")
    emu = EventEmulator(device="cuda", seed=seed, rng_mode="philox", max_iters=1024, **kw)
    ev, counts = emu.generate_events_batch(frames, times, use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    assert emu._engine.last_pipeline()[0] == ("k_chain(fused records)" if fused else "k_chain")
    planes = [emu.base_log_frame.cpu().numpy(), emu.lp_log_frame.cpu().numpy()]
    if emu.timestamp_mem is not None:
        planes.append(emu.timestamp_mem.cpu().numpy())
    return ev, list(counts), planes


def _check(kw, frames, times, ora, oev, monkeypatch, hip_frames=None):
    ocounts = [0 if e is None else len(e) for e in oev]
    assert sum(ocounts) > 0
    oplanes = [ora.base_log_frame, ora.lp_log_frame]
    if kw.get("refractory_period_s", 0) > 0:
        oplanes.append(ora.timestamp_mem)
    ref = np.concatenate([e for e in oev if e is not None])
    runs = {fused: _hip(kw, frames if hip_frames is None else hip_frames, times, fused, monkeypatch) for fused in (False, True)}
    for fused, (ev, counts, planes) in runs.items():
        tag = "fused" if fused else "k_ahead records"
        assert counts == ocounts, tag
        assert np.array_equal(ev, ref), tag
        for a, b in zip(planes, oplanes):
            assert np.array_equal(a, b), tag
    assert np.array_equal(runs[False][0], runs[True][0])


def test_dense_shot_noise_reaches_the_partial_wave(oracle_lib, monkeypatch):
    kw = dict(ALL_ON, shot_noise_rate_hz=40.0)
    frames, times = _clip(75, seed=21)  # two full 32-frame launches and a partial one
    ora, oev, son, soff = _oracle(oracle_lib, kw, frames, times)
    assert son[:, LAST_WAVE:].any() and soff[:, LAST_WAVE:].any()  # both polarities among pixels 1216 .. 1220
    _check(kw, frames, times, ora, oev, monkeypatch)


def test_sparse_shot_noise_takes_both_sides_of_the_sub_pass_test(oracle_lib, monkeypatch):
    """Some (wave, 8-frame sub-pass) pairs carry no shot bit at all -- nothing is decoded -- and others do, in the same launches."""
    kw = dict(ALL_ON, shot_noise_rate_hz=0.5)
    frames, times = _clip(75, seed=22)
    ora, oev, son, soff = _oracle(oracle_lib, kw, frames, times)
    any_bit = son | soff  # [run frame][pixel]
    nf = any_bit.shape[0]
    pad = np.zeros((nf, (NPX + 63) // 64 * 64), bool)
    pad[:, :NPX] = any_bit
    per = np.array([[pad[s:s + SUB, w * 64:(w + 1) * 64].any() for w in range(pad.shape[1] // 64)] for s in range(0, nf, SUB)])
    first_launch = per[:32 // SUB]  # both kinds within one launch
    assert first_launch.any() and not first_launch.all(), per.mean()
    assert 0.15 < per.mean() < 0.85, per.mean()
    _check(kw, frames, times, ora, oev, monkeypatch)


def test_refractory_heavy_redo_passes_restage_the_previous_launch(oracle_lib, monkeypatch):
    kw = dict(ALL_ON, refractory_period_s=0.004, shot_noise_rate_hz=20.0)
    frames, times = _clip(75, seed=23)
    ora, oev, son, soff = _oracle(oracle_lib, kw, frames, times)
    assert son.any() and soff.any()
    _check(kw, frames, times, ora, oev, monkeypatch)


def test_last_frame_at_the_end_of_its_allocation(oracle_lib, monkeypatch):
    """The run's frames as a device tensor sized exactly (the run itself is the slice from frame 1): behind pixel npx - 1 of the
    last frame there is nothing, and a padding lane that read the frame would read past it -- or, in any other frame, pick up
    the start of the next one."""
    kw = dict(ALL_ON, shot_noise_rate_hz=20.0)
    frames, times = _clip(41, seed=24)  # 40 run frames: a full launch and one sub-pass of another
    assert (frames[:, -1, 3:] != 0).all() and frames[-1, -1, -1] != 0
    ora, oev, _, _ = _oracle(oracle_lib, kw, frames, times)
    dev = torch.from_numpy(frames).cuda()
    assert dev.numel() == len(frames) * NPX and dev.is_contiguous()
    _check(kw, frames, times, ora, oev, monkeypatch, hip_frames=dev)


def test_ring_wrap_with_the_mask_plane(oracle_lib, monkeypatch):
    """200 frames in one blocking run: the ring of frame slots (three emission batches of 64) wraps, the mask plane with it."""
    kw = dict(ALL_ON, refractory_period_s=0.002, shot_noise_rate_hz=20.0)
    frames, times = _clip(200, seed=25)
    ora, oev, son, soff = _oracle(oracle_lib, kw, frames, times)
    assert (son | soff)[3 * 64:].any()  # shot events behind the wrap
    _check(kw, frames, times, ora, oev, monkeypatch)


def test_two_clips_on_k_ahead_records(oracle_lib, monkeypatch):
    """Two pixel arrays in one engine on the chain that reads k_ahead's records: the mask plane's clip stride."""
    from v2e_amd.emulator import EventEmulator
    from v2e_amd.engine import EmuEngine
    NC, F = 2, 41
    kw = dict(cutoff_hz=300, leak_rate_hz=0.2, shot_noise_rate_hz=30.0, refractory_period_s=0.0005)
    clips = [_clip(F, seed=30 + c)[0] for c in range(NC)]
    times = [i / 300 for i in range(F)]
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "0")
    proto = EventEmulator(device="cuda", seed=5, rng_mode="philox", **kw)
    proto._thres_scalar = (0.2, 0.2)
    proto._thres_is_scalar = False
    P = proto._params()
    eng = EmuEngine(H, W, n_clips=NC, device="cuda")
    eng.alloc_state(True)
    frames = torch.from_numpy(np.stack(clips, axis=1)).cuda()  # [F][NC][H][W]
    eng.init_state(P, frames[0].contiguous(), times[0])
    ev = eng.event_buffer(4 * H * W * F)
    recs = eng.alloc_recs(F - 1)
    t_prev = np.array([[0.0] * NC] + [[times[f]] * NC for f in range(1, F - 1)])
    t_frame = np.array([[times[f]] * NC for f in range(1, F)])
    eng.run(P, frames[1:].contiguous(), t_prev, t_frame, 1, ev, recs, use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    assert eng.last_pipeline()[0] == "k_chain"
    r = eng.recs_to_numpy(recs)
    assert not r["flags"].any()
    for c in range(NC):
        ora, oev, son, soff = _oracle(oracle_lib, kw, clips[c], times, seed=5, clip=c)
        assert son[:, LAST_WAVE:].any() or soff[:, LAST_WAVE:].any(), "clip %d" % c
        ref = np.concatenate([e for e in oev if e is not None])
        n = int(r["n_events"][:, c].sum())
        assert n == len(ref), "clip %d" % c
        assert np.array_equal(ev[c, :n].cpu().numpy(), ref), "clip %d" % c
        assert np.array_equal(eng.plane(eng.base, c).cpu().numpy(), ora.base_log_frame)
        assert np.array_equal(eng.plane(eng.ts_mem, c).cpu().numpy(), ora.timestamp_mem)
