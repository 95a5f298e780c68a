"""GPU parity of the chain's 16-bit count words (count in bits 0-12, saturating at 8191; sign, shot ON / OFF in bits 13-15)
against the CPU oracle, on the chain that reads k_ahead's records (V2E_AMD_CHAIN_FUSED=0) and on the one that builds its
records itself (=1).

33x37 pixels, scalar thresholds (sigma_thres=0), max_iters=1024.  One column steps 0 -> 255 -> 0; the threshold decides how
many events that is per pixel and frame (lin-log of 255 is about 5.54):
  hundreds   threshold 0.01:   counts above 255 (more than a byte) and below 1024
  saturated  threshold 0.0005: more than 8191 events -- the word saturates, the frame is refused as before
  near_max   threshold 0.0055: a frame just below max_iters, then ordinary frames: the state behind it is the oracle's
Every precondition is asserted from the oracle's own counts."""
import numpy as np
import pytest

from v2e_amd._capi import RUN_GRAPH, RUN_REQUIRE_CHAIN, V2EAmdError

pytestmark = pytest.mark.gpu

H, W = 33, 37
MAX_ITERS = 1024
COL = 5
KWS = {
    "plain": dict(cutoff_hz=0, leak_rate_hz=.1, shot_noise_rate_hz=2.0, refractory_period_s=0),
    "all_on": dict(cutoff_hz=300, leak_rate_hz=.3, shot_noise_rate_hz=3.0, refractory_period_s=0.0005),
}
THRES = {"hundreds": 0.01, "saturated": 0.0005, "near_max": 0.0055}


def _case(name, kwn):
    th = THRES[name]
    kw = dict(KWS[kwn], pos_thres=th, neg_thres=th, sigma_thres=0)
    rng = np.random.Generator(np.random.PCG64(5))
    n = 12
    col = [0, 0, 0, 255, 255, 255, 0, 0, 0, 255, 255, 0]  # the stepping column, frame by frame
    if name == "near_max":
        col = [0, 0, 255] + [255] * 9  # one large frame, ordinary frames behind it
        if kw["refractory_period_s"] > 0:
            # a refractory period the large frame's event spacing (4 ms / 1007) stays above: the rule would filter most of the
            # column's events and leave it firing just as hard in every frame behind
            kw["refractory_period_s"] = 1e-6
    frames = np.empty((n, H, W), np.uint8)
    for i in range(n):
        frames[i] = 120 + (rng.integers(0, 2, size=(H, W)) if i % 3 == 1 else 0)  # a grey level up and down: an event here and there
        frames[i, :, COL] = col[i]
    times = [0.001 + i / 250 for i in range(n)]
    return kw, frames, times


def _oracle(oracle_lib, kw, frames, times):
    ora = oracle_lib.OracleEmulator(seed=7, rng_mode="philox", **kw)
    evs, Ms = [], []
    for f, t in zip(frames, times):
        e = ora.generate_events(f, t)
        evs.append(e)
        Ms.append(0 if not ora.last else int(ora.last["M"]))
    return ora, evs, Ms


def _hip(kw, frames, times, fused, monkeypatch):
    from v2e_amd import EventEmulator
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "1" if fused else "0")
    emu = EventEmulator(device="cuda", seed=7, rng_mode="philox", max_iters=MAX_ITERS, **kw)
    ev, counts = emu.generate_events_batch(frames, times, use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    assert emu._engine.last_pipeline()[0] == ("k_chain(fused records)" if fused else "k_chain")
    planes = [emu.base_log_frame.cpu().numpy(), emu.lp_log_frame.cpu().numpy()]
    if emu.timestamp_mem is not None:
        planes.append(emu.timestamp_mem.cpu().numpy())
    return ev, list(counts), planes


def _check_exact(oracle_lib, kw, frames, times, monkeypatch, ora, evs):
    ref = np.concatenate([e for e in evs if e is not None])
    ocounts = [0 if e is None else len(e) for e in evs]
    oplanes = [ora.base_log_frame, ora.lp_log_frame]
    if kw["refractory_period_s"] > 0:
        oplanes.append(ora.timestamp_mem)
    for fused in (False, True):
        ev, counts, planes = _hip(kw, frames, times, fused, monkeypatch)
        tag = "fused" if fused else "k_ahead records"
        assert counts == ocounts, tag
        assert np.array_equal(ev, ref), tag
        for a, b in zip(planes, oplanes):
            assert np.array_equal(a, b), tag


@pytest.mark.parametrize("kwn", list(KWS))
def test_counts_in_the_hundreds_match_oracle(kwn, oracle_lib, monkeypatch):
    kw, frames, times = _case("hundreds", kwn)
    ora, evs, Ms = _oracle(oracle_lib, kw, frames, times)
    assert 255 < max(Ms) < MAX_ITERS, Ms  # more than a byte, accepted by the emission
    assert sum(1 for m in Ms if m > 255) >= 3, Ms  # steps of both signs
    _check_exact(oracle_lib, kw, frames, times, monkeypatch, ora, evs)


@pytest.mark.parametrize("kwn", list(KWS))
@pytest.mark.parametrize("fused", [False, True])
def test_saturated_count_is_refused_as_before(kwn, fused, oracle_lib, monkeypatch):
    kw, frames, times = _case("saturated", kwn)
    _, _, Ms = _oracle(oracle_lib, kw, frames, times)
    assert max(Ms) > 8191, Ms  # beyond what the 13-bit count holds
    with pytest.raises(V2EAmdError, match="more than max_iters"):
        _hip(kw, frames, times, fused, monkeypatch)


@pytest.mark.parametrize("kwn", list(KWS))
def test_state_behind_a_frame_just_below_max_iters(kwn, oracle_lib, monkeypatch):
    kw, frames, times = _case("near_max", kwn)
    ora, evs, Ms = _oracle(oracle_lib, kw, frames, times)
    big = int(np.argmax(Ms))
    assert MAX_ITERS - 64 <= Ms[big] <= MAX_ITERS - 1, Ms
    assert big + 6 <= len(Ms) and max(Ms[big + 1:]) < 64, Ms  # ordinary frames behind it
    _check_exact(oracle_lib, kw, frames, times, monkeypatch, ora, evs)
