"""k_chain's redo passes (v2e_amd/csrc/emu_chain.h) on scripted clips whose rule-on frames are placed on purpose
(tests/chain_redo.py), checked against the CPU oracle AND against a model of the rule-on rows the device leaves
(EmuEngine.debug_chain_rows):

* parity: events in order, final planes, event totals bit-exact with the oracle;
* row 0 of every launch (its own pass, speculating "rule off" throughout: the light frame body, with its rule-on maxima
  published in one batch per sub-pass) equals a rule-off replay of the oracle from the launch's first frame;
* the redo rounds replayed from the device's rows settle every launch on the true rule-on decisions, write nothing where
  they must not, and take the first two decisions the CPU model predicts;
* the rows of the records-from-k_ahead chain (light and general frame bodies) equal those of the fused chain (general
  body only) bit for bit -- including the entries computed from mispredicted state, which no CPU model gives;
* every clip still reaches the redo cases it is there for, asserted from the device's rows.
"""
import functools

import numpy as np
import pytest
import torch

import chain_redo as cr
from v2e_amd._capi import RUN_GRAPH, RUN_REQUIRE_CHAIN

pytestmark = pytest.mark.gpu

MODES = [RUN_REQUIRE_CHAIN | RUN_GRAPH, RUN_REQUIRE_CHAIN]

# what the replayed device rows of each clip must show (chain_redo.coverage)
DEVICE_CASES = {
    "k8": {"j_offset0", "j_frame0", "j_partial_sub", "no_rendezvous", "rendezvous", "c0=0", "false_negative", "false_positive",
           "wrong_value", "rounds>=3", "tail_redo_last_frame_on"},
    "k11": {"j_offset7_rule_on", "j_partial_sub", "c0=0", "c0>0", "mixed_light_general", "false_negative", "rounds>=3",
            "tail_redo_last_frame_on"},
    "k32": {"j_offset0", "c0>0", "no_rendezvous", "mixed_light_general", "rounds>=3", "tail_redo_last_frame_on"},
    "ragged": {"j_frame0", "j_partial_sub", "tail_redo_last_frame_on"},
    "hd": {"j_offset7_rule_on", "c0>0", "mixed_light_general"},
}


@functools.lru_cache(maxsize=None)
def _model(name):
    from oracle import oracle as orc
    sc = cr.SCENARIOS[name]
    frames, times = cr.scenario_clip(sc)
    return frames, times, cr.oracle_model(orc, frames, times, cr.KW, sc["K"], seed=cr.SEED)


def _run(frames, times, K, fused, mode, monkeypatch, kw=cr.KW):
    """One blocking device-resident run on a fresh emulator (a second run on the same one would take one frame per launch:
    the rule is on in more than 5 % of these frames).  Returns (emulator, events, rule-on rows, records)."""
    from v2e_amd import EventEmulator
    monkeypatch.setenv("V2E_AMD_CHAIN_K", str(K))
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "1" if fused else "0")
    emu = EventEmulator(device="cuda", seed=cr.SEED, rng_mode="philox", **kw)
    ev, _ = emu.generate_events_batch(frames, times, use_graph=mode)
    eng = emu._engine
    kind, fpl, _ = eng.last_pipeline()
    assert kind == ("k_chain(fused records)" if fused else "k_chain") and fpl == K
    rows = eng.debug_chain_rows()
    recs = eng.recs_to_numpy(eng.alloc_recs(len(frames) - 1, 2))
    return emu, ev, rows, recs


def _check_parity(emu, ev, recs, model):
    from v2e_amd._capi import FLAG_SYNC_TIMEOUT
    assert not (recs["flags"] & FLAG_SYNC_TIMEOUT).any() and not recs["flags"].any()
    ref = model["events"]
    assert ev is not None and ev.shape == ref.shape and np.array_equal(ev, ref), "events differ from the oracle"
    assert np.array_equal(emu.base_log_frame.cpu().numpy(), model["base"])
    assert np.array_equal(emu.lp_log_frame.cpu().numpy(), model["lp"])
    assert np.array_equal(emu.timestamp_mem.cpu().numpy(), model["ts"])
    assert (emu.num_events_total, emu.num_events_on, emu.num_events_off) == tuple(model["counters"])


def _check_rows(rows, model, K, fused):
    """rows [launches][K + 1][K] of one clip against the CPU model; returns the replay."""
    plan = model["plan"]
    assert rows.shape == (len(plan), K + 1, K)
    # row 0: the own pass of every launch, exactly (zero beyond a launch's frames; the tail launch has no own pass)
    assert np.array_equal(rows[:, 0].astype(np.int64), model["row0"]), "row 0 differs from the rule-off replay"
    assert not rows[-1].any(), "the tail launch's rows are never written"
    rep = cr.replay(rows.astype(np.int64), plan, K, fused=fused)
    decisions = {d["L"]: d for d in cr.model_decisions(model)}
    for d in rep:
        R = rows[d["L"] - 1]
        assert d["settle"] <= K
        assert not R[d["settle"] + 1:].any(), "a row was written after the launch settled (L=%d)" % d["L"]
        for i, r in enumerate(d["rounds"]):  # row i + 1 is written by redo pass i + 1, on the frames after its j only
            assert not R[i + 1][:r["j"] + 1].any(), "redo pass %d on launch %d published frames <= j" % (i + 1, d["L"] - 1)
        true = model["true"][d["pf0"]:d["pf0"] + d["pnf"]]
        assert np.array_equal(d["decision"], true), "launch %d settled on %s, true %s" % (d["L"] - 1, d["decision"], true)
        m = decisions[d["L"]]
        js = [r["j"] for r in d["rounds"]] + [None, None]
        assert (js[0], js[1]) == (m["j1"], m["j2"]), (d["L"], js, m)
        if m["j1"] is not None:
            assert d["rounds"][0]["row_v"] == m["v1"]
        if m["j2"] is not None:
            assert (d["rounds"][1]["pred_j"], d["rounds"][1]["row_v"]) == (m["pred2"], m["v2"])
    return rep


@pytest.mark.parametrize("mode", MODES, ids=["graph", "plain"])
@pytest.mark.parametrize("name", ["k8", "k11", "k32", "ragged", "hd"])
def test_redo_passes_match_oracle_and_row_model(name, mode, monkeypatch):
    sc = cr.SCENARIOS[name]
    K = sc["K"]
    frames, times, model = _model(name)
    rows = {}
    for fused in (False, True):
        emu, ev, rw, recs = _run(frames, times, K, fused, mode, monkeypatch)
        _check_parity(emu, ev, recs, model)
        assert rw is not None and rw.shape[2] == 1
        rows[fused] = rw[:, :, 0, :]
        rep = _check_rows(rows[fused], model, K, fused)
        del emu
        if not fused:
            cov = cr.coverage(rep, K, len(frames) - 1)
            assert DEVICE_CASES[name] <= cov, "clip %s did not reach %s on the device" % (name, sorted(DEVICE_CASES[name] - cov))
    # light + general bodies (k_ahead's records) against the general body alone (fused records): the same arithmetic, so
    # every published maximum -- also those of frames a redo pass ran under a wrong prediction -- is the same
    assert np.array_equal(rows[False], rows[True]), "the light frame body published other maxima than the general one"


def test_multi_clip_rows_equal_single_clip_runs(monkeypatch):
    """Three clips in one EmuEngine, each with its own schedule and frame interval (so its own rule threshold; clip 2's is never
    reached): each clip's rule-on rows equal those of a run of that clip alone, and its events the oracle's.  (No random draw
    moves a count here -- scalar thresholds, no leak jitter or rate spread, no shot noise -- so a single-clip run, whose Philox
    stream is clip 0's, flags what the clip flags inside the engine.)"""
    from oracle import oracle as orc
    from v2e_amd.emulator import EventEmulator
    from v2e_amd.engine import EmuEngine
    K, H, W, F = 8, 48, 80, 42
    kw = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.0, cutoff_hz=200.0, leak_rate_hz=0.1, leak_jitter_fraction=0.0,
              noise_rate_cov_decades=0.0, shot_noise_rate_hz=0.0, refractory_period_s=0.0008)
    fps = (300.0, 200.0, 100.0)  # rule on from M >= 5, M >= 7, M >= 13 (a 40 -> 200 step fires 8)
    events = [[(3, 200), (15, 40), (23, 200), (40, 40)], [(7, 200), (8, 40), (20, 200), (33, 40)], [(5, 200), (30, 40)]]
    clips, times = [], []
    for c in range(3):
        fr = cr.scripted_clip(H, W, F, [(6, 10, 12, 40, cr.schedule(F, [(r + 1, lv) for r, lv in events[c]]))], seed=10 + c)
        clips.append(fr)
        times.append([i / fps[c] for i in range(F)])
    monkeypatch.setenv("V2E_AMD_CHAIN_K", str(K))
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "0")
    proto = EventEmulator(device="cuda", seed=cr.SEED, rng_mode="philox", **kw)
    proto._thres_scalar = (0.2, 0.2)
    proto._thres_is_scalar = True
    P = proto._params()
    eng = EmuEngine(H, W, n_clips=3, device="cuda")
    eng.alloc_state(True)
    frames = torch.from_numpy(np.stack(clips, axis=1)).cuda()  # [F][3][H][W]
    eng.init_state(P, frames[0].contiguous(), 0.0)
    ev = eng.event_buffer(4 * H * W * F)
    recs = eng.alloc_recs(F - 1)
    t_prev = np.array([[0.0] * 3] + [[times[c][f] for c in range(3)] for f in range(1, F - 1)])
    t_frame = np.array([[times[c][f] for c in range(3)] for f in range(1, F)])
    eng.run(P, frames[1:].contiguous(), t_prev, t_frame, 1, ev, recs, use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    assert eng.last_pipeline()[:2] == ("k_chain", K)
    r = eng.recs_to_numpy(recs)
    assert not r["flags"].any()
    rows = eng.debug_chain_rows()
    assert rows is not None and rows.shape[1:] == (K + 1, 3, K)
    for c in range(3):
        model = cr.oracle_model(orc, clips[c], times[c], kw, K, seed=cr.SEED, clip=c)
        n = int(r["n_events"][:, c].sum())
        assert n == len(model["events"]) and np.array_equal(ev[c, :n].cpu().numpy(), model["events"]), "clip %d" % c
        assert np.array_equal(eng.plane(eng.base, c).cpu().numpy(), model["base"])
        assert np.array_equal(eng.plane(eng.ts_mem, c).cpu().numpy(), model["ts"])
        _check_rows(rows[:, :, c, :], model, K, False)
        if c == 2:
            assert not model["true"].any() and not rows[:, :, c, :].any()
        else:
            assert model["true"].any()
        _, _, single, srecs = _run(clips[c], times[c], K, False, RUN_REQUIRE_CHAIN | RUN_GRAPH, monkeypatch, kw=kw)
        assert np.array_equal(rows[:, :, c, :], single[:, :, 0, :]), "clip %d: rows differ from its single-clip run" % c
