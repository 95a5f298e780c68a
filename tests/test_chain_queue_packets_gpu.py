"""Pipelined device-resident runs hand their chain over through STOP EVENTS (v2e_amd/csrc/emu_chain_host.h): what used to be an
event record on the caller's stream behind a k_chain launch -- the emission batch the launch makes final, the run's end, what
k_ahead waits for where the ring wraps -- is the stop event of that launch (hipExtLaunchKernel).  Checked here:

* the same events, per-frame counts and final state planes as the CPU oracle and as the blocking one-graph run, bit for bit,
  on clips whose rule-on frames (redo passes, `tsold` / `ruleM` of held-back events) sit on the launch and batch boundaries;
* what the schedule puts on the caller's stream (v2e_emu_last_run_queue_ops): launches and one wait, no record;
* runs in flight on one handle, results read in either order (the handle's events re-used run after run, the host waiting on a
  stop event);
* a ring of three batches (V2E_AMD_CHAIN_RING=3), where chain and k_ahead wait for one another batch by batch;
* the chain that builds its own records (V2E_AMD_CHAIN_FUSED=1).

33x37 frames (1 221 pixels: five workgroups, the last one ragged), the v2e CLI's default DVS parameters with its refractory
period, 300 frames/s: the rule is on from 7 events per pixel and frame, which a patch stepping between grey levels 40 and 200
reaches on the frame of the step; two patches stepping on consecutive frames give rule-on frames on both sides of a boundary.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import chain_redo as cr

pytestmark = pytest.mark.gpu

H, W, FPS, K, E = 33, 37, 300.0, 32, 64
KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=300.0, leak_rate_hz=0.01, shot_noise_rate_hz=0.001,
          refractory_period_s=0.0005)
SEED = 5
PATCHES = ((4, 5, 12, 20), (20, 5, 10, 20))  # y0, x0, h, w

# run frames at which each of the two patches steps (to 200, back to 40, ...): the rule is on in exactly those frames
CLIPS = {
    # 70 run frames = launches of 32, 32 and 6 frames and the tail, emission batches of 64 and 6: rule-on frames on both sides of
    # the first launch boundary and of the batch boundary, and in the partial launch the tail validates
    "two_launches": dict(n_run=70, steps=((31, 63), (32, 64, 67))),
    # three runs of 70: at most three rule-on frames each (beyond 5 % of a run's frames the next run takes one frame per launch);
    # the last run's last frame is one of them
    "three_runs": dict(n_run=210, steps=((31, 70 + 63, 140 + 66), (32, 70 + 64, 140 + 69))),
    # 300 run frames in a ring of three 64-frame batches: the ring wraps at run frame 192
    "ring": dict(n_run=300, steps=((62, 126, 191, 254), (63, 192, 297))),
}


@functools.lru_cache(maxsize=None)
def _clip(name):
    c = CLIPS[name]
    F = c["n_run"] + 1
    patches = []
    for patch, steps in zip(PATCHES, c["steps"]):
        lv, ev = 40, []
        for r in steps:
            lv = 200 if lv == 40 else 40
            ev.append((r + 1, lv))  # run frame r is the clip's frame r + 1
        patches.append(patch + (cr.schedule(F, ev),))
    frames = cr.scripted_clip(H, W, F, patches, seed=3)
    return frames, tuple(i / FPS for i in range(F))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The CPU oracle over the clip, frame by frame: events per frame, final planes, counters, rule-on flag per run frame."""
    from oracle import oracle as orc
    frames, times = _clip(name)
    ora = orc.OracleEmulator(seed=SEED, rng_mode="philox", **KW)
    per_frame, on = [], []
    for f in range(len(frames)):
        t_prev = float(ora.t_previous) if f else 0.0
        e = ora.generate_events(frames[f], times[f])
        per_frame.append(e if e is not None else np.zeros((0, 4), np.float32))
        if f:
            on.append(cr.rule_entry(ora.last_M, t_prev, times[f], KW["refractory_period_s"]) != 0)
    return dict(per_frame=per_frame, on=np.array(on), base=ora.base_log_frame.copy(), lp=ora.lp_log_frame.copy(),
                ts=ora.timestamp_mem.copy(), counters=(ora.num_events_total, ora.num_events_on, ora.num_events_off))


def _expect(model, f0, f1):
    """(events, counts) of the clip's frames [f0, f1) as one device-resident run returns them."""
    pf = model["per_frame"][f0:f1]
    return np.concatenate(pf), np.array([len(e) for e in pf], dtype=np.int64)


def _emulator():
    from v2e_amd import EventEmulator
    return EventEmulator(device="cuda", seed=SEED, rng_mode="philox", **KW)


def _check_final(emu, model):
    assert np.array_equal(emu.base_log_frame.cpu().numpy(), model["base"])
    assert np.array_equal(emu.lp_log_frame.cpu().numpy(), model["lp"])
    assert np.array_equal(emu.timestamp_mem.cpu().numpy(), model["ts"])
    assert (emu.num_events_total, emu.num_events_on, emu.num_events_off) == tuple(model["counters"])


def _plan_launches(n_run, ring, fused):
    from v2e_amd import _capi
    return int(_capi.lib().v2e_emu_chain_plan(n_run, K, E, ring, 1, int(fused), None, 0))


def test_clips_put_rule_on_frames_on_the_boundaries():
    """The clips are what the tests below need them to be (the oracle's own rule-on frames)."""
    for name, c in CLIPS.items():
        on = np.nonzero(_oracle(name)["on"])[0].tolist()
        assert on == sorted(c["steps"][0] + c["steps"][1]), "%s: the rule is on in run frames %s" % (name, on)
    on = _oracle("two_launches")["on"]
    assert on[31] and on[32], "rule-on frames on both sides of the first launch boundary"
    assert on[63] and on[64], "... and of the boundary of the first emission batch"
    assert on[67], "... and in the partial launch the tail validates"
    on = _oracle("three_runs")["on"]
    for k in range(3):
        n = int(on[70 * k:70 * (k + 1)].sum())
        assert 1 <= n <= 3, "run %d: %d rule-on frames (the next run keeps 32 frames per launch up to 5 %%)" % (k, n)
    on = _oracle("ring")["on"]
    assert on[191] and on[192], "rule-on frames on both sides of the ring's wrap"


def _pipelined_against_oracle_and_graph(name, ring, fused):
    frames, times = _clip(name)
    n_run = len(frames) - 1
    model = _oracle(name)
    ref_ev, ref_counts = _expect(model, 0, len(frames))
    emu = _emulator()
    pend = emu.generate_events_batch_async(frames, times, use_graph=0)
    eng = emu._engine
    assert eng.last_pipeline() == ("k_chain(fused records)" if fused else "k_chain", K, E)
    assert pend.ticket is not None, "the run went out in pieces (pipelined)"
    ops = eng.last_run_queue_ops()
    ev, counts = pend.result()
    assert ev.shape == ref_ev.shape and np.array_equal(ev, ref_ev), "events differ from the oracle"
    assert np.array_equal(counts, ref_counts)
    _check_final(emu, model)
    blk = _emulator()
    ev_g, counts_g = blk.generate_events_batch(frames, times, use_graph=1)  # (1, not True: one graph, also for a first run)
    ops_g = blk._engine.last_run_queue_ops()
    assert np.array_equal(ev, ev_g) and np.array_equal(counts, counts_g), "pipelined and one-graph runs differ"
    _check_final(blk, model)
    return ops, ops_g, _plan_launches(n_run, ring, fused)


def test_parity_over_two_launches_and_a_tail_and_queue_operations():
    ops, ops_g, n_launch = _pipelined_against_oracle_and_graph("two_launches", 5, False)
    assert n_launch == 4
    launches, waits, records = ops
    assert records == 0, "a record on the caller's stream"
    assert launches == n_launch, "the caller's stream carries the chain's launches and nothing else"
    assert waits <= 1
    # The captured run, as before (enqueue_run_chain, ring of 3, K = 32, E = 64, 70 frames: 4 chain launches, m = 2, 2 batches):
    #   launches  the zero fill + 4 chain launches
    #   records   the fork, EV_CHAIN behind launches 0 and 2, EV_FORK behind launches 2 and 3 (batches 0 and 1)
    #   waits     EV_AHEAD of batches 0 and 1, the rest of batch 0 before launch 1, and the join: the last rows, the last k_ahead
    assert ops_g == (5, 5, 5)


def test_queue_operations_with_resident_frames():
    """The benchmark's call (frames_resident=True): the schedule's count is the whole of what the run puts on the stream."""
    frames, times = _clip("two_launches")
    emu = _emulator()
    pend = emu.generate_events_batch_async(frames, times, use_graph=0, frames_resident=True)
    assert emu._engine.last_run_queue_ops() == (4, 1, 0)
    ev, _ = pend.result()
    assert np.array_equal(ev, _expect(_oracle("two_launches"), 0, len(frames))[0])


@pytest.mark.parametrize("reverse", [False, True], ids=["read_in_order", "read_last_two_reversed"])
def test_two_runs_in_flight(reverse):
    frames, times = _clip("three_runs")
    model = _oracle("three_runs")
    cuts = [(0, 71), (71, 141), (141, 211)]
    emu = _emulator()
    eng_ops = []

    def enqueue(k):
        f0, f1 = cuts[k]
        p = emu.generate_events_batch_async(frames[f0:f1], list(times[f0:f1]), use_graph=0, frames_resident=True)
        assert emu._engine.last_pipeline() == ("k_chain", K, E), "run %d fell back to another launch length" % k
        eng_ops.append(emu._engine.last_run_queue_ops())
        return p

    p = [enqueue(0), enqueue(1)]
    res = {0: p[0].result()}
    p.append(enqueue(2))  # (the benchmark's order: the next run is enqueued before the previous result is read)
    for k in ((2, 1) if reverse else (1, 2)):
        res[k] = p[k].result()
    assert eng_ops == [(4, 1, 0)] * 3
    blk = _emulator()
    for k, (f0, f1) in enumerate(cuts):
        ref_ev, ref_counts = _expect(model, f0, f1)
        ev_b, counts_b = blk.generate_events_batch(frames[f0:f1], list(times[f0:f1]))
        assert np.array_equal(res[k][0], ev_b) and np.array_equal(res[k][1], counts_b), "run %d differs from the blocking run" % k
        assert np.array_equal(res[k][0], ref_ev) and np.array_equal(res[k][1], ref_counts), "run %d differs from the oracle" % k
    _check_final(emu, model)
    _check_final(blk, model)


def test_ring_wrap(monkeypatch):
    monkeypatch.setenv("V2E_AMD_CHAIN_RING", "3")
    frames, times = _clip("ring")
    model = _oracle("ring")
    emu = _emulator()
    pend = emu.generate_events_batch_async(frames, times, use_graph=0)
    eng = emu._engine
    assert eng.last_pipeline() == ("k_chain", K, E)
    # 300 frames in a ring of 192: k_ahead goes out batch by batch and the chain waits for it (5 batches), for the run's head, and
    # for the emission of batches 0 and 1 before it overwrites their slots -- and still records nothing
    plan = np.zeros((16, 8), np.int32)
    from v2e_amd import _capi
    n = _capi.lib().v2e_emu_chain_plan(300, K, E, 3, 1, 0, plan.ctypes.data_as(C.c_void_p), 16)
    assert n == 11 and (plan[:n, 4] >= 0).sum() == 2 and (plan[:n, 5] >= 0).sum() == 5
    assert eng.last_run_queue_ops() == (11, 1 + 2 + 5, 0)
    ev, counts = pend.result()
    ref_ev, ref_counts = _expect(model, 0, len(frames))
    assert ev.shape == ref_ev.shape and np.array_equal(ev, ref_ev), "events differ from the oracle"
    assert np.array_equal(counts, ref_counts)
    _check_final(emu, model)


def test_fused_chain(monkeypatch):
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "1")
    ops, _, n_launch = _pipelined_against_oracle_and_graph("two_launches", 5, True)
    assert ops == (n_launch, 1, 0)
