"""CPU checks of the scripted clips and the replay that tests/test_chain_redo_gpu.py uses on k_chain's rule-on rows: the
clips reach the redo cases they are there for (by the oracle alone, so that an edit to a schedule cannot quietly lose
one), and the replay of the round decisions agrees with the protocol model of tests/test_chain_protocol_model.py."""
import numpy as np
import pytest

import chain_redo as cr
from test_chain_protocol_model import Toy, chain


@pytest.mark.parametrize("name", sorted(cr.SCENARIOS))
def test_scripted_clip_reaches_its_cases(name, oracle_lib):
    sc = cr.SCENARIOS[name]
    frames, times = cr.scenario_clip(sc)
    model = cr.oracle_model(oracle_lib, frames, times, cr.KW, sc["K"], seed=cr.SEED)
    cov = cr.model_coverage(model)
    assert cr.MODEL_CASES[name] <= cov, "clip %s no longer reaches %s" % (name, sorted(cr.MODEL_CASES[name] - cov))
    # row 0 of a launch flags nothing before the launch's first true rule-on frame, and flags that one with its true M
    for L, (f0, nf, _, _) in enumerate(model["plan"]):
        r0, tr = model["row0"][L][:nf], model["true"][f0:f0 + nf]
        assert not model["row0"][L][nf:].any()
        on = np.nonzero(tr)[0]
        if on.size:
            assert not r0[:on[0]].any() and r0[on[0]] == tr[on[0]], (name, L)
        else:
            assert not r0.any(), (name, L)


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 11, 16, 32])
@pytest.mark.parametrize("mon", [2, 4, 7])
def test_replay_follows_the_protocol_model(K, mon):
    """replay() on the toy protocol's rule-on rows takes the toy's redo passes: the same first disagreeing frames, in the same
    order, with the same checkpoint restarts; its final decisions are the frames' true M where the rule is on."""
    for seed in range(6):
        rng = np.random.default_rng(100 * K + 10 * mon + seed)
        npx, F = 37, int(rng.integers(1, 75))
        toy = Toy(npx, mon, seed)
        drift = np.cumsum(rng.integers(0, 12, (F, 1)), axis=0)
        frames = (drift + rng.integers(0, 30, (F, npx))).astype(np.int64)
        trace = {}
        chain(toy, frames, K, checkpoints=True, predict=True, lockstep=False, trace=trace)
        plan = cr.chain_plan(F, K)
        rep = cr.replay(trace["rows"], plan, K)
        got = [(d["L"], r["j"], r["c0"]) for d in rep for r in d["rounds"]]
        assert got == trace.get("passes", []), (K, mon, seed)
        # the decisions: the toy's M where the rule is on, frame by frame (sequential processing)
        base, ts = toy.base0.copy(), toy.ts0.copy()
        true = []
        for f, x in enumerate(frames):
            c = toy.count(base, x)
            m = int(c.max())
            true.append(m if m >= toy.mon else 0)
            base, ts, _ = toy.finalise(base, ts, c, f, true[-1])
        for d in rep:
            assert np.array_equal(d["decision"], true[d["pf0"]:d["pf0"] + d["pnf"]]), (K, mon, seed, d["L"])
