"""Scripted clips, a CPU model and a replay of k_chain's redo decisions (v2e_amd/csrc/emu_chain.h), for the tests of its
redo passes (tests/test_chain_redo_model.py on the CPU, tests/test_chain_redo_gpu.py on the device).

The refractory rule (emulator.py:830) couples the frames of a clip through one number per frame, the max event count M.
k_chain advances K frames per launch assuming the rule is off; the rule-on rows it leaves ([launch][K + 1][n_clips][K]:
row 0 what a launch's own pass flagged, row r what the r-th redo pass on that launch flagged) say which redo passes the
next launch took.  Here:

* `scripted_clip` builds a quiet clip with patches whose grey level follows a per-frame schedule, so that rule-on frames
  land where a test wants them;
* `oracle_model` runs the CPU oracle over it and gives what the device must produce: the events, the final planes, the
  true rule-on entry of every frame, and row 0 of every launch (a rule-off replay of a deep copy of the oracle taken at
  the launch's first frame: exactly what the launch's own pass computes);
* `replay` restates the kernel's round decisions (emu_chain.h, the pass loop of k_chain) on a launch's rows.

Frames are run-relative: run frame r is the clip's frame r + 1 (the clip's first frame only initialises the state).
"""
import copy
import ctypes as C

import numpy as np

CHAIN_SUB = 8   # frames of a k_chain sub-pass (emu_chain.h)
BACKGROUND = 100


def scripted_clip(H, W, F, patches, seed=0, noise=2):
    """uint8 frames [F][H][W]: a flat background with +-`noise` grey levels of independent noise per pixel and frame, and
    patches (y0, x0, h, w, schedule) whose level is schedule[f] on frame f (a sequence of F levels)."""
    rng = np.random.default_rng(seed)
    fr = BACKGROUND + rng.integers(-noise, noise + 1, size=(F, H, W))
    for (y0, x0, h, w, sched) in patches:
        sched = np.asarray(sched)
        assert len(sched) == F, "a schedule gives one level per frame"
        fr[:, y0:y0 + h, x0:x0 + w] = sched[:, None, None] + rng.integers(-noise, noise + 1, size=(F, min(h, H - y0), min(w, W - x0)))
    return np.clip(fr, 0, 255).astype(np.uint8)


def schedule(F, events, base=40):
    """A patch schedule of F frames: `base` everywhere, then each (frame, level) of `events` holds from that frame on."""
    s = np.full(F, base, np.int64)
    for f, lv in sorted(events):
        s[f:] = lv
    return s


def rule_entry(M, t_prev, t_frame, refr):
    """What a rule-on row holds for a frame whose max count is M: M where the refractory rule is on (emulator.py:830,
    `refractory_period_s > delta_time / M`, in float64 -- the predicate behind FrameCtl::refr_on_n), else 0."""
    M = int(M)
    if M <= 0:
        return 0
    return M if float(refr) > (float(t_frame) - float(t_prev)) / float(M) else 0


def chain_plan(n_frames, K):
    """v2e_emu_chain_plan's launches of a refractory run, as (f0, nf, pf0, pnf) per launch (the last one the tail launch)."""
    from v2e_amd import _capi
    lib = _capi.lib()
    n = lib.v2e_emu_chain_plan(n_frames, K, K, 3, 1, 0, None, 0)
    buf = (C.c_int32 * (8 * n))()
    assert lib.v2e_emu_chain_plan(n_frames, K, K, 3, 1, 0, buf, n) == n
    plan = np.frombuffer(buf, dtype=np.int32).reshape(n, 8)
    return [tuple(int(v) for v in row[:4]) for row in plan]


def oracle_model(orc, frames, times, kw, K, seed=5, clip=0):
    """The CPU oracle over a clip (Philox mode): a dict with
      events, counters (total, on, off), base / lp / ts (final planes)
      M [n_run], true [n_run]   max count and true rule-on entry of every run frame
      row0 [launches][K]        row 0 of every launch: its own pass, rule off from the exact state at its first frame
      plan                      (f0, nf, pf0, pnf) per launch
    """
    refr = float(kw["refractory_period_s"])
    n_run = len(frames) - 1
    plan = chain_plan(n_run, K)
    starts = {f0: L for L, (f0, nf, _, _) in enumerate(plan) if nf > 0}
    ora = orc.OracleEmulator(seed=seed, rng_mode="philox", clip=clip, **kw)
    ora.generate_events(frames[0], times[0])
    evs, M, true, tp = [], np.zeros(n_run, np.int64), np.zeros(n_run, np.int64), np.zeros(n_run)
    row0 = np.zeros((len(plan), K), np.int64)
    for r in range(n_run):
        if r in starts:  # the launch's own pass: the same frames from here with the rule off
            L = starts[r]
            f0, nf = plan[L][:2]
            snap = copy.deepcopy(ora)
            snap.refractory_period_s = 0.0
            for k in range(nf):
                t_prev = float(snap.t_previous)
                snap.generate_events(frames[f0 + k + 1], times[f0 + k + 1])
                row0[L, k] = rule_entry(snap.last_M, t_prev, times[f0 + k + 1], refr)
        tp[r] = float(ora.t_previous)
        e = ora.generate_events(frames[r + 1], times[r + 1])
        if e is not None:
            evs.append(e)
        M[r] = ora.last_M
        true[r] = rule_entry(ora.last_M, tp[r], times[r + 1], refr)
    events = np.concatenate(evs) if evs else np.zeros((0, 4), np.float32)
    return dict(events=events, counters=(ora.num_events_total, ora.num_events_on, ora.num_events_off),
                base=ora.base_log_frame, lp=ora.lp_log_frame, ts=ora.timestamp_mem, M=M, true=true, row0=row0, plan=plan,
                K=K)


def replay(rows, plan, K, fused=False):
    """k_chain's round decisions (emu_chain.h, the pass loop) on one clip's rule-on rows [launches][K + 1][K]: for every
    launch that validates a predecessor, a dict
      L, pf0, pnf           the launch and the frames it validates (launch L - 1's)
      rounds                one dict per redo pass: j (first disagreeing frame), exact_v / pred_v (the values the row
                            was checked against and the values the pass runs under), row_v (row[j], M(j) exact), c0
                            (checkpoint restart), rendezvous (a check follows), light (per sub-pass of the pass: the
                            light frame body?)
      settle                the round whose row agreed with its predictions
      decision              the M every frame of launch L - 1 was finally taken under (0: rule off)
    """
    out = []
    ck = K > CHAIN_SUB  # mid-launch checkpoints exist (ChainArgs::ckp_base)
    for L, (f0, nf, pf0, pnf) in enumerate(plan):
        if pnf <= 0:
            continue
        R = rows[L - 1]
        exact = np.zeros(K, np.int64)
        pred = np.zeros(K, np.int64)
        last_exact, rnd, rounds = -1, 0, []
        lanes = np.arange(K)
        while True:
            gv = np.where(lanes < pnf, R[rnd], 0).astype(np.int64)
            hit = np.nonzero((gv != pred) & (lanes > last_exact))[0]
            if hit.size == 0:
                break
            j = int(hit[0])
            pred_j = int(pred[j])
            exact = np.where(lanes > last_exact, gv, exact)
            pred = np.where(lanes > j, gv, 0)
            last_exact = j
            rnd += 1
            c0 = (j // CHAIN_SUB) * CHAIN_SUB if ck else 0
            light = [] if fused else [(k0, not exact[k0:k0 + CHAIN_SUB].any()) for k0 in range(c0, pnf, CHAIN_SUB)]
            rounds.append(dict(j=j, exact_v=exact.copy(), pred_v=pred.copy(), pred_j=pred_j, row_v=int(gv[j]), c0=c0,
                               rendezvous=j < pnf - 1, light=light))
            assert rnd <= K, "more redo passes than frames"
        out.append(dict(L=L, pf0=pf0, pnf=pnf, rounds=rounds, settle=rnd, decision=exact[:pnf].copy()))
    return out


def model_decisions(model):
    """What the CPU model knows of every launch's first two redo decisions: per validating launch (j1, v1, j2, pred2, v2),
    None where that round does not happen.  j1: first frame row 0 flags; j2: first frame after it whose true entry differs
    from row 0 (the first redo pass runs the frames after j1 under row 0's values, from exact state up to j2)."""
    out = []
    for L, (f0, nf, pf0, pnf) in enumerate(model["plan"]):
        if pnf <= 0:
            continue
        r0 = model["row0"][L - 1][:pnf]
        tr = model["true"][pf0:pf0 + pnf]
        nz = np.nonzero(r0)[0]
        if nz.size == 0:
            out.append(dict(L=L, j1=None, j2=None))
            continue
        j1 = int(nz[0])
        assert tr[:j1].sum() == 0 and tr[j1] == r0[j1], "frames before the first flagged one are exact"
        d = np.nonzero(tr[j1 + 1:] != r0[j1 + 1:])[0]
        j2 = int(d[0]) + j1 + 1 if d.size else None
        out.append(dict(L=L, j1=j1, v1=int(r0[j1]), j2=j2, pred2=None if j2 is None else int(r0[j2]),
                        v2=None if j2 is None else int(tr[j2])))
    return out


def prediction_kind(pred, true):
    if pred == 0 and true != 0:
        return "false_negative"
    if pred != 0 and true == 0:
        return "false_positive"
    return "wrong_value" if pred != true else None


def coverage(rep, K, n_run):
    """The redo cases one clip's replayed rows reached, as a set of names (see test_chain_redo_gpu.py)."""
    cov = set()
    for d in rep:
        pnf = d["pnf"]
        if d["rounds"]:
            cov.add("redone")
        if d["settle"] >= 3:
            cov.add("rounds>=3")
        for i, r in enumerate(d["rounds"]):
            j, off = r["j"], r["j"] % CHAIN_SUB
            if off == 0:
                cov.add("j_offset0")
            if off == CHAIN_SUB - 1 and j // CHAIN_SUB < (pnf - 1) // CHAIN_SUB and r["row_v"] != 0:
                cov.add("j_offset7_rule_on")
            if j == 0:
                cov.add("j_frame0")
            if pnf % CHAIN_SUB and j // CHAIN_SUB == (pnf - 1) // CHAIN_SUB:
                cov.add("j_partial_sub")
            cov.add("no_rendezvous" if j == pnf - 1 else "rendezvous")
            cov.add("c0=0" if r["c0"] == 0 else "c0>0")
            if i > 0:
                k = prediction_kind(r["pred_j"], r["row_v"])
                if k:
                    cov.add(k)
            kinds = {lt for _, lt in r["light"]}
            if kinds == {True, False}:
                cov.add("mixed_light_general")
        if d["pf0"] + pnf == n_run and d["rounds"] and d["decision"][pnf - 1] != 0:
            cov.add("tail_redo_last_frame_on")
    return cov


# ---------------------------------------------------------------- the scripted clips of the tests
# Refractory period 0.8 ms at 300 frames/s: the rule is on from M >= 5.  A patch's step from grey level 40 to 200 (or back)
# fires 8-15 events per pixel on that frame and is a rule-on CASCADE of two or three frames (the rule holds events back, the
# next frames fire them); a step 40 -> 90 is a single rule-on frame.  Patch events are (run frame, level): the level holds
# from that run frame on (run frame r = the clip's frame r + 1).
KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=200.0, leak_rate_hz=0.1, shot_noise_rate_hz=1.0,
          refractory_period_s=0.0008)
SEED = 5


def _p(y0, x0, h, w, events):
    return (y0, x0, h, w, tuple(events))


SCENARIOS = {
    # 8 frames per launch, 61 run frames (the last launch has 5: a partial sub-pass)
    "k8": dict(H=48, W=80, K=8, F=62, fps=300.0, patches=[
        _p(4, 8, 10, 30, [(8, 200), (20, 40), (23, 200), (34, 40), (44, 120), (45, 40), (58, 200)]),
        _p(20, 8, 10, 30, [(4, 90), (5, 40), (55, 90)]),
    ]),
    # 11 frames per launch: sub-passes of 8 and 3 frames; a rule-on cascade from offset 7 of the first
    "k11": dict(H=48, W=80, K=11, F=51, fps=300.0, patches=[
        _p(4, 8, 10, 30, [(18, 200), (47, 40)]),
        _p(20, 8, 10, 30, [(3, 90), (4, 40), (32, 90), (49, 200)]),
        _p(34, 44, 10, 30, [(22, 200)]),
    ]),
    # 32 frames per launch, 75 run frames (the last launch has 11)
    "k32": dict(H=48, W=80, K=32, F=76, fps=300.0, patches=[
        _p(4, 8, 10, 30, [(3, 200), (15, 40), (40, 200), (73, 40)]),
        _p(20, 8, 10, 30, [(50, 90), (51, 40), (63, 90)]),
    ]),
    # npx = 3500: the last wave of the last workgroup is partial; a patch there and one in a later workgroup
    "ragged": dict(H=50, W=70, K=8, F=34, fps=300.0, patches=[
        _p(49, 26, 1, 44, [(5, 200), (17, 40), (32, 200)]),
        _p(20, 40, 10, 21, [(10, 200), (23, 90)]),
    ]),
    # the benchmark's sensor size: 352 workgroups at every rendezvous
    "hd": dict(H=260, W=346, K=32, F=41, fps=300.0, patches=[
        _p(200, 290, 30, 50, [(7, 200), (38, 40)]),
        _p(5, 5, 20, 40, [(20, 200), (26, 90)]),
    ]),
}


def scenario_clip(sc):
    F = sc["F"]
    patches = [(y0, x0, h, w, schedule(F, [(r + 1, lv) for r, lv in ev])) for (y0, x0, h, w, ev) in sc["patches"]]
    frames = scripted_clip(sc["H"], sc["W"], F, patches, seed=1)
    times = [i / sc["fps"] for i in range(F)]
    return frames, times


def model_coverage(model):
    """The redo cases the CPU model alone shows a clip reaches (first two decisions of every launch, rule-on cascades)."""
    cov = set()
    n_run = len(model["true"])
    for d, (f0, nf, pf0, pnf) in zip(model_decisions(model), [p for p in model["plan"] if p[3] > 0]):
        for key in ("j1", "j2"):
            j = d[key]
            if j is None:
                continue
            if j % CHAIN_SUB == 0:
                cov.add(key + "_offset0")
            if j % CHAIN_SUB == CHAIN_SUB - 1 and j // CHAIN_SUB < (pnf - 1) // CHAIN_SUB:
                cov.add(key + "_offset7_rule_on" if key == "j1" or d["v2"] else key + "_offset7")
            if j == 0:
                cov.add(key + "_frame0")
            if pnf % CHAIN_SUB and j // CHAIN_SUB == (pnf - 1) // CHAIN_SUB:
                cov.add(key + "_partial_sub")
            cov.add(key + ("_last" if j == pnf - 1 else "_before_last"))
        if d["j2"] is not None:
            cov.add(prediction_kind(d["pred2"], d["v2"]))
        if pf0 + pnf == n_run and model["true"][n_run - 1] != 0 and d["j1"] is not None:
            cov.add("tail_redo_last_frame_on")
    on = np.concatenate([[0], (model["true"] != 0).astype(np.int64), [0]])
    edges = np.nonzero(np.diff(on))[0]
    runs = edges[1::2] - edges[0::2]
    if runs.size and runs.max() >= 3:
        cov.add("cascade>=3")
    return cov


# what the CPU model shows each scripted clip reaches (tests/test_chain_redo_model.py keeps the clips honest)
MODEL_CASES = {
    "k8": {"j1_offset0", "j1_frame0", "j1_last", "j1_before_last", "j1_partial_sub", "false_negative", "false_positive",
           "wrong_value", "cascade>=3", "tail_redo_last_frame_on"},
    "k11": {"j1_offset7_rule_on", "j2_partial_sub", "j2_offset0", "false_positive", "false_negative", "tail_redo_last_frame_on"},
    "k32": {"j1_offset0", "j2_last", "j2_partial_sub", "cascade>=3", "tail_redo_last_frame_on"},
    "ragged": {"j1_frame0", "j1_partial_sub", "tail_redo_last_frame_on"},
    "hd": {"j1_offset7_rule_on", "j2_offset0", "cascade>=3"},
}
