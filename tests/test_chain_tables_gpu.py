"""k_chain's per-launch decode tables (v2e_amd/csrc/emu_chain.h, CHAIN_TAB_MAX) and its coarse speculation test, on the grid
where the chain reads k_ahead's records by default: events, per-frame counts and the base / lp / timestamp planes of the
default run equal the CPU oracle, the fused chain (V2E_AMD_CHAIN_FUSED=1) and the same run decoding record by record
(V2E_AMD_CHAIN_TABLES=0), bit for bit.

A launch takes the table path when the dt_over_tau values of its own frames and of its predecessor's (which it may have to
redo) have at most four distinct bit patterns; otherwise the whole launch decodes record by record.  Which of the two a
timing pattern reaches is asserted here on the CPU: dt / tau recomputed as make_ctl does (emu_shared.h), distinct bit
patterns counted over every 32-frame window at every alignment -- so the intended path holds whatever the launch partition
is -- and, for the run's actual partition, by the kernel's own rule (`_launch_paths`).

What the windows of `t = i / 300` really hold: 7 distinct values in the first window (the differences of small i / 300
vary in their last bits), 4 or fewer from frame 5 on, 2-3 from frame 18 on.  The first two launches of that pattern
therefore decode record by record and the later ones through tables, which is asserted as such.

The coarse test is not observable by itself (a wave that passes it runs the exact per-frame code, which decides what is
published).  Its case asserts what can be seen: on the CPU that exactly one pixel -- so exactly one wave -- of the quiet
clip ever has a signal event, and on the device that the rule-on rows equal the oracle model's and that the run redoes.
"""
import functools
import math

import numpy as np
import pytest

import chain_redo as cr
from test_record8_gpu import ALL_ON, H, W, _clip
from v2e_amd._capi import RUN_GRAPH, RUN_REQUIRE_CHAIN

pytestmark = pytest.mark.gpu

N_FRAMES = 141   # the first frame initialises the state: 140 run frames, four full 32-frame launches and a partial one
K_REFR = 32      # frames per launch of a small grid with a refractory period (64 without one)
TAB_MAX = 4      # CHAIN_TAB_MAX
STEP = 2.0 ** -12


@functools.lru_cache(maxsize=None)
def _frames():
    return _clip(N_FRAMES, seed=21)[0]  # (shared by every case; nothing writes to it)


def _dtaus(times, cutoff_hz):
    """dt_over_tau of every run frame as make_ctl computes it (the first frame leaves t_previous at 0)."""
    tau = 1.0 / (math.pi * 2 * cutoff_hz)
    out, tp = [], 0.0
    for t in times[1:]:
        out.append((float(t) - tp) / tau)
        tp = float(t)
    return np.array(out, dtype=np.float64)


def _distinct(d):
    return len(set(np.ascontiguousarray(d).view(np.uint64).tolist()))


def _windows(d, w=K_REFR, first=0):
    """distinct bit patterns of every w-frame window starting at frame >= first"""
    return [_distinct(d[i:i + w]) for i in range(first, len(d) - w + 1)]


def _launch_paths(d, K, has_refr):
    """The kernel's rule on the run's launch partition: per launch (tail launch included) True = tables.  A launch counts
    its own frames and, with a refractory period, its predecessor's."""
    n = len(d)
    nB = (n + K - 1) // K
    out = []
    for L in range(nB + (1 if has_refr else 0)):
        lo = (L - 1) * K if (has_refr and L > 0) else L * K
        out.append(_distinct(d[max(lo, 0):min((L + 1) * K, n)]) <= TAB_MAX if lo < n else True)
    return out


def _cum(intervals):
    return [0.0] + list(np.cumsum(np.asarray(intervals, dtype=np.float64)))


def _times(pattern):
    n = N_FRAMES - 1
    if pattern == "fps300":
        return [i / 300 for i in range(N_FRAMES)]
    if pattern == "one_value":
        return [i * 2.0 ** -8 for i in range(N_FRAMES)]
    vals = [m * STEP for m in (13, 17, 21, 25, 19, 27)]  # multiples of 2**-12 between 0.003 and 0.007 s: sums of them are exact
    assert all(0.003 < v < 0.007 for v in vals)
    if pattern == "four_values":
        return _cum([vals[i % 4] for i in range(n)])
    if pattern == "six_in_the_middle":  # 6 values on run frames 40-100, 2 elsewhere
        return _cum([vals[i % 6] if 40 <= i <= 100 else vals[i % 2] for i in range(n)])
    if pattern == "disjoint_pairs":  # launches alternate between two value pairs: own and predecessor frames share none
        return _cum([vals[2 * ((i // K_REFR) % 2) + i % 2] for i in range(n)])
    raise KeyError(pattern)


def _assert_structure(pattern, d, K, has_refr):
    paths = _launch_paths(d, K, has_refr)
    w32 = _windows(d)
    if pattern == "fps300":
        assert w32[0] == 7 and max(w32[5:]) <= TAB_MAX and set(w32[18:]) == {2, 3}
        assert not paths[0] and all(paths[2:])
    elif pattern == "one_value":
        assert set(w32) == {1} and _distinct(d) == 1 and all(paths)
    elif pattern == "four_values":
        assert set(w32) == {4} and _distinct(d) == 4 and all(paths)  # the cap itself
    elif pattern == "six_in_the_middle":
        assert set(_windows(d[40:101])) == {6} and set(_windows(d[:40])) | set(_windows(d[101:])) == {2}
        assert paths[0] and not paths[1] and not paths[2] and paths[-1]
        # a record-by-record launch validates a table launch (launch 1 redoes launch 0) and a table launch a record-by-record one
        assert any(a and not b for a, b in zip(paths, paths[1:])) and any(b and not a for a, b in zip(paths, paths[1:]))
    elif pattern == "disjoint_pairs":
        assert max(w32) <= TAB_MAX and all(paths)
        for L in range(1, len(d) // K_REFR):
            own, prev = d[L * K_REFR:(L + 1) * K_REFR], d[(L - 1) * K_REFR:L * K_REFR]
            assert _distinct(own) == 2 and _distinct(prev) == 2 and _distinct(np.concatenate([own, prev])) == 4


def _hip(kw, frames, times, monkeypatch, fused, tables, seed=7, want_rows=False):
    from v2e_amd import EventEmulator
    monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "1" if fused else "0")
    monkeypatch.setenv("V2E_AMD_CHAIN_TABLES", "1" if tables else "0")
    emu = EventEmulator(device="cuda", seed=seed, rng_mode="philox", max_iters=1024, **kw)
    ev, counts = emu.generate_events_batch(frames, times, use_graph=RUN_REQUIRE_CHAIN | RUN_GRAPH)
    kind, fpl, _ = emu._engine.last_pipeline()
    assert kind == ("k_chain(fused records)" if fused else "k_chain")
    planes = [emu.base_log_frame.cpu().numpy(), emu.lp_log_frame.cpu().numpy()]
    if emu.timestamp_mem is not None:
        planes.append(emu.timestamp_mem.cpu().numpy())
    rows = emu._engine.debug_chain_rows() if want_rows else None
    return ev, list(counts), planes, fpl, rows


def _check(kw, frames, times, pattern, oracle_lib, monkeypatch, seed=7):
    has_refr = kw.get("refractory_period_s", 0) > 0
    ora = oracle_lib.OracleEmulator(seed=seed, rng_mode="philox", **kw)
    oev = [ora.generate_events(f, t) for f, t in zip(frames, times)]
    ocounts = [0 if e is None else len(e) for e in oev]
    assert sum(ocounts) > 0
    oplanes = [ora.base_log_frame, ora.lp_log_frame] + ([ora.timestamp_mem] if has_refr else [])
    ref = np.concatenate([e for e in oev if e is not None])
    runs = {"tables": _hip(kw, frames, times, monkeypatch, False, True, seed),
            "record by record": _hip(kw, frames, times, monkeypatch, False, False, seed),
            "fused": _hip(kw, frames, times, monkeypatch, True, True, seed)}
    K = runs["tables"][3]
    assert K == (K_REFR if has_refr else 64)
    if pattern is not None:
        cut = kw.get("cutoff_hz", 0)
        _assert_structure(pattern, _dtaus(times, cut), K, has_refr)
    for tag, (ev, counts, planes, _, _) in runs.items():
        assert counts == ocounts, tag
        assert np.array_equal(ev, ref), tag
        assert len(planes) == len(oplanes)
        for a, b in zip(planes, oplanes):
            assert np.array_equal(a, b), tag


PATTERNS = ["fps300", "one_value", "four_values", "six_in_the_middle", "disjoint_pairs"]


@pytest.mark.parametrize("refr", [0.0005, 0.004], ids=["all_on", "refractory_heavy"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_table_decode_matches_oracle_fused_and_record_decode(pattern, refr, oracle_lib, monkeypatch):
    kw = dict(ALL_ON, refractory_period_s=refr)
    _check(kw, _frames(), _times(pattern), pattern, oracle_lib, monkeypatch)


@pytest.mark.parametrize("case", ["eps_clamped", "log_input", "no_refractory"])
def test_table_decode_switch_combinations(case, oracle_lib, monkeypatch):
    kw = dict(ALL_ON)
    if case == "eps_clamped":
        # eps = min(lut_I * dt_over_tau, 1).  At 1000 Hz and 1 / 300 s EVERY table entry is clamped (om = 0, el = L exactly); the
        # tables that hold clamped and unclamped entries side by side are those of the 300 Hz cases above
        kw["cutoff_hz"] = 1000
        eps = {hz: np.array([(v + 20.0) / 275.0 for v in (0, 255)]) * ((1 / 300) * (math.pi * 2 * hz)) for hz in (300, 1000)}
        assert eps[1000].min() > 1.0 and eps[300][0] < 1.0 < eps[300][1]
    elif case == "log_input":  # the table's L is the pixel byte itself
        kw.update(hdr=True, pos_thres=2.0, neg_thres=1.5)
    elif case == "no_refractory":  # never a predecessor set; 64 frames per launch
        kw["refractory_period_s"] = 0
    times = _times("fps300")
    # (the last bits of dt / tau depend on tau: the launches that take the table path, by the kernel's rule, for this cutoff)
    has_refr = kw["refractory_period_s"] > 0
    paths = _launch_paths(_dtaus(times, kw["cutoff_hz"]), K_REFR if has_refr else 64, has_refr)
    assert not paths[0] and all(paths[2:]) and len(paths) == (6 if has_refr else 3)
    _check(kw, _frames(), times, None, oracle_lib, monkeypatch)


def test_coarse_speculation_test_passes_one_wave(oracle_lib, monkeypatch):
    """A flat, noise-free scene in which one pixel jumps 0 -> 255 on one frame, refractory period 4 ms at 300 frames/s (the rule
    is on from one event): only that pixel's wave ever reaches the smallest rule threshold of a pass."""
    kw = dict(ALL_ON, refractory_period_s=0.004)
    jy, jx, jf = 50, 70, 45  # run frame 44: the second launch, not on a sub-pass boundary
    frames = np.full((N_FRAMES, H, W), 100, np.uint8)
    frames[:jf, jy, jx] = 0
    frames[jf:, jy, jx] = 255
    times = _times("fps300")
    # on the CPU: without shot noise (whose events are not counts) every event of the clip is that pixel's
    quiet = oracle_lib.OracleEmulator(seed=7, rng_mode="philox", **dict(kw, shot_noise_rate_hz=0))
    qev = [quiet.generate_events(f, t) for f, t in zip(frames, times)]
    assert all(e is None or len(e) == 0 for e in qev[:jf])
    qall = np.concatenate([e for e in qev if e is not None and len(e)])
    assert len(qall) > 0 and set(zip(qall[:, 1].astype(int), qall[:, 2].astype(int))) == {(jx, jy)}
    _check(kw, frames, times, "fps300", oracle_lib, monkeypatch)
    # on the device: the rule-on rows are the model's, and the run redoes
    model = cr.oracle_model(oracle_lib, frames, times, kw, K_REFR, seed=7)
    assert model["true"].any()
    for tables in (True, False):
        rows = _hip(kw, frames, times, monkeypatch, False, tables, want_rows=True)[4]
        assert rows is not None and rows.shape[2] == 1
        rows = rows[:, :, 0, :].astype(np.int64)
        assert np.array_equal(rows[:, 0], model["row0"]) and rows[:, 0].any()
        rep = cr.replay(rows, model["plan"], K_REFR)
        assert any(d["rounds"] for d in rep), "no launch was redone"
        for d in rep:
            assert np.array_equal(d["decision"], model["true"][d["pf0"]:d["pf0"] + d["pnf"]])
