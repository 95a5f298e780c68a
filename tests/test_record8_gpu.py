"""GPU parity of the chain that reads k_ahead's 8-byte records (V2E_AMD_CHAIN_FUSED=0: the pixel byte, the leak step and the
shot decisions; the chain rebuilds lin-log and eps from the byte and the frame's dt_over_tau as it stages them) against the
CPU oracle and against the chain that builds its records itself (=1), bit for bit.

The frame intervals are NOT uniform, so that every frame has its own dt_over_tau: a record decoded with another frame's
scalar (the wrong lane, or in a redo pass the current launch's frames instead of the previous launch's) changes eps and
shows.  The frames hold the pixel values 0 and 255 on whole columns."""
import numpy as np
import pytest
import torch

from fixtures import sha
from v2e_amd._capi import RUN_GRAPH, RUN_REQUIRE_CHAIN

pytestmark = pytest.mark.gpu

H, W = 97, 131  # a small grid: the chain reads k_ahead's records by default


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
        f[:, 2] = 255 if i % 2 else 0  # 0 <-> 255 every frame
        frames.append(f)
    dts = rng.uniform(0.0004, 0.006, size=n)  # non-uniform frame intervals: a dt_over_tau per frame
    times = list(np.cumsum(dts) + 0.001)
    return np.stack(frames), times


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


def _check(kw, frames, times, oracle_lib, monkeypatch, seed=7):
    ora = oracle_lib.OracleEmulator(seed=seed, rng_mode="philox", **kw)
    oev = [ora.generate_events(f, t) for f, t in zip(frames, times)]
    ocounts = [0 if e is None else len(e) for e in oev]
    assert sum(ocounts) > 0
    oplanes = [ora.base_log_frame, ora.lp_log_frame]
    if kw.get("refractory_period_s", 0) > 0:
        oplanes.append(ora.timestamp_mem)
    ref = np.concatenate([e for e in oev if e is not None])
    runs = {fused: _hip(kw, frames, times, fused, monkeypatch, seed) for fused in (False, True)}
    for fused, (ev, counts, planes) in runs.items():
        tag = "fused" if fused else "k_ahead records"
        assert counts == ocounts, tag
        assert np.array_equal(ev, ref), tag
        for a, b in zip(planes, oplanes):
            assert np.array_equal(a, b), tag
    assert np.array_equal(runs[False][0], runs[True][0])


ALL_ON = dict(pos_thres=.2, neg_thres=.15, sigma_thres=.03, cutoff_hz=300, leak_rate_hz=.3, shot_noise_rate_hz=3.0,
              leak_jitter_fraction=0.1, refractory_period_s=0.0005)


@pytest.mark.parametrize("case", [
    "all_on",
    "refractory_heavy",   # the rule on in most frames: redo passes re-stage the previous launch's frames
    "eps_clamped",        # eps = min(lut_I * dt_over_tau, 1) at 1 on some frames and pixels, below it on others
    "log_input",
    "no_cutoff",
    "no_leak",
    "no_jitter",
    "no_shot",
])
def test_ahead_records_match_oracle_and_fused_chain(case, oracle_lib, monkeypatch):
    kw = dict(ALL_ON)
    if case == "refractory_heavy":
        kw["refractory_period_s"] = 0.004
    elif case == "eps_clamped":
        kw["cutoff_hz"] = 1000
    elif case == "log_input":  # L = the pixel value itself: thresholds in grey levels (a 0 -> 255 step stays below 1024 events)
        kw.update(hdr=True, pos_thres=2.0, neg_thres=1.5)
    elif case == "no_cutoff":
        kw["cutoff_hz"] = 0
    elif case == "no_leak":
        kw["leak_rate_hz"] = 0
    elif case == "no_jitter":
        kw["leak_jitter_fraction"] = 0
    elif case == "no_shot":
        kw["shot_noise_rate_hz"] = 0
    frames, times = _clip(75, seed=11)  # two full 32-frame launches and a partial one
    _check(kw, frames, times, oracle_lib, monkeypatch)


def test_ahead_records_run_longer_than_the_ring(oracle_lib, monkeypatch):
    """400 frames in one run: the ring of frame slots (three emission batches of 64) wraps twice."""
    frames, times = _clip(400, seed=12)
    _check(dict(ALL_ON, refractory_period_s=0.002), frames, times, oracle_lib, monkeypatch)


class _DigestSink:
    def __init__(self):
        self.steps = []

    def submit(self, ev, n, ready_event=None, run_bound=None):
        self.steps.append((int(n), sha(ev[:n].cpu().numpy())))

    def wait(self):
        pass


def test_bench_step_loop_ahead_records_equal_fused_chain(monkeypatch):
    """benchutil.run_steps as bench.py runs it (pipelined 300-frame runs of the benchmark clip): every step's event stream and
    the final planes, k_ahead's records against the chain's own."""
    import bench as B
    from v2e_amd import EventEmulator
    from v2e_amd.benchutil import run_steps
    dev = torch.device("cuda")
    F, steps, warm = B.FRAMES_PER_STEP, 3, 1
    frames_all = B.gen_frames_device(2 * F + 1, 1, dev)
    out = {}
    for fused in (False, True):
        monkeypatch.setenv("V2E_AMD_CHAIN_FUSED", "1" if fused else "0")
        emu = EventEmulator(device=dev, seed=1, rng_mode="philox", **B.DEFAULT_KW)
        emu.generate_events(frames_all[0], 0.0)
        sink = _DigestSink()
        run_steps(emu, frames_all, F, B.DT, steps, warm, sink, None, dev)
        assert emu._engine.last_pipeline()[0] == ("k_chain(fused records)" if fused else "k_chain")
        out[fused] = (sink.steps, emu.base_log_frame.cpu().numpy(), emu.lp_log_frame.cpu().numpy(), emu.timestamp_mem.cpu().numpy())
        del emu
    a, b = out[False], out[True]
    assert len(a[0]) == steps + warm and a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
