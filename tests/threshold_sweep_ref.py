"""Inputs and the CPU reference of the ThresholdSweep tests (tests/test_threshold_sweep.py, tests/test_threshold_sweep_gpu.py).

The reference is the sweep's contract taken literally: one fresh `oracle.OracleEmulator(rng_mode="philox", ...)` per column, the
clip's frames given to it one by one, its rows counted inside the inclusive ROI.  Each configuration is computed once per process
and shared (`reference`); the arrays it returns are read-only.
"""
import functools

import numpy as np

SEED = 7
ROI = ((3, 28), (5, 30))  # ((x0, x1), (y0, y1)), inclusive
THRESHOLDS = (0.13, 0.15, 0.17, 0.2, 0.25, 0.31, 0.38, 0.45, 0.6, 0.8, 1.0)
NEG_THRESHOLDS = tuple(reversed(THRESHOLDS))  # the "neg_thresholds different from thresholds" case
REFRACTORY_S = 4e-4  # with 1 ms frames the rule (emulator.py:830) is on when a frame's largest per-pixel count M >= 3

# name -> (model parameters, neg_thresholds or None)
CONFIGS = {
    "defaults": ({}, None),
    "scalar_f32": (dict(sigma_thres=0.0, leak_rate_hz=0.0), None),
    "cutoff_f64": (dict(cutoff_hz=100.0), None),
    "no_jitter": (dict(leak_jitter_fraction=0.0), None),
    "neg_differs": ({}, NEG_THRESHOLDS),
    "refractory": (dict(refractory_period_s=REFRACTORY_S), None),
    "refractory_scalar": (dict(refractory_period_s=REFRACTORY_S, sigma_thres=0.0, leak_rate_hz=0.0), None),
}


def make_clip(height=37, width=33, n_frames=40, rng_seed=3):
    """frame[k] = clip(120 + 70 sin(2 pi (x + 0.5 k) / 17) cos(2 pi (y - 0.3 k) / 23) + rng.integers(-2, 3), 0, 255) as uint8,
    t[k] = k * 1e-3.  Returns (frames [F,H,W] uint8, times [F] float64)."""
    rng = np.random.default_rng(rng_seed)
    y, x = np.mgrid[0:height, 0:width]
    frames = np.empty((n_frames, height, width), np.uint8)
    for k in range(n_frames):
        v = 120 + 70 * np.sin(2 * np.pi * (x + 0.5 * k) / 17) * np.cos(2 * np.pi * (y - 0.3 * k) / 23)
        frames[k] = np.clip(v + rng.integers(-2, 3, size=(height, width)), 0, 255).astype(np.uint8)
    return frames, np.arange(n_frames, dtype=np.float64) * 1e-3


def count_in_roi(ev, roi):
    """(ON, OFF) of host rows [N,4] = (t, x, y, p) inside the inclusive ROI; ev may be None (no events)."""
    if ev is None or len(ev) == 0:
        return 0, 0
    (x0, x1), (y0, y1) = roi
    inside = (ev[:, 1] >= x0) & (ev[:, 1] <= x1) & (ev[:, 2] >= y0) & (ev[:, 2] <= y1)
    return int(np.count_nonzero(inside & (ev[:, 3] > 0))), int(np.count_nonzero(inside & (ev[:, 3] < 0)))


def oracle_sweep(frames, times, pos, neg, roi, seed=SEED, **model):
    """One oracle run per column.  Returns dict(on, off: int64 [T]; rule_on: bool [T], the refractory rule was on in some frame;
    max_m: int64 [T], the largest per-pixel count of any frame)."""
    from oracle import oracle as orc
    T = len(pos)
    on, off = np.zeros(T, np.int64), np.zeros(T, np.int64)
    rule_on, max_m = np.zeros(T, bool), np.zeros(T, np.int64)
    refr = float(model.get("refractory_period_s", 0.0))
    for j in range(T):
        emu = orc.OracleEmulator(pos_thres=float(pos[j]), neg_thres=float(neg[j]), rng_mode="philox", seed=seed,
                                 shot_noise_rate_hz=0.0, **model)
        t_prev = 0.0
        for k, (f, t) in enumerate(zip(frames, times)):
            ev = emu.generate_events(f, float(t))
            if k == 0:
                assert ev is None  # the first frame initialises the emulator (and leaves t_previous where it was)
                continue
            a, b = count_in_roi(ev, roi)
            on[j] += a
            off[j] += b
            max_m[j] = max(max_m[j], emu.last_M)
            if refr > (float(t) - t_prev) / max(1, emu.last_M):  # emulator.py:830
                rule_on[j] = True
            t_prev = float(t)
    return dict(on=on, off=off, rule_on=rule_on, max_m=max_m)


@functools.lru_cache(maxsize=None)
def clip():
    frames, times = make_clip()
    frames.setflags(write=False)
    times.setflags(write=False)
    return frames, times


@functools.lru_cache(maxsize=None)
def reference(name, roi=ROI):
    """The oracle's sweep of the test clip under CONFIGS[name] (computed once, read-only)."""
    model, neg = CONFIGS[name]
    frames, times = clip()
    ref = oracle_sweep(frames, times, THRESHOLDS, THRESHOLDS if neg is None else neg, roi, **model)
    for v in ref.values():
        v.setflags(write=False)
    return ref
