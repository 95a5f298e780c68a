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
    max_m: int64 [T], the largest per-pixel count of any frame; max_m_roi: the same among the pixels inside the ROI)."""
    from oracle import oracle as orc
    T = len(pos)
    on, off = np.zeros(T, np.int64), np.zeros(T, np.int64)
    rule_on, max_m, max_m_roi = np.zeros(T, bool), np.zeros(T, np.int64), np.zeros(T, np.int64)
    (x0, x1), (y0, y1) = roi
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
            max_m_roi[j] = max(max_m_roi[j], max(emu.last[c][y0:y1 + 1, x0:x1 + 1].max() for c in ("pos_cnt", "neg_cnt")))
            if refr > (float(t) - t_prev) / max(1, emu.last_M):  # emulator.py:830
                rule_on[j] = True
            t_prev = float(t)
    return dict(on=on, off=off, rule_on=rule_on, max_m=max_m, max_m_roi=max_m_roi)


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


# ---------------------------------------------------------------------------------------------------------------------
# Inputs aimed at the arms of k_sweep (v2e_amd/csrc/sweep.hip) that make_clip never reaches.  The predicates are those of
# tests/chain_dtypes.py; tests/test_threshold_sweep.py keeps every builder honest with the oracle alone.
import chain_dtypes as cd  # noqa: E402

WHOLE = ((0, 32), (0, 36))  # the whole 33 x 37 sensor as an ROI
AIM_SIGMA = 1e-12  # per-pixel thresholds (sigma_thres > 0 selects the kernel) that all round to the nominal one
AIM_DT = 0.05      # with cutoff_hz = 100 every grey level's eps = inten01 * dt / tau >= 2.28 clamps to 1: lp == L exactly
AIM_FRAMES = 8
# float32 thresholds in float64 state: without a leak no estimate is ever too large (test_threshold_sweep.py says why).  A leak of
# about one unit in the last place of the base (0.05 s * 1e-14 Hz * theta) puts an OFF quotient that far below an exact multiple.
AIM_LEAK = dict(leak_rate_hz=1e-14, leak_jitter_fraction=0.0, noise_rate_cov_decades=0.0)  # every pixel's rate is leak_rate_hz
AIM_N = (1, 2, 4, 8, 16, 3)  # theta = |L[b] - L[a]| / n
# the four instantiations k_sweep<R, *, SCALAR>: the state type follows cutoff_hz > 0, SCALAR follows sigma_thres == 0
INSTANTIATIONS = {
    "f32_scalar": dict(state=np.float32, scalar=True, model=dict(sigma_thres=0.0, cutoff_hz=0.0, leak_rate_hz=0.0)),
    "f32_pixel": dict(state=np.float32, scalar=False, model=dict(sigma_thres=AIM_SIGMA, cutoff_hz=0.0, leak_rate_hz=0.0)),
    "f64_scalar": dict(state=np.float64, scalar=True, model=dict(sigma_thres=0.0, cutoff_hz=100.0, leak_rate_hz=0.0)),
    "f64_pixel": dict(state=np.float64, scalar=False, model=dict(sigma_thres=AIM_SIGMA, cutoff_hz=100.0, **AIM_LEAK)),
}
# what a pixel-frame-column is to the floor division: the estimate one too large (`mag -= r0 < 0`), one too small (`mag += r0 >=
# bt`), one too small on an exact multiple (r0 == bt, the equality of that arm)
LARGE, SMALL, SMALL_EXACT = 1, 2, 3


@functools.lru_cache(maxsize=None)
def levels_lin_log():
    """The oracle's lin-log (float32 [256]) of the 256 grey levels."""
    from oracle import oracle as orc
    L = np.array(cd._oracle_lin_log(orc, np.arange(256, dtype=np.float32)))
    L.setflags(write=False)
    return L


def _kinds(am, theta, R):
    """LARGE / SMALL / SMALL_EXACT / 0 of quotients am / theta held in type R (0 too where no event fires)."""
    fires = am >= theta
    amf = np.where(fires, am, theta)
    off = cd.estimate_off_by_one(amf, theta, R)
    zero = cd.remainder_zero(amf, theta, R)
    return np.where(fires & (off == 1), LARGE, np.where(fires & (off == -1), np.where(zero, SMALL_EXACT, SMALL), 0))


def aimed_leak(model, times, k, theta):
    """Frame k's leak step ((float)dt * rate) * theta in float32, as k_sweep and the emulator round it, for a model without jitter
    and with noise_rate_cov_decades = 0 (rate = leak_rate_hz on every pixel); frame 1's interval runs from time 0."""
    theta = np.asarray(theta, np.float32)
    if not model["leak_rate_hz"] > 0:
        return np.zeros(theta.shape, np.float32)
    assert model["leak_jitter_fraction"] == 0 and model["noise_rate_cov_decades"] == 0
    dt = np.float32(times[k] - (times[k - 1] if k > 1 else 0.0))
    return ((dt * np.float32(model["leak_rate_hz"])) * theta).astype(np.float32)


def _leaky_large_columns(model):
    """(a, b, n, theta), theta = fl32((L[b] - L[a]) / n), for float64 state under AIM_LEAK: frame 1 goes a -> b (n ON events, the
    base lands on L[b] less the leak's rounding), frame 2 comes back and its OFF quotient lies just below n: estimate too large."""
    R = np.float64
    L = levels_lin_log().astype(R)
    a, b = np.triu_indices(256, 1)
    times = AIM_DT * np.arange(1, 4)
    out = []
    for n in range(1, 17):
        th = ((L[b] - L[a]) / n).astype(np.float32)
        ok = (th >= 0.05) & (th <= 1.0)
        th = np.where(ok, th, np.float32(1))
        bc = L[a] - aimed_leak(model, times, 1, th).astype(R)
        q, _ = cd._exact_floor_and_rem(np.where(ok, L[b] - bc, 1.0), th.astype(R), R)
        base = bc + (q.astype(np.float32) * th).astype(np.float32).astype(R)
        am = (base - aimed_leak(model, times, 2, th).astype(R)) - L[a]
        fires = ok & (am >= th)
        kind = np.where(fires, _kinds(np.where(fires, am, 1.0), th.astype(R), R), 0)
        out += [(int(a[i]), int(b[i]), n, float(th[i])) for i in np.nonzero(kind == LARGE)[0]]
    return out


@functools.lru_cache(maxsize=None)
def aimed_columns(instantiation):
    """12 columns (a, b, n, theta) with theta = |L[b] - L[a]| / n in [0.05, 1], held as the instantiation holds it (scalar thresholds
    in float64 state: the double; otherwise a float32 value), whose own transition a -> b the reciprocal estimate gets wrong: 5 with
    the estimate too small on the exact multiple and n a power of two, 3 the same with n = 3, and 4 too large (n = 3).  Float32
    thresholds in float64 state have no transition of the last kind; theirs come from _leaky_large_columns."""
    inst = INSTANTIATIONS[instantiation]
    R = inst["state"]
    L = levels_lin_log()
    a, b = np.triu_indices(256, 1)
    d = (L[b].astype(R) - L[a].astype(R)).astype(R)
    found = {"pow2": [], "small3": [], "large3": []}
    for n in AIM_N:
        theta = d.astype(np.float64) / n
        if not (inst["scalar"] and R == np.float64):
            theta = theta.astype(np.float32).astype(np.float64)
        ok = (theta >= 0.05) & (theta <= 1.0)
        kind = np.where(ok, _kinds(d, np.where(ok, theta, 1.0).astype(R), R), 0)
        for name, k in (("small3", SMALL_EXACT), ("large3", LARGE)) if n == 3 else (("pow2", SMALL_EXACT),):
            found[name] += [(int(a[i]), int(b[i]), n, float(theta[i])) for i in np.nonzero(kind == k)[0]]
    if inst["model"]["leak_rate_hz"] > 0:
        assert not found["large3"]
        found["large3"] = _leaky_large_columns(inst["model"])
    cols, seen = [], set()
    for name, want in (("pow2", 5), ("small3", 3), ("large3", 4)):
        c = sorted(found[name], key=lambda r: r[3])
        assert len(c) >= 2 * want, (instantiation, name, len(c))
        for i in np.linspace(0, len(c) - 1 - want, want).astype(int):  # spread over [0.05, 1]
            while c[i][3] in seen:
                i += 1
            seen.add(c[i][3])
            cols.append(c[i])
    return tuple(cols)


@functools.lru_cache(maxsize=None)
def aimed_clip(instantiation, height=37, width=33, n_frames=AIM_FRAMES, seed=11):
    """(frames uint8 [F][H][W], times [F], thresholds [T]) for one instantiation of k_sweep; the model parameters are
    INSTANTIATIONS[instantiation]["model"], refractory_period_s = 0, neg_thresholds = thresholds.

    Frame 0 gives pixel p the level a (or b, every other time) of column p % T, so that frame 1 can make that column's own
    transition and frame 2 the way back.  Every frame from 1 on is searched: one oracle per column holds the state, and per pixel
    the grey levels (float32 state: all 256; float64 state, where a hit comes from the columns' own lattice and never by chance:
    the levels a and b of the columns) are tried against every column's base less the frame's leak step.  The first level is kept
    at which some column's quotient is of the kind the pixel asks for this frame (a third each: LARGE, SMALL, SMALL_EXACT), else
    any hit, else a random level.  In float64 state the frame interval clamps eps to 1 (AIM_DT), so lp is the level's lin-log
    exactly and the search can aim as in float32."""
    from oracle import oracle as orc
    inst = INSTANTIATIONS[instantiation]
    R = inst["state"]
    cols = aimed_columns(instantiation)
    T, npx = len(cols), height * width
    thetas = np.array([c[3] for c in cols])
    rng = np.random.Generator(np.random.PCG64(seed))
    times = AIM_DT * np.arange(1, n_frames + 1)
    L = levels_lin_log().astype(R)
    ab = np.array([c[:2] for c in cols])
    cand = np.arange(256) if R == np.float32 else np.unique(ab)
    oras = [orc.OracleEmulator(pos_thres=float(t), neg_thres=float(t), rng_mode="philox", seed=SEED, shot_noise_rate_hz=0.0,
                               refractory_period_s=0.0, **inst["model"]) for t in thetas]
    p = np.arange(npx)
    frames = [ab[p % T, (p // T) % 2].astype(np.uint8).reshape(height, width)]
    for k in range(n_frames):
        if k > 0:
            base = np.stack([o.base_log_frame.reshape(npx) for o in oras])  # [T][npx]
            # the divisors as the instantiation holds them: the double that was passed in, or the float32 plane
            th = np.stack([np.full(npx, o._pos_scalar, R) if inst["scalar"] else o.pos_thres_arr.reshape(npx).astype(R) for o in oras])
            base = base - aimed_leak(inst["model"], times, k, th).astype(R)
            diff = (L[cand][None, None, :] - base[:, :, None]).astype(R)
            kind = _kinds(np.abs(diff), np.broadcast_to(th[:, :, None], diff.shape), R)  # [T][npx][len(cand)]
            pref = np.array([LARGE, SMALL, SMALL_EXACT])[(p + k) % 3]
            wanted = (kind == pref[None, :, None]).any(axis=0)  # [npx][len(cand)]
            anyhit = (kind != 0).any(axis=0)
            level = np.where(wanted.any(axis=1), cand[np.argmax(wanted, axis=1)],
                             np.where(anyhit.any(axis=1), cand[np.argmax(anyhit, axis=1)], rng.integers(0, 256, size=npx)))
            frames.append(level.astype(np.uint8).reshape(height, width))
        for o in oras:
            o.generate_events(frames[-1], float(times[k]))
            assert o.lp_log_frame.dtype == R and np.array_equal(o.lp_log_frame, L[frames[-1]])
            assert not inst["model"]["leak_rate_hz"] > 0 or np.all(o.noise_rate_array == 1)
    frames = np.stack(frames)
    frames.setflags(write=False)
    times.setflags(write=False)
    return frames, times, tuple(float(t) for t in thetas)


@functools.lru_cache(maxsize=None)
def aimed_reference(instantiation):
    """oracle_sweep of aimed_clip(instantiation) over the whole sensor (computed once, read-only)."""
    frames, times, thetas = aimed_clip(instantiation)
    ref = oracle_sweep(frames, times, thetas, thetas, WHOLE, refractory_period_s=0.0, **INSTANTIATIONS[instantiation]["model"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def column_model(frames, times, pos, neg, roi, R=np.float32):
    """(ON, OFF) of one column by plain numpy: scalar thresholds, no leak, refractory rule off, state of type R.  R = float32 is
    the model without a cutoff; R = float64 is the model with a cutoff whose eps clamps to 1 in every frame (lp == L, AIM_DT).
    It stands in for the oracle where a pixel fires millions of events per frame, which the oracle would emit row by row."""
    assert len(times) == len(frames)
    L = levels_lin_log().astype(R)
    (x0, x1), (y0, y1) = roi
    inside = np.zeros(frames.shape[1:], bool)
    inside[y0:y1 + 1, x0:x1 + 1] = True
    base, on, off = L[frames[0]], 0, 0
    for f in frames[1:]:
        diff = (L[f] - base).astype(R)
        is_pos = diff > 0
        q, _ = cd._exact_floor_and_rem(np.abs(diff), np.where(is_pos, R(pos), R(neg)), R)
        step = (q.astype(np.float32) * np.where(is_pos, np.float32(pos), np.float32(neg))).astype(np.float32)
        base = (base + np.where(is_pos, step, -step).astype(R)).astype(R)
        on += int(q[inside & is_pos].sum())
        off += int(q[inside & ~is_pos].sum())
    return on, off


def model_sweep(frames, times, pos, neg, roi, R=np.float32):
    """column_model per column, in oracle_sweep's layout."""
    c = np.array([column_model(frames, times, p, n, roi, R) for p, n in zip(pos, neg)], np.int64).reshape(-1, 2)
    return dict(on=c[:, 0].copy(), off=c[:, 1].copy())


def alternating_clip(height, width, n_frames, dt=AIM_DT):
    """Whole frames of 0 and 255 in turn (frame 0 is 0), t[k] = (k + 1) dt."""
    frames = np.zeros((n_frames, height, width), np.uint8)
    frames[1::2] = 255
    return frames, dt * np.arange(1, n_frames + 1)


GENERIC = {  # name -> (state, threshold, model): the per-frame quotient 5.54 / theta exceeds QMAX (1e6 float32, 1e9 float64 state)
    "f32": (np.float32, 2.0 ** -20, dict(sigma_thres=0.0, cutoff_hz=0.0, leak_rate_hz=0.0, refractory_period_s=0.0)),
    "f64": (np.float64, 2.0 ** -28, dict(sigma_thres=0.0, cutoff_hz=100.0, leak_rate_hz=0.0, refractory_period_s=0.0)),
}
WAVE_SUM_THETA = 2.0 ** -20


def wave_sum_frames():
    """The fewest alternating frames at which the 64 pixels of an 8 x 8 sensor together pass 2^32 events of one polarity at
    WAVE_SUM_THETA, from the model: (n_frames, (ON, OFF) of all 64 pixels, the largest total of one pixel and polarity)."""
    for n in range(3, 64):
        frames, times = alternating_clip(8, 8, n)
        on, off = column_model(frames, times, WAVE_SUM_THETA, WAVE_SUM_THETA, ((0, 7), (0, 7)))
        if max(on, off) > 2 ** 32:
            one = column_model(frames, times, WAVE_SUM_THETA, WAVE_SUM_THETA, ((0, 0), (0, 0)))
            return n, (on, off), max(one)
    raise AssertionError("no frame count found")


LEVELS_T0 = 0.004


@functools.lru_cache(maxsize=None)
def levels_clip(t0=LEVELS_T0, height=37, width=33, n_frames=10, seed=21):
    """(frames, times): every grey level 0..255 on some pixel of every frame (pixel p of frame k holds (37 p + 101 k) mod 256),
    the first 8 pixels step through 0, 20, 21 and 255 in both directions (the switch of lin-log and the ends of the scale), frame
    intervals drawn as chain_dtypes.clip draws them (uniform 0.4 - 6 ms).  t[0] = t0: with t0 > 0 entry 0 of the sweep's frame
    table has a non-zero dt_over_tau and frame 1's interval runs from time 0; t0 = 0 gives the same intervals from t[0] on."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = np.arange(height * width)
    walk = np.array([0, 20, 21, 255, 21, 20, 0, 255, 20, 0, 21, 255])
    frames = np.empty((n_frames, height * width), np.uint8)
    for k in range(n_frames):
        frames[k] = (37 * p + 101 * k) % 256
        frames[k, :8] = walk[(k + np.arange(8)) % len(walk)]
    times = t0 + np.concatenate(([0.0], np.cumsum(rng.uniform(0.0004, 0.006, size=n_frames - 1))))
    frames = frames.reshape(n_frames, height, width)
    frames.setflags(write=False)
    times.setflags(write=False)
    return frames, times


@functools.lru_cache(maxsize=None)
def levels_reference(name, t0=LEVELS_T0):
    frames, times = levels_clip(t0)
    model, neg = CONFIGS[name]
    ref = oracle_sweep(frames, times, THRESHOLDS, THRESHOLDS if neg is None else neg, ROI, **model)
    for v in ref.values():
        v.setflags(write=False)
    return ref


CLAMP_CUTOFF_HZ = 100.0


@functools.lru_cache(maxsize=None)
def clamp_clip(seed=22):
    """levels_clip's frames at intervals of 2.5 - 3.5 ms: with CLAMP_CUTOFF_HZ, eps = inten01 * dt / tau passes 1 for the bright
    levels (from about 126 up) and stays below it for the dark ones, in every frame."""
    frames, _ = levels_clip()
    rng = np.random.Generator(np.random.PCG64(seed))
    times = np.cumsum(rng.uniform(0.0025, 0.0035, size=len(frames)))
    times.setflags(write=False)
    return frames, times


def clamp_eps(frames, times, cutoff_hz=CLAMP_CUTOFF_HZ):
    """eps before its clamp, [F][H][W]: (level + 20) / 275 * dt / tau with the emulator's intervals (frames 0 and 1 from time 0)."""
    t_prev = np.concatenate(([0.0, 0.0], times[1:-1]))
    tau = 1.0 / (np.pi * 2 * cutoff_hz)
    return (frames.astype(np.float64) + 20.0) / 275.0 * ((times - t_prev) / tau)[:, None, None]


@functools.lru_cache(maxsize=None)
def clamp_reference(leak):
    frames, times = clamp_clip()
    ref = oracle_sweep(frames, times, THRESHOLDS, THRESHOLDS, ROI, cutoff_hz=CLAMP_CUTOFF_HZ, **({} if leak else dict(leak_rate_hz=0.0)))
    for v in ref.values():
        v.setflags(write=False)
    return ref


# per-pixel thresholds drawn around 0.02 and 0.04 with sigma 0.03 fall below 0.01 on many pixels: k_init's clamp
THRES_CLAMP = dict(thresholds=(0.02, 0.04, 0.2), frames=12, model=dict(sigma_thres=0.03, refractory_period_s=0.0))


@functools.lru_cache(maxsize=None)
def thres_clamp_reference():
    frames, times = clip()
    n = THRES_CLAMP["frames"]
    ref = oracle_sweep(frames[:n], times[:n], THRES_CLAMP["thresholds"], THRES_CLAMP["thresholds"], ROI, **THRES_CLAMP["model"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


def thres_clamp_fraction():
    """The share of pixels whose ON (OFF) threshold in the smallest column is the clamp's 0.01, from the oracle's arrays."""
    from oracle import oracle as orc
    frames, times = clip()
    t = min(THRES_CLAMP["thresholds"])
    emu = orc.OracleEmulator(pos_thres=t, neg_thres=t, rng_mode="philox", seed=SEED, shot_noise_rate_hz=0.0, **THRES_CLAMP["model"])
    emu.generate_events(frames[0], float(times[0]))
    return float(np.mean(emu.pos_thres_arr == np.float32(0.01))), float(np.mean(emu.neg_thres_arr == np.float32(0.01)))


LONE_PIXEL = (0, 0)  # (x, y), outside ROI
LONE_FRAME = 5


def lone_pixel_clip(lone=True, height=37, width=33, n_frames=12):
    """(frames, times) for CONFIGS["refractory"]: every pixel climbs 3 grey levels per frame from 100 + (x + y) % 7 (an event every
    few frames, never two in one), t[k] = k ms.  With `lone`, pixel LONE_PIXEL -- outside ROI -- jumps 60 levels higher from frame
    LONE_FRAME on: three or more events in that frame at the smaller thresholds, which switches the refractory rule on for the
    whole frame (refr_on_n = 3)."""
    y, x = np.mgrid[0:height, 0:width]
    frames = np.stack([100 + (x + y) % 7 + 3 * k for k in range(n_frames)]).astype(np.uint8)
    if lone:
        frames[LONE_FRAME:, LONE_PIXEL[1], LONE_PIXEL[0]] += 60
    return frames, np.arange(n_frames, dtype=np.float64) * 1e-3


@functools.lru_cache(maxsize=None)
def lone_pixel_reference(lone=True):
    frames, times = lone_pixel_clip(lone)
    model, _ = CONFIGS["refractory"]
    ref = oracle_sweep(frames, times, THRESHOLDS, THRESHOLDS, ROI, **model)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def prefix_reference(name, n_frames, roi=ROI):
    """The oracle's sweep of the first n_frames frames of the test clip under CONFIGS[name]."""
    model, neg = CONFIGS[name]
    frames, times = clip()
    ref = oracle_sweep(frames[:n_frames], times[:n_frames], THRESHOLDS, THRESHOLDS if neg is None else neg, roi, **model)
    for v in ref.values():
        v.setflags(write=False)
    return ref


SMALL_SENSORS = ((1, 1), (1, 70), (67, 1), (5, 7))  # (height, width): less than a wave, and one or two workgroups of mostly idle lanes
SMALL_THRESHOLDS = (0.13, 0.2, 0.31)


@functools.lru_cache(maxsize=None)
def small_sensor_case(height, width, one_pixel):
    """(frames, times, roi, oracle reference) of make_clip at a tiny size, 12 frames, default model, T = 3; the ROI is the whole
    sensor or its middle pixel."""
    frames, times = make_clip(height, width, 12)
    roi = ((width // 2, width // 2), (height // 2, height // 2)) if one_pixel else ((0, width - 1), (0, height - 1))
    return frames, times, roi, oracle_sweep(frames, times, SMALL_THRESHOLDS, SMALL_THRESHOLDS, roi)
