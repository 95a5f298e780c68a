"""Input builders and CPU predicates for the tests of k_chain's float-frame and float32-state instantiations
(v2e_amd/csrc/emu_chain.h; tests/test_chain_dtypes.py on the CPU keeps the inputs honest, tests/test_chain_dtypes_gpu.py
compares the device with the oracle on them).  No GPU in here.

* `clip` builds frames of a dtype in the style of test_record8_gpu._clip: non-uniform frame intervals, a redraw every 7th frame,
  and whole columns fixed to the values where frame_record_table's float branch can go wrong (EDGE_VALUES);
* `exact_multiple_clip` makes the quotient of frame_body's floor division an exact integer on most pixel-frames (r0 == 0);
* `fixup_frames` searches, with the oracle's own lin-log values, pixel values whose quotient in float32 state lies so close
  to an integer that the reciprocal estimate floor(am * (1 / theta)) is one off: the two arms of frame_body's fix-up;
* `estimate_off_by_one` / `remainder_zero` say, on the CPU, where that happens.
"""
import numpy as np

LINLOG_F = float.fromhex("0x1.32c352f8fe941p-3")  # (1 / 20) * log(20), emulator_utils.py:34

# every feature on: test_record8_gpu.ALL_ON (tests/test_chain_dtypes.py asserts the two are the same)
ALL_ON = dict(pos_thres=.2, neg_thres=.15, sigma_thres=.03, cutoff_hz=300, leak_rate_hz=.3, shot_noise_rate_hz=3.0,
              leak_jitter_fraction=0.1, refractory_period_s=0.0005)
MAX_ITERS = 1024  # what the device emulators of these tests are built with

_F32_BELOW_20 = float(np.nextafter(np.float32(20.0), np.float32(0.0)))
_F32_ABOVE_20 = float(np.nextafter(np.float32(20.0), np.float32(100.0)))
# whole columns of a float clip without hdr: the lin / log switch and its float32 neighbours, the ends of the grey scale, and
# two values beyond it (inten01 > 1: eps reaches its clamp at a smaller dt_over_tau than any grey level's)
EDGE_VALUES = (0.0, 20.0, _F32_BELOW_20, _F32_ABOVE_20, 255.0, 300.0, 1000.0)
# float64 clips add the float64 neighbours of 20.0 (not float32 values: a frame read as float32 rounds them to 20.0)
EDGE_VALUES_F64 = EDGE_VALUES + (float(np.nextafter(20.0, 0.0)), float(np.nextafter(20.0, 100.0)))
HDR_MAX = 5.55  # natural-log intensities: ln 255 = 5.54


def edge_values(dtype, hdr):
    """The values `clip` fixes whole columns to (column i holds value i); the column behind them alternates every frame."""
    if hdr:
        return (0.0, HDR_MAX)
    return EDGE_VALUES_F64 if np.dtype(dtype) == np.float64 else EDGE_VALUES


def clip(dtype, n, H, W, seed, hdr=False):
    """(frames [n][H][W] of a float `dtype`, times [n]): small steps, a full redraw every 7th frame (many events per pixel: the refractory
    rule switches on), frame intervals drawn from uniform(0.0004, 0.006) (a dt_over_tau per frame).  Float dtypes without hdr:
    values in [0, 255] with fractional parts (float64: not float32 values); with hdr natural-log values in [0, HDR_MAX].  Column i
    holds edge_values(dtype, hdr)[i] on every frame, the column behind them alternates between the ends of the range."""
    dtype = np.dtype(dtype)
    rng = np.random.Generator(np.random.PCG64(seed))
    edges = edge_values(dtype, hdr)
    assert W > len(edges) + 1
    hi = HDR_MAX if hdr else 255.0
    step = hi * 14.0 / 255.0

    assert dtype in (np.float32, np.float64)
    base = rng.uniform(0.0, hi, size=(H, W))
    frames = []
    for i in range(n):
        if i % 7 == 3:
            base = rng.uniform(0.0, hi, size=(H, W))
        else:
            base = np.clip(base + rng.uniform(-step, step, size=(H, W)), 0.0, hi)
        f = base.astype(dtype)
        for c, v in enumerate(edges):
            f[:, c] = v
        f[:, len(edges)] = hi if i % 2 else 0.0  # 0 <-> 255 (hdr: HDR_MAX)
        frames.append(f)
    times = np.cumsum(rng.uniform(0.0004, 0.006, size=n)) + 0.001
    return np.stack(frames), [float(t) for t in times]


# ---------------------------------------------------------------- exact multiples: r0 == 0
EXACT_KW = dict(hdr=True, pos_thres=0.25, neg_thres=0.125, sigma_thres=0.0, cutoff_hz=0, leak_rate_hz=0.0,
                shot_noise_rate_hz=0.0, refractory_period_s=0.0005)
EXACT_KW_NOISY = dict(EXACT_KW, leak_rate_hz=0.3, shot_noise_rate_hz=3.0)


def exact_multiple_clip(n, H, W, seed):
    """(frames float32 [n][H][W], times): multiples of 0.125 in [0, 5.5].  With hdr and no cutoff L is the pixel value itself, the
    state is float64, and with the thresholds of EXACT_KW (binary fractions) every base level is a multiple of 0.125 too: the
    quotient |L - base| / theta is an exact integer as long as no leak has moved the base.  A test feeds the first half with
    EXACT_KW and the second with EXACT_KW_NOISY (leak and shot noise on: the ordinary quotients, from the state the first half left)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 45, size=(H, W))
    frames = []
    for i in range(n):
        if i % 7 == 3:
            base = rng.integers(0, 45, size=(H, W))
        else:
            base = np.clip(base + rng.integers(-3, 4, size=(H, W)), 0, 44)
        frames.append((base * 0.125).astype(np.float32))
    times = np.cumsum(rng.uniform(0.0004, 0.006, size=n)) + 0.001
    return np.stack(frames), [float(t) for t in times]


# ---------------------------------------------------------------- the predicates
def _exact_floor_and_rem(am, theta, R):
    """floor(am / theta) and am - floor * theta of operands held in type R, exactly.  fmod is exact in any format; in a format with
    p more mantissa bits than R's the multiple am - fmod is exact for quotients below 2^p, and so is its division by theta
    (float32 operands in float64: p = 29; float64 operands in longdouble: p = 11 where longdouble is the x87 format).  Where theta
    is a power of two the multiple is am with its low bits cleared and the division only moves the exponent: exact at any quotient."""
    W = np.float64 if np.dtype(R) == np.float32 else np.longdouble
    p = np.finfo(W).nmant - np.finfo(R).nmant
    a, t = np.asarray(am, R).astype(W), np.asarray(theta, R).astype(W)
    rem = np.fmod(a, t)
    q = np.rint((a - rem) / t)
    pow2 = np.frexp(t)[0] == 0.5
    assert p > 0 and np.all((q < 2.0 ** p) | pow2), "quotient beyond what %s holds exactly" % np.dtype(W).name
    return q.astype(np.int64), rem


def estimate(am, theta, R):
    """frame_body's q0 = floor(am * (1 / theta)), every operation rounded to type R."""
    am, theta = np.asarray(am, R), np.asarray(theta, R)
    rbt = (R(1) / theta).astype(R)
    return np.floor((am * rbt).astype(R)).astype(np.int64)


def estimate_off_by_one(am, theta, R):
    """-1 where the estimate q0 is the true floor less one (frame_body's `r0 >= bt` arm), +1 where it is one more (`r0 < 0`),
    0 where it is the true floor.  am = |lp_new - base| and theta as arrays of type R."""
    q, _ = _exact_floor_and_rem(am, theta, R)
    d = estimate(am, theta, R) - q
    assert np.all(np.abs(d) <= 1), "the estimate is more than one off: the kernel's fix-up would not cover it"
    return d


def remainder_zero(am, theta, R):
    """True where am is an exact non-zero multiple of theta (the true remainder, and r0 of a right estimate, is 0)."""
    q, rem = _exact_floor_and_rem(am, theta, R)
    return (rem == 0) & (q > 0)


def frame_quotients(ora_before_base, ora_after_lp, pos_thres, neg_thres, R, leak=None):
    """(am, theta, is_pos) of a frame from the oracle's planes around it: am = |lp_new - base| as the kernel computes it in type R,
    theta the divisor of its sign.  leak: the frame's leak step (float32, per pixel), taken off the base first; None: leak off."""
    base = np.asarray(ora_before_base, R)
    if leak is not None:
        base = (base - np.asarray(leak, np.float32).astype(R)).astype(R)
    diff = (np.asarray(ora_after_lp, R) - base).astype(R)
    is_pos = diff > 0
    theta = np.where(is_pos, np.asarray(pos_thres, R), np.asarray(neg_thres, R)).astype(R)
    return np.abs(diff), theta, is_pos


# ---------------------------------------------------------------- fix-up frames (float32 state)
FIXUP_KW = dict(pos_thres=0.2, neg_thres=0.15, sigma_thres=0.0, cutoff_hz=0, leak_rate_hz=0.0, shot_noise_rate_hz=0.0,
                refractory_period_s=0.0)
# fl(1 / 0.2f) and fl(1 / 0.15f) both lie ABOVE the true reciprocal, so with FIXUP_KW the estimate is never too small (see
# test_chain_dtypes.py).  These two thresholds (55 / 256 and 355 / 2048) have reciprocals that round DOWN, far enough that
# fl(theta * fl(1 / theta)) < 1: the estimate of an exact multiple n theta is n - 1 and r0 == theta, the equality in `r0 >= bt`.
# Few mantissa bits, so that differences of lin-log values (multiples of 2^-22 below 4) hit n theta exactly.
FIXUP_KW_DOWN = dict(FIXUP_KW, pos_thres=0.21484375, neg_thres=0.17333984375)
FIXUP_NEIGHBOURS = 24
FIXUP_BUILT = (1, 2, 3)  # the frames fixup_frames builds (frame 0 initialises the state)


def _oracle_lin_log(orc, x):
    """lin-log (float32) of float32 or float64 pixel values from the oracle itself: one oracle frame holding them, read back from
    base_log_frame."""
    x = np.ascontiguousarray(x, dtype=None if np.asarray(x).dtype == np.float64 else np.float32)
    o = orc.OracleEmulator(seed=1, rng_mode="philox", **FIXUP_KW)
    o.generate_events(x.reshape(1, -1) if x.ndim == 1 else x, 0.0)
    assert o.base_log_frame.dtype == np.float32
    return o.base_log_frame.reshape(x.shape)


def _neighbours(x0, k):
    """x0 [...] float32 -> [..., 2 k + 1]: x0 and its k float32 neighbours on either side (positive values: consecutive bit patterns)."""
    bits = np.ascontiguousarray(x0, dtype=np.float32).view(np.int32)[..., None] + np.arange(-k, k + 1, dtype=np.int32)
    return bits.view(np.float32)


def fixup_frames(orc, kw, H, W, seed):
    """(frames float32 [4][H][W], times, hits [3][H][W]) for float32 state, float32 frames and scalar thresholds (FIXUP_KW; kw may
    add to it what leaves the counts alone).  Frame 0 is uniform in [1, 19].  Frames 1-3 are built per pixel from the oracle's
    state before them so that L(x) - base lies next to n * theta: for n = 1, 2, ... the value x = (base +- n theta) / LINLOG_F and
    its +-24 float32 neighbours (while they stay inside (0, 20): the linear part of lin-log), L of every candidate taken from the
    oracle, and the first candidate kept whose quotient the estimate misses by one or hits with remainder 0.  A third of the pixels
    asks first for an estimate that is too small, a third for one too large, so that both arms get their share.  Frame 1 goes up
    (ON events, pos_thres), frame 2 down (OFF, neg_thres), frame 3 either way by the pixel's parity.  hits: what the kept
    candidate is (-1 / +1 the estimate's error, 2 remainder 0 with a right estimate, 0 no candidate found: an ordinary event)."""
    assert float(kw["cutoff_hz"]) == 0 and not kw.get("hdr") and float(kw["sigma_thres"]) == 0
    rng = np.random.Generator(np.random.PCG64(seed))
    npx = H * W
    times = [0.001, 0.0032, 0.0047, 0.0101]
    ora = orc.OracleEmulator(seed=seed, rng_mode="philox", **kw)
    f0 = rng.uniform(1.0, 19.0, size=(H, W)).astype(np.float32)
    ora.generate_events(f0, times[0])
    thp, thn = np.float32(kw["pos_thres"]), np.float32(kw["neg_thres"])
    frames, hits = [f0], []
    want = np.arange(npx) % 3  # 0: too small first, 1: too large first, 2: whatever comes first
    for k in FIXUP_BUILT:
        base = ora.base_log_frame.reshape(npx).astype(np.float64)
        up = np.full(npx, k == 1) if k < 3 else (np.arange(npx) % 2 == 0)
        theta = np.where(up, thp, thn).astype(np.float32)
        sgn = np.where(up, 1.0, -1.0)
        n_max = int(np.ceil(20.0 * LINLOG_F / float(min(thp, thn))))
        ns = np.arange(1, n_max + 1)
        x0 = ((base[:, None] + sgn[:, None] * ns[None, :] * theta.astype(np.float64)[:, None]) / LINLOG_F)
        ok0 = (x0 > 0.05) & (x0 < 19.95)
        cand = _neighbours(np.where(ok0, x0, 1.0).astype(np.float32), FIXUP_NEIGHBOURS)  # [npx][n][49]
        Lc = _oracle_lin_log(orc, cand.reshape(npx, -1)).reshape(cand.shape)
        b32 = ora.base_log_frame.reshape(npx, 1, 1)
        diff = (Lc - b32).astype(np.float32)
        right_way = np.where(up[:, None, None], diff > 0, diff < 0) & ok0[:, :, None]
        am = np.abs(diff)
        th3 = np.broadcast_to(theta[:, None, None], am.shape)
        amf, thf = np.where(right_way, am, np.float32(1.0)), th3
        off = np.where(right_way, estimate_off_by_one(amf, thf, np.float32), 0)
        zero = right_way & remainder_zero(amf, thf, np.float32)
        kind = np.where(off != 0, off, np.where(zero, 2, 0)).reshape(npx, -1)
        flat = cand.reshape(npx, -1)
        pick = np.full(npx, -1)
        for w, pref in ((0, -1), (1, 1)):
            first = np.argmax(kind == pref, axis=1)
            has = (kind == pref).any(axis=1) & (want == w)
            pick = np.where(has & (pick < 0), first, pick)
        first = np.argmax(kind != 0, axis=1)
        pick = np.where((pick < 0) & (kind != 0).any(axis=1), first, pick)
        # no candidate: the n = 1 value itself (an ordinary event), or the pixel's old value where even that leaves (0, 20)
        centre = FIXUP_NEIGHBOURS
        plain = np.where(ok0[:, 0], flat[:, centre], frames[-1].reshape(npx))
        f = np.where(pick >= 0, flat[np.arange(npx), np.maximum(pick, 0)], plain).astype(np.float32).reshape(H, W)
        hits.append(np.where(pick >= 0, kind[np.arange(npx), np.maximum(pick, 0)], 0).reshape(H, W))
        frames.append(f)
        ora.generate_events(f, times[k])
    return np.stack(frames), times, np.stack(hits)


def fixup_frames_rounded(orc, kw, H, W, seed):
    """(frames uint8 [4][H][W], times): fixup_frames' frames rounded to bytes.  Whatever hit is left is left by chance (the CPU test
    counts them from the oracle's planes: 8 of 3 663 pixel-frames at 33x37, seed 3)."""
    frames, times, _ = fixup_frames(orc, kw, H, W, seed)
    return np.rint(frames).astype(np.uint8), times


def fixup_frames_u8(orc, kw, H, W, seed, n_built=6):
    """(frames uint8 [1 + n_built][H][W], times, hits [n_built][H][W]): the same search among the 256 grey levels, for
    k_chain<float, uint8_t, *> (float32 state reads lin-log from the 256-entry table).  fixup_frames' float values rounded to
    bytes (fixup_frames_rounded) keep a hit only by chance -- their quotients sit within a few float32 steps of an integer, the
    next grey level is 10^5 steps away -- so the bytes are also searched directly: per pixel and built frame every grey level in
    either direction, the first one with a hit kept, a random level where there is none (which also spreads the states the next
    frame searches from)."""
    assert float(kw["cutoff_hz"]) == 0 and not kw.get("hdr") and float(kw["sigma_thres"]) == 0
    rng = np.random.Generator(np.random.PCG64(seed))
    npx = H * W
    times = [float(t) for t in 0.001 + np.cumsum(rng.uniform(0.0004, 0.006, size=1 + n_built))]
    ora = orc.OracleEmulator(seed=seed, rng_mode="philox", **kw)
    f0 = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    ora.generate_events(f0, times[0])
    thp, thn = np.float32(kw["pos_thres"]), np.float32(kw["neg_thres"])
    levels = np.arange(256, dtype=np.uint8)
    Lc = _oracle_lin_log(orc, levels.astype(np.float32))
    frames, hits = [f0], []
    for k in range(1, n_built + 1):
        diff = (Lc[None, :] - ora.base_log_frame.reshape(npx, 1)).astype(np.float32)
        theta = np.where(diff > 0, thp, thn).astype(np.float32)
        am = np.abs(diff)
        fires = am >= theta
        amf = np.where(fires, am, np.float32(1.0))
        off = np.where(fires, estimate_off_by_one(amf, theta, np.float32), 0)
        kind = np.where(off != 0, off, np.where(fires & remainder_zero(amf, theta, np.float32), 2, 0))
        has = (kind != 0).any(axis=1)
        pick = np.where(has, np.argmax(kind != 0, axis=1), rng.integers(0, 256, size=npx))
        frames.append(levels[pick].reshape(H, W))
        hits.append(kind[np.arange(npx), pick].reshape(H, W))
        ora.generate_events(frames[-1], times[k])
    return np.stack(frames), times, np.stack(hits)


# ---------------------------------------------------------------- the cases both test files walk
# a row per k_chain instantiation (state type, frame type) the uint8 tests do not reach, and how a caller gets it
ROWS = {
    "f64state_f32frames": dict(frames=np.float32, state=np.float64, hdr=False, kw=dict(cutoff_hz=300), refr_mixed=0.00012),
    "f64state_f32frames_hdr": dict(frames=np.float32, state=np.float64, hdr=True, kw=dict(cutoff_hz=300), refr_mixed=0.00012),
    "f64state_f32frames_hdr_nocutoff": dict(frames=np.float32, state=np.float64, hdr=True, kw=dict(cutoff_hz=0), refr_mixed=0.00005),
    "f32state_f32frames": dict(frames=np.float32, state=np.float32, hdr=False, kw=dict(cutoff_hz=0), refr_mixed=0.00005),
    "f64state_f64frames": dict(frames=np.float64, state=np.float64, hdr=False, kw=dict(cutoff_hz=300), refr_mixed=0.00012),
    "f32state_f64frames": dict(frames=np.float64, state=np.float32, hdr=False, kw=dict(cutoff_hz=0), refr_mixed=0.00005),
}
SHAPES = {"97x131": (97, 131), "33x37": (33, 37)}  # 12 707 pixels: 50 workgroups, the last one ragged; 1 221: five, the last ragged
VARIANTS = {
    "all_on": {},
    "refractory_heavy": dict(refractory_period_s=0.004),  # the rule on in most frames: redo passes in most launches
    # the alternating column fires some 30 events per pixel on every frame: with 0.0005 s the rule is on in (nearly) EVERY frame.
    # With the row's `refr_mixed` (the median of dt / M over its clips: 120 us with the low-pass, 50 us without) it is on in about
    # half of the frames: launches with and without redo passes, right and wrong speculation
    "refractory_mixed": dict(refractory_period_s=None),
    "scalar_thres": dict(sigma_thres=0.0),
    "no_leak_no_shot": dict(leak_rate_hz=0.0, shot_noise_rate_hz=0.0),
}
N_FRAMES = 75   # two full 32-frame launches and a partial one (at 8 frames per launch: nine and a partial one)
N_WRAP = 260    # 259 run frames: more than the ring of three emission batches of 64 frames
SEED = 7        # the emulators' seed


def case_kw(row, variant="all_on", **extra):
    kw = dict(ALL_ON)
    kw.update(ROWS[row]["kw"])
    if ROWS[row]["hdr"]:
        kw["hdr"] = True
    kw.update(VARIANTS[variant])
    if kw["refractory_period_s"] is None:
        kw["refractory_period_s"] = ROWS[row]["refr_mixed"]
    kw.update(extra)
    return kw


def case_clip(row, shape, n=N_FRAMES):
    H, W = SHAPES[shape]
    seed = 100 + 10 * list(ROWS).index(row) + list(SHAPES).index(shape) + (1000 if n != N_FRAMES else 0)
    return clip(ROWS[row]["frames"], n, H, W, seed, hdr=ROWS[row]["hdr"])


# three clips in one engine (test_multi_clip_engine_equals_single_clips' pattern: thresholds 0.2 / 0.2 drawn per pixel)
MULTI_SEED = 5
MULTI_KW = dict(leak_rate_hz=0.2, shot_noise_rate_hz=4.0, refractory_period_s=0.002)


def multi_clip_case(dtype, cutoff_hz, H=60, W=100, F=8, NC=3):
    """(clips: NC arrays [F][H][W], times [F][NC]: every clip its own frame times, kw)"""
    made = [clip(dtype, F, H, W, 40 + c) for c in range(NC)]
    return [m[0] for m in made], np.array([m[1] for m in made]).T, dict(MULTI_KW, cutoff_hz=cutoff_hz)


def fallback_case():
    """float64 log frames (hdr): the configuration k_chain refuses.  (frames, times, kw)"""
    frames, times = clip(np.float64, 20, 33, 37, 51, hdr=True)
    return frames, times, dict(ALL_ON, hdr=True)


def oracle_run(orc, kw, frames, times, seed=SEED, clip=0, phases=(), watch=None):
    """The oracle over a clip (Philox mode): dict(events [N][4], counts per frame, base, lp, ts, counters (total, on, off), max_count
    the largest per-pixel count of any frame, state the state dtype).  phases: (frame, {attribute: value}) pairs, set on the oracle
    before that frame is fed (the mutable attributes of the emulator, changed between runs).  watch(k, base_before, ora) is called
    behind every frame k >= 1."""
    ora = orc.OracleEmulator(seed=seed, rng_mode="philox", clip=clip, **kw)
    evs, counts, mx = [], [], 0
    for k, (f, t) in enumerate(zip(frames, times)):
        for at, attrs in phases:
            if at == k:
                for name, v in attrs.items():
                    setattr(ora, name, v)
        before = None if (watch is None or k == 0) else ora.base_log_frame.copy()
        e = ora.generate_events(f, t)
        counts.append(0 if e is None else len(e))
        if e is not None:
            evs.append(e)
        if k > 0:
            mx = max(mx, int(ora.last_M))
            if watch is not None:
                watch(k, before, ora)
    return dict(events=np.concatenate(evs) if evs else np.zeros((0, 4), np.float32), counts=counts, base=ora.base_log_frame,
                lp=ora.lp_log_frame, ts=ora.timestamp_mem, counters=(ora.num_events_total, ora.num_events_on, ora.num_events_off),
                max_count=mx, state=ora.base_log_frame.dtype)
