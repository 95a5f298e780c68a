"""What tests/test_detmath.py (the header against independent references, CPU) and tests/test_detmath_gpu.py (device == host, bit
for bit) share: an independent Philox4x32-10 and float64 Box-Muller, and the argument sets of include/v2e_detmath.h's functions.
Every set is deterministic, so the figures in the tests' docstrings are constants."""
import functools

import numpy as np

# ------------------------------------------------------------------ independent references
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)   # Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11), table 2
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)   # the Weyl constants of the key: golden ratio, sqrt(3) - 1
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

STREAM_FRAME, STREAM_THRES, STREAM_RATE, STREAM_PNOISE = 0, 1, 2, 4


def _philox_round(c, k0, k1):
    """one round of the paper's Philox-4x32: (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))"""
    p0, p1 = _M0 * c[0], _M1 * c[2]   # 32 x 32 -> 64 bits: no overflow in uint64
    return [(p1 >> _S32) ^ c[1] ^ k0, p1 & _LO, (p0 >> _S32) ^ c[3] ^ k1, p0 & _LO]


def philox_ref(ctr, k0, k1):
    """Philox4x32-10 of the counters ctr[n][4] under keys k0, k1 (scalars or [n]) in numpy uint64 arithmetic: uint32 [n][4].
    Written from the paper, round function first, the key bumped before every round but the first."""
    ctr = np.asarray(ctr, dtype=np.uint64).reshape(-1, 4)
    c = [ctr[:, j].copy() for j in range(4)]
    k0 = np.broadcast_to(np.asarray(k0, dtype=np.uint64), c[0].shape).copy()
    k1 = np.broadcast_to(np.asarray(k1, dtype=np.uint64), c[0].shape).copy()
    c = _philox_round(c, k0, k1)
    for _ in range(9):
        k0 = (k0 + _W0) & _LO
        k1 = (k1 + _W1) & _LO
        c = _philox_round(c, k0, k1)
    return np.stack(c, axis=1).astype(np.uint32)


def stream_words(seed, clip, stream, index, pixels):
    """the four words of counter (pixel, index, stream id, clip) under key (seed low, seed high), by philox_ref"""
    pixels = np.asarray(pixels, dtype=np.uint64)
    ctr = np.stack([pixels, np.full_like(pixels, index), np.full_like(pixels, stream), np.full_like(pixels, clip)], axis=1)
    return philox_ref(ctr, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def u01_ref(w):
    """(w >> 8) * 2^-24 as float32: exact"""
    return ((np.asarray(w, dtype=np.uint32) >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def box_muller_ref(a, b):
    """float64 Box-Muller of the words (a, b): u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24; (r cos 2 pi u2, r sin 2 pi u2)"""
    u1 = ((np.asarray(a, dtype=np.uint32) >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(b, dtype=np.uint32) >> 8).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)


def ulp_error(y, ref):
    """|y - ref| in float32 spacings at |ref| (the convention of test_sleef_sinhf_restatement_properties)"""
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(y, dtype=np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------ argument sets
# (counter, key, output): Random123's kat_vectors for philox4x32-10
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

N24 = 1 << 24
NORMAL_ABS_BOUND = 1e-6   # v2e_normal2 against float64 Box-Muller (tests/test_detmath.py::test_normal2_accuracy measures 8.2e-7)
EXPF_ULP_BOUND = 1.1      # v2e_det_expf against float64 exp


def logf_args():
    """every value of v2e_u01_open0: (k + 1) 2^-24, k = 0 .. 2^24 - 1"""
    return ((np.arange(N24, dtype=np.float64) + 1.0) * 2.0 ** -24).astype(np.float32)


def sincos_args():
    """every value of v2e_u01: k 2^-24"""
    return (np.arange(N24, dtype=np.float64) * 2.0 ** -24).astype(np.float32)


LOG2E_F = np.float32(1.44269504089)
LN10COV_F = np.float32(np.log(10.0) * 0.1)   # emu_kernels.h / emu_oracle.c: (float)(log(10) * noise_rate_cov_decades), the default 0.1
EXPF_GRID = N24 - (1 << 22)
EXPF_SEED = (0x5EED << 32) | 77


def expf_tie_args():
    """arguments whose product with the header's float32 log2(e) lies within an ulp of a half-integer (rintf's tie): for every
    half-integer h with |h / log2(e)| < 80, the float32 nearest h / log2(e) and its four neighbours on either side"""
    h = np.arange(-115, 115, dtype=np.float64) + 0.5
    x0 = (h / np.float64(LOG2E_F)).astype(np.float32)
    xs = [x0]
    lo = hi = x0
    for _ in range(4):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        xs += [lo, hi]
    x = np.concatenate(xs)
    x = x[np.abs(x) <= 80]
    prod = x * LOG2E_F   # float32, as the header forms it
    near = np.abs(prod.astype(np.float64) - (np.floor(prod.astype(np.float64)) + 0.5)) <= np.spacing(np.abs(prod)).astype(np.float64)
    assert near.sum() >= 3 * len(h) - 20, "the tie set misses rintf's ties"
    return x


def expf_args(oracle_lib):
    """a grid of 12 582 912 points over [-80, 80] (step 1.27e-5); the arguments the kernels form -- ln10cov_f * n over the 2^20
    noise-rate normals and 0.5f * n over the 2^20 SCIDVS normals of one seed; the rintf ties; +-80 and +-0"""
    grid = (-80.0 + np.arange(EXPF_GRID, dtype=np.float64) * (160.0 / (EXPF_GRID - 1))).astype(np.float32)
    _, _, n_rate = oracle_lib.draw_init(EXPF_SEED, 0, 0, 1 << 20)
    n_sc = oracle_lib.draw_scidvs(EXPF_SEED, 0, 0, 1 << 20)
    edge = np.asarray([80.0, -80.0, 0.0, -0.0], np.float32)
    x = np.concatenate([grid, LN10COV_F * n_rate, np.float32(0.5) * n_sc, expf_tie_args(), edge])
    assert x.dtype == np.float32 and x.size <= N24
    return x


NORMAL2_B_SETS = 4


@functools.lru_cache(maxsize=None)
def normal2_args(j):
    """b set j of 4 for every a: a = k << 8 | (low bits, which v2e_u01_open0 drops), k = 0 .. 2^24 - 1, so every u1 occurs -- u1 = 1
    (a >= 0xFFFFFF00, radius 0) and u1 = 2^-24 (a < 256, the largest radius) included; b = j 2^30 + 256 for k = 0 mod 4,
    j 2^30 - 256 for k = 1 mod 4 (either side of a quadrant boundary of v2e_det_sincos2pi), random words otherwise"""
    rng = np.random.Generator(np.random.PCG64(1000 + j))
    k = np.arange(N24, dtype=np.uint32)
    a = (k << np.uint32(8)) | rng.integers(0, 256, N24, dtype=np.uint32)
    b = rng.integers(0, 1 << 32, N24, dtype=np.uint32)
    b[0::4] = np.uint32((j << 30) + 256)
    b[1::4] = np.uint32(((j << 30) - 256) & 0xFFFFFFFF)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def sinhf_args():
    """2^20 float32 arguments (a multiple of 64: torch's vectorised sinh has no scalar tail on them): 2^19 evenly over [-89.5, 89.5],
    and 2^18 magnitudes per sign spaced evenly in the logarithm from 1e-38 to 89.5"""
    n = 1 << 19
    lin = (-89.5 + np.arange(n, dtype=np.float64) * (179.0 / (n - 1))).astype(np.float32)
    mag = np.exp(np.log(1e-38) + np.arange(n // 2, dtype=np.float64) * ((np.log(89.5) - np.log(1e-38)) / (n // 2 - 1))).astype(np.float32)
    x = np.concatenate([lin, mag, -mag])
    assert x.size == 1 << 20
    return x


def sinhf_edge_args():
    """+-89, +-89.0001, +-104, +-0, +-inf, NaN, and 2^16 subnormal and near-subnormal arguments: with both signs, every 512th bit
    pattern of the subnormals (0 included) and every 1021st of the normals from 2^-126 to just under 2^-124"""
    sub = (np.arange(1 << 14, dtype=np.uint32) * np.uint32(512)).view(np.float32)             # 0 .. just below 2^-126
    near = (np.uint32(0x00800000) + np.arange(1 << 14, dtype=np.uint32) * np.uint32(1021)).view(np.float32)  # 2^-126 .. 2^-124
    mag = np.concatenate([sub, near])
    pts = np.asarray([89, -89, 89.0001, -89.0001, 104, -104, 0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    x = np.concatenate([mag, -mag, pts])
    assert x.size == (1 << 16) + len(pts)
    return x


TS_COUNTS = list(range(1, 201)) + [256, 513, 1000]
TS_PER_COUNT = 40


def ts_cases():
    """(t_prev, t_frame, n) for n = 1 .. 200, 256, 513, 1000 and 40 random frames each: t_prev in [0, 100) s, intervals from 1e-4 to
    0.1 s evenly in the logarithm -- as Python floats, like the emulator's clock"""
    rng = np.random.Generator(np.random.PCG64(31))
    cases = []
    for n in TS_COUNTS:
        t_prev = rng.uniform(0, 100, TS_PER_COUNT) * (rng.random(TS_PER_COUNT) < 0.9)   # (a tenth start at 0, like a clip's first pair)
        dt = 10.0 ** rng.uniform(-4, -1, TS_PER_COUNT)
        cases += [(float(p), float(p + d), n) for p, d in zip(t_prev, dt)]
    return cases


def ts_elements(cases):
    """the cases element by element: (i, n, start, end, step) with start, end, step formed as TsGen forms them (emu_kernels.h) --
    float64 clock arithmetic rounded to float32, the step a float32 division"""
    i, cnt, st, en, sp = [], [], [], [], []
    for t_prev, t_frame, n in cases:
        ts_step = (t_frame - t_prev) / float(n)
        start, end = np.float32(t_prev + ts_step), np.float32(t_frame)
        step = (end - start) / np.float32(n - 1) if n > 1 else np.float32(0)
        i.append(np.arange(n, dtype=np.uint32))
        cnt.append(np.full(n, n, np.uint32))
        st.append(np.full(n, start, np.float32))
        en.append(np.full(n, end, np.float32))
        sp.append(np.full(n, step, np.float32))
    return tuple(np.concatenate(v) for v in (i, cnt, st, en, sp))


def bit_select_cases():
    """the masks of test_inverse_bijection_and_group_bit_select (tests/test_philox_statistics.py) with every r: (masks uint64 [n][4],
    r [n], expected position [n] from numpy)"""
    rng = np.random.default_rng(5)
    masks = [rng.integers(0, 2 ** 64, 4, dtype=np.uint64) for _ in range(40)]
    masks += [rng.integers(0, 2 ** 64, 4, dtype=np.uint64) & rng.integers(0, 2 ** 64, 4, dtype=np.uint64) &
              rng.integers(0, 2 ** 64, 4, dtype=np.uint64) for _ in range(40)]
    masks += [np.array([0, 0, 0, 1 << 63], np.uint64), np.array([1, 0, 0, 0], np.uint64), np.array([0, 1 << 31, 1 << 32, 0], np.uint64),
              np.full(4, 2 ** 64 - 1, np.uint64)]
    m_all, r_all, want = [], [], []
    for m in masks:
        bits = np.flatnonzero(np.unpackbits(m.view(np.uint8), bitorder="little"))
        m_all.append(np.tile(m, (len(bits), 1)))
        r_all.append(np.arange(len(bits), dtype=np.uint32))
        want.append(bits.astype(np.uint32))
    return np.concatenate(m_all), np.concatenate(r_all), np.concatenate(want)
