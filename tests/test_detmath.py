"""include/v2e_detmath.h against references that do not share its code (CPU, through the oracle library's array loops).

The header is compiled verbatim into the HIP kernels and into the oracle, and every Philox-mode fixture was generated from it: a bug
in it is common-mode, kernel and oracle still agree.  Here its Philox is held to the published known answers and to an independent
numpy implementation, its stream layout to a recomputation from that, its logarithm / sine / cosine / exponential / Box-Muller to
float64 on their whole domains where those are finite, its sinh and timestamp formula to torch bit for bit.
tests/test_detmath_gpu.py then holds the device to the host on the same arguments."""
import numpy as np
import pytest

import detmath_cases as dc

SEEDS = [(0xC0FFEE12 << 32) | 0x9E3779B1, 123456789]   # a non-zero high word; below 2^32
PIXELS = np.asarray([0, 1, 1 << 20, 921599], np.uint32)


def _requires_vectorised_torch():
    """torch.sinh / torch.linspace on float32 are the Sleef / fused vector kernels the header restates only in an AVX2 or AVX-512
    build of ATen: elsewhere the comparison says nothing about the header and is skipped (the rule of LiveTapeFixture)."""
    import torch
    cap = torch.backends.cpu.get_cpu_capability()
    if cap not in ("AVX2", "AVX512"):
        pytest.skip("torch's CPU kernels here are the %s build, not the AVX2 / AVX-512 one the header restates" % cap)
    return torch


# ------------------------------------------------------------------ 1. Philox
def test_philox_known_answers(oracle_lib):
    """The three published vectors, from the header (plain and key-schedule forms) and from the independent implementation."""
    for ctr, key, want in dc.KNOWN_ANSWERS:
        want = np.asarray([want], np.uint32)
        assert np.array_equal(oracle_lib.philox_words([ctr], *key), want), ctr
        assert np.array_equal(oracle_lib.philox_words([ctr], *key, key_schedule=True), want), ctr
        assert np.array_equal(dc.philox_ref([ctr], *key), want), ctr


def test_philox_matches_independent_implementation(oracle_lib):
    """2^16 random counters -- 2048 of them each under a random key of its own, the rest under 16 random keys (the oracle's loop takes
    one key per call) -- and every counter and key with a single bit set (a hi / lo or word swap moves those)."""
    rng = np.random.Generator(np.random.PCG64(2))
    n = 1 << 16
    ctr = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint32)
    keys = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint32)
    want = dc.philox_ref(ctr, keys[:, 0], keys[:, 1])
    for ks in (False, True):
        got = np.concatenate([oracle_lib.philox_words(ctr[i:i + 1], int(keys[i, 0]), int(keys[i, 1]), key_schedule=ks) for i in range(2048)])
        assert np.array_equal(got, want[:2048]), ks
    # the other counters under 16 keys, 4096 counters each
    for g in range(16):
        sl = slice(g * 4096, (g + 1) * 4096)
        k0, k1 = int(keys[g, 0]), int(keys[g, 1])
        want_g = dc.philox_ref(ctr[sl], k0, k1)
        assert np.array_equal(oracle_lib.philox_words(ctr[sl], k0, k1), want_g), g
        assert np.array_equal(oracle_lib.philox_words(ctr[sl], k0, k1, key_schedule=True), want_g), g
    one = np.zeros((128, 4), np.uint32)
    for w in range(4):
        one[32 * w + np.arange(32), w] = np.uint32(1) << np.arange(32, dtype=np.uint32)
    for k0, k1 in [(0, 0), (0x12345678, 0x9ABCDEF0)]:
        assert np.array_equal(oracle_lib.philox_words(one, k0, k1), dc.philox_ref(one, k0, k1))
    zero = np.zeros((1, 4), np.uint32)
    for bit in range(32):
        for k0, k1 in [(1 << bit, 0), (0, 1 << bit)]:
            want1 = dc.philox_ref(zero, k0, k1)
            assert np.array_equal(oracle_lib.philox_words(zero, k0, k1), want1), (k0, k1)
            assert np.array_equal(oracle_lib.philox_words(zero, k0, k1, key_schedule=True), want1), (k0, k1)


# ------------------------------------------------------------------ 2. stream layout
def _close(got, want):
    return np.max(np.abs(got.astype(np.float64) - want)) <= dc.NORMAL_ABS_BOUND


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("clip", [0, 5])
def test_stream_layout(oracle_lib, seed, clip):
    """Every draw recomputed from the independent Philox and a float64 Box-Muller: counter = (pixel, pair or frame, stream id, clip),
    key = (seed low, seed high).  Which word feeds which draw: threshold normals from words (0,1) and (2,3) of stream 1, the rate
    normal from (0,1) and the SCIDVS normal from (2,3) of stream 2, the photoreceptor-noise normal from (0,1) of stream 4 at the FRAME;
    of stream 0 at the PAIR (frame + 1) >> 1: cosine branch and word [2] -> the odd frame, sine branch and word [3] -> the even frame.
    Uniforms exactly, normals within the bound of test_normal2_accuracy."""
    def at(fn):   # the oracle's loop over a pixel range, at each of the pixels
        cols = [fn(int(p)) for p in PIXELS]
        return [np.concatenate([np.atleast_1d(c[k]) for c in cols]) for k in range(len(cols[0]))]

    w = dc.stream_words(seed, clip, dc.STREAM_THRES, 0, PIXELS)
    r = dc.stream_words(seed, clip, dc.STREAM_RATE, 0, PIXELS)
    n_pos, n_neg, n_rate = at(lambda p: oracle_lib.draw_init(seed, clip, p, 1))
    assert _close(n_pos, dc.box_muller_ref(w[:, 0], w[:, 1])[0]) and _close(n_neg, dc.box_muller_ref(w[:, 2], w[:, 3])[0])
    assert _close(n_rate, dc.box_muller_ref(r[:, 0], r[:, 1])[0])
    (n_sc,) = at(lambda p: (oracle_lib.draw_scidvs(seed, clip, p, 1),))
    assert _close(n_sc, dc.box_muller_ref(r[:, 2], r[:, 3])[0])
    for frame in range(7):
        pw = dc.stream_words(seed, clip, dc.STREAM_PNOISE, frame, PIXELS)
        (pn,) = at(lambda p: (oracle_lib.draw_pnoise(seed, clip, frame, p, 1),))
        assert _close(pn, dc.box_muller_ref(pw[:, 0], pw[:, 1])[0]), frame
        pair = (frame + 1) >> 1
        fw = dc.stream_words(seed, clip, dc.STREAM_FRAME, pair, PIXELS)
        n_cos, n_sin = dc.box_muller_ref(fw[:, 0], fw[:, 1])
        odd = frame % 2 == 1
        leak, shot = at(lambda p: oracle_lib.draw_frame(seed, clip, frame, p, 1))
        assert _close(leak, n_cos if odd else n_sin), frame
        assert np.array_equal(shot, dc.u01_ref(fw[:, 2] if odd else fw[:, 3])), frame
        for ks in (False, True):
            (quad,) = at(lambda p: (oracle_lib.draw_pair(seed, clip, pair, p, 1, key_schedule=ks),))
            quad = quad.reshape(-1, 4)
            assert _close(quad[:, 0], n_cos) and _close(quad[:, 2], n_sin), (frame, ks)
            assert np.array_equal(quad[:, 1], dc.u01_ref(fw[:, 2])) and np.array_equal(quad[:, 3], dc.u01_ref(fw[:, 3])), (frame, ks)
        (quad0,) = at(lambda p: (oracle_lib.draw_pair(seed, clip, pair, p, 1, want_normal=False),))
        quad0 = quad0.reshape(-1, 4)
        assert not quad0[:, 0].any() and not quad0[:, 2].any() and np.array_equal(quad0[:, 1], dc.u01_ref(fw[:, 2]))


def test_stream_layout_over_a_pixel_range(oracle_lib):
    """The same over 4096 consecutive pixels ending at 921 599 (the last of 1280 x 720): the loops' pixel0 + i, and more words."""
    seed, clip, n = SEEDS[0], 5, 4096
    px = np.arange(921600 - n, 921600, dtype=np.uint32)
    w = dc.stream_words(seed, clip, dc.STREAM_THRES, 0, px)
    r = dc.stream_words(seed, clip, dc.STREAM_RATE, 0, px)
    n_pos, n_neg, n_rate = oracle_lib.draw_init(seed, clip, int(px[0]), n)
    assert _close(n_pos, dc.box_muller_ref(w[:, 0], w[:, 1])[0]) and _close(n_neg, dc.box_muller_ref(w[:, 2], w[:, 3])[0])
    assert _close(n_rate, dc.box_muller_ref(r[:, 0], r[:, 1])[0])
    assert _close(oracle_lib.draw_scidvs(seed, clip, int(px[0]), n), dc.box_muller_ref(r[:, 2], r[:, 3])[0])
    for frame in (5, 6):
        fw = dc.stream_words(seed, clip, dc.STREAM_FRAME, 3, px)
        leak, shot = oracle_lib.draw_frame(seed, clip, frame, int(px[0]), n)
        assert _close(leak, dc.box_muller_ref(fw[:, 0], fw[:, 1])[frame % 2 == 0])
        assert np.array_equal(shot, dc.u01_ref(fw[:, 2 + (frame % 2 == 0)]))
    # the older whole-plane taps are the same streams from pixel 0
    a, b = oracle_lib.philox_frame(seed, clip, 5, 64)
    a2, b2 = oracle_lib.draw_frame(seed, clip, 5, 0, 64)
    assert np.array_equal(a.view(np.uint32), a2.view(np.uint32)) and np.array_equal(b, b2)


# ------------------------------------------------------------------ 3. accuracy
def test_det_logf_accuracy_exhaustive(oracle_lib):
    """v2e_det_logf on ALL 2^24 values of v2e_u01_open0 against float64: max error < 2.6 ulp.
    Measured (exhaustive, so a constant): 2.508 ulp at x = 13 088 785 * 2^-24 (k = 13 088 784), max abs error 5.1e-7; log(1) = +0."""
    x = dc.logf_args()
    y = oracle_lib.det_logf(x)
    ref = np.log(x.astype(np.float64))
    err = dc.ulp_error(y, ref)
    k = int(np.argmax(err))
    print("det_logf: max %.4f ulp at k = %d, max abs %.3e" % (err[k], k, np.max(np.abs(y - ref))))
    assert err[k] < 2.6, (err[k], k)
    assert np.max(np.abs(y.astype(np.float64) - ref)) < 6e-7
    assert y[-1] == 0 and not np.signbit(y[-1]) and x[-1] == 1
    assert np.all(y[:-1] < 0)


def test_det_sincos2pi_accuracy_exhaustive(oracle_lib):
    """v2e_det_sincos2pi on ALL 2^24 values of v2e_u01: max abs error <= 1.2e-7 for sine and cosine, s^2 + c^2 within 3e-7 of 1,
    exact at the quadrant points.  Measured: 1.067e-7 (sine), 1.067e-7 (cosine), |s^2 + c^2 - 1| <= 1.54e-7."""
    u = dc.sincos_args()
    s, c = oracle_lib.det_sincos2pi(u)
    ang = 2 * np.pi * u.astype(np.float64)
    es, ec = np.max(np.abs(s - np.sin(ang))), np.max(np.abs(c - np.cos(ang)))
    norm = np.max(np.abs(s.astype(np.float64) ** 2 + c.astype(np.float64) ** 2 - 1))
    print("det_sincos2pi: max abs error sine %.4e cosine %.4e, |s^2 + c^2 - 1| <= %.3e" % (es, ec, norm))
    assert es <= 1.2e-7 and ec <= 1.2e-7, (es, ec)
    assert norm <= 3e-7, norm
    # u = 0, 1/4, 1/2, 3/4: (0, 1), (1, 0), (0, -1), (-1, 0); the zeros' signs as the quadrant selects define them
    q = np.asarray([0, 1 << 22, 1 << 23, 3 << 22])
    bits = lambda v: np.asarray(v, np.float32).view(np.uint32).tolist()
    assert bits(s[q]) == bits([0.0, 1.0, -0.0, -1.0]), s[q]
    assert bits(c[q]) == bits([1.0, -0.0, -1.0, 0.0]), c[q]


def test_det_expf_accuracy(oracle_lib):
    """v2e_det_expf against float64 on 12.6 M grid points over [-80, 80], on the arguments the kernels form (ln10cov_f * n and 0.5f * n
    over 2^20 draws each), on the rintf ties and at +-80, +-0: max error <= 1.1 ulp.
    Measured: 1.023 ulp on the grid, 0.881 ulp on the kernels' arguments, 0.966 ulp on the ties; exp(+-0) = 1 exactly."""
    x = dc.expf_args(oracle_lib)
    y = oracle_lib.det_expf(x)
    err = dc.ulp_error(y, np.exp(x.astype(np.float64)))
    g, t = dc.EXPF_GRID, len(dc.expf_tie_args())
    print("det_expf: max ulp grid %.4f, consumers %.4f, ties %.4f, edges %.4f"
          % (err[:g].max(), err[g:g + (2 << 20)].max(), err[g + (2 << 20):-4].max(), err[-4:].max()))
    assert len(x) == g + (2 << 20) + t + 4
    k = int(np.argmax(err))
    assert err[k] <= dc.EXPF_ULP_BOUND, (err[k], x[k])
    assert y[-2] == 1 and y[-1] == 1


@pytest.fixture(scope="module")
def normal2_host(oracle_lib):
    """v2e_normal2 on the four b sets (shared by the accuracy and the edge test; never written to)"""
    return [oracle_lib.normal2(*dc.normal2_args(j)) for j in range(dc.NORMAL2_B_SETS)]


def test_normal2_accuracy(oracle_lib, normal2_host):
    """v2e_normal2 against float64 Box-Muller for every a (top 24 bits) with four b each, quadrant boundaries k 2^30 +- 256 among
    them: abs error <= 1e-6 on both branches.  Measured: 7.20e-7 (cosine branch), 8.19e-7 (sine branch)."""
    worst = [0.0, 0.0]
    for j in range(dc.NORMAL2_B_SETS):
        a, b = dc.normal2_args(j)
        want = dc.box_muller_ref(a, b)
        for h in range(2):
            worst[h] = max(worst[h], float(np.max(np.abs(normal2_host[j][h] - want[h]))))
    print("normal2: max abs error cosine branch %.3e sine branch %.3e" % tuple(worst))
    assert max(worst) <= dc.NORMAL_ABS_BOUND, worst


def test_normal2_edges(oracle_lib, normal2_host):
    """u1 = 1 (a >= 0xFFFFFF00): the logarithm is +0, the radius sqrt(-0) = -0, so both branches are zeros signed against the
    trigonometric factor -- pinned as it is.  u1 = 2^-24 (a < 256): the largest radius, sqrt(48 ln 2) = 5.768, which with b = 0 is
    the largest draw there is."""
    for j in range(dc.NORMAL2_B_SETS):
        a, b = dc.normal2_args(j)
        top = a >= 0xFFFFFF00
        assert top.sum() == 1
        s, c = oracle_lib.det_sincos2pi(dc.u01_ref(b[top]))
        nc, ns = normal2_host[j][0][top], normal2_host[j][1][top]
        assert np.array_equal(nc.view(np.uint32), (np.float32(-0.0) * c).view(np.uint32))
        assert np.array_equal(ns.view(np.uint32), (np.float32(-0.0) * s).view(np.uint32))
    a = np.arange(0xFFFFFF00, 1 << 32, dtype=np.uint64).astype(np.uint32)
    nc, ns = oracle_lib.normal2(a, np.full_like(a, 12345 << 8))   # a first-quadrant angle: -0 on both branches
    assert np.all(nc.view(np.uint32) == 0x80000000) and np.all(ns.view(np.uint32) == 0x80000000)
    a = np.arange(256, dtype=np.uint32)
    nc, ns = oracle_lib.normal2(a, np.zeros_like(a))
    assert np.all(np.abs(nc.astype(np.float64) - np.sqrt(48 * np.log(2.0))) <= dc.NORMAL_ABS_BOUND) and not ns.any()
    biggest = max(float(np.max(np.abs(h))) for pair in normal2_host for h in pair)
    assert biggest <= float(nc[0]), biggest


# ------------------------------------------------------------------ 4. sinhf == torch.sinh
def test_sleef_sinhf_equals_torch_sinh(oracle_lib):
    """v2e_sleef_sinhf == torch.sinh on float32 CPU tensors, bit for bit, on 2^20 arguments over [-89.5, 89.5] and down to 1e-38
    (what tests/golden/make_golden_scidvs.py asserts before it writes a fixture)."""
    torch = _requires_vectorised_torch()
    x = dc.sinhf_args()
    assert x.size % 64 == 0
    t = torch.sinh(torch.from_numpy(x)).numpy()
    y = oracle_lib.sleef_sinhf(x)
    diff = np.flatnonzero(y.view(np.uint32) != t.view(np.uint32))
    assert diff.size == 0, (diff.size, x[diff[:4]], y[diff[:4]], t[diff[:4]])


# ------------------------------------------------------------------ 5. ts_formula == torch.linspace
def test_ts_formula_equals_torch_linspace(oracle_lib):
    """v2e_ts_formula == torch.linspace(t_prev + dt / n, t_frame, n, float32), bit for bit, for n = 1 .. 200, 256, 513, 1000 and 40
    random frames each -- through the oracle's v2e_oracle_ts, and with start, end and step formed here as the kernels' TsGen does."""
    torch = _requires_vectorised_torch()
    cases = dc.ts_cases()
    assert len(cases) == 203 * 40
    want = []
    for t_prev, t_frame, n in cases:
        ts_step = (t_frame - t_prev) / n
        ref = torch.linspace(start=t_prev + ts_step, end=t_frame, steps=n, dtype=torch.float32).numpy()
        got = oracle_lib.ts_formula(t_prev, t_frame, n)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (t_prev, t_frame, n)
        want.append(ref)
    got = oracle_lib.ts_formula_arr(*dc.ts_elements(cases))
    assert np.array_equal(got.view(np.uint32), np.concatenate(want).view(np.uint32))


# ------------------------------------------------------------------ 6. bijection
def test_bijection_for_every_small_n(oracle_lib):
    """v2e_perm_apply is a bijection on [0, n) and v2e_perm_invert its inverse for EVERY n in 1 .. 4100: the shape of the domain
    split changes at the powers of two and of four."""
    for n in range(1, 4101):
        idx = oracle_lib.perm_idx(3, 0, n, n % 5, n)   # idx[apply(c)] = c
        assert np.array_equal(np.sort(idx), np.arange(n)), n
        assert np.array_equal(oracle_lib.perm_inv_idx(3, 0, n, n % 5, n), idx), n
    c = np.arange(4100, dtype=np.uint32)
    fwd = oracle_lib.perm_map(3, 0, 4100, 0, 4100, c)
    assert np.array_equal(oracle_lib.perm_map(3, 0, 4100, 0, 4100, fwd, invert=True), c)
    assert np.array_equal(oracle_lib.perm_idx(3, 0, 4100, 0, 4100)[fwd], c)


def test_bit_select_array_form(oracle_lib):
    """the array loop over v2e_nth_set_bit_256 (what the device is compared with) against numpy on the masks of
    test_inverse_bijection_and_group_bit_select, every r"""
    m, r, want = dc.bit_select_cases()
    assert np.array_equal(oracle_lib.nth_set_bit_256_arr(m, r), want)


def test_function_table_matches_header():
    import os
    import re
    from v2e_amd import _capi
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "v2e_amd.h")).read()
    body = re.search(r"enum \{\s*(V2E_DM_PHILOX = 0.*?), V2E_DM_COUNT", src, flags=re.S).group(1)
    names = [s.strip().split(" ")[0].replace("V2E_DM_", "") for s in body.split(",")]
    assert tuple(names) == _capi.DM_FUNCTIONS


def test_seed_above_2_32_reaches_the_kernels_whole():
    """A Philox seed keys the streams with both of its words: the Python class takes one above 2^32 (numpy's generator, which takes
    32 bits, gets the low word there; the constructor used to raise) and hands all 64 bits to the C struct.  On the device:
    tests/test_detmath_gpu.py::test_first_frame_planes_in_situ_at_1280x720."""
    from v2e_amd import EventEmulator
    for seed in SEEDS + [2 ** 64 - 1]:
        emu = EventEmulator(seed=seed, rng_mode="philox")
        emu._thres_scalar = (0.2, 0.2)
        assert emu._params().seed == seed
    with pytest.raises(ValueError):   # tape mode seeds numpy like the reference, which raises
        EventEmulator(seed=SEEDS[0], rng_mode="tape")
