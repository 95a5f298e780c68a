"""include/v2e_detmath.h on the device == on the host, bit for bit (v2e_detmath_eval, v2e_amd/csrc/detmath_eval.hip, against the
oracle library's loops over the same header): on the whole domains of the logarithm and of sine / cosine, and on the argument sets
tests/test_detmath.py holds to float64 -- so the device's division, square root, rintf, fmaf and subnormal handling are put to every
argument, not to those a fixture happens to form, and a translation unit that lost -ffp-contract=off shows.  Every comparison is
equality of bit patterns.  The last test reads the product kernels' own copies of the header at 1280 x 720."""

import numpy as np
import pytest

import detmath_cases as dc

pytestmark = pytest.mark.gpu

SEED = (0xC0FFEE12 << 32) | 0x9E3779B1   # a non-zero high word
CLIP = 5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dm_eval(fn, a, b=None, width=1, two=False):
    """v2e_detmath_eval(fn) of the words a (and b): out0 as uint32 [n] or [n][width]; with two, (out0, out1).  One launch."""
    import torch
    from v2e_amd import _capi
    a = _bits(a)
    per = {"PHILOX": 4, "PHILOX_KS": 4, "NTH_SET_BIT_256": 8, "TS_FORMULA": 4}.get(fn, 1)
    n = a.size // per
    assert a.size == n * per and n <= 1 << 24
    dev = lambda v: None if v is None else torch.tensor(_bits(v).view(np.int32).reshape(-1)).cuda()   # (a copy: some sets are read-only)
    a_d, b_d = dev(a), dev(b)
    out0 = torch.empty(n * width, dtype=torch.int32, device="cuda")
    out1 = torch.empty(n, dtype=torch.int32, device="cuda") if two else None
    _capi.check(_capi.lib().v2e_detmath_eval(_capi.DM_FUNCTIONS.index(fn), _capi.ptr(a_d), _capi.ptr(b_d), _capi.ptr(out0),
                                             _capi.ptr(out1), n, _capi.stream_ptr("cuda")), "v2e_detmath_eval(%s)" % fn)
    torch.cuda.synchronize()
    o0 = out0.cpu().numpy().view(np.uint32)
    o0 = o0.reshape(n, width) if width > 1 else o0
    return (o0, out1.cpu().numpy().view(np.uint32)) if two else o0


def _same(dev, host, args=None):
    """bit patterns equal; on a mismatch, how many and the first few (argument, device, host)"""
    host = _bits(host).reshape(dev.shape)
    bad = np.flatnonzero((dev != host).reshape(len(dev), -1).any(axis=1))
    if bad.size:
        first = bad[:4]
        pytest.fail("%d of %d differ; first at %s: args %s device %s host %s"
                    % (bad.size, len(dev), first.tolist(), None if args is None else np.asarray(args)[first].tolist(),
                       [hex(v) for v in dev[first].reshape(-1)], [hex(v) for v in host[first].reshape(-1)]))


def test_logf_every_argument(oracle_lib):
    """all 2^24 values of v2e_u01_open0 (a division and five fused multiply-adds each)"""
    x = dc.logf_args()
    _same(dm_eval("LOGF", x), oracle_lib.det_logf(x), x)


def test_sincos2pi_every_argument(oracle_lib):
    """all 2^24 values of v2e_u01, both outputs, the sign of zero included"""
    u = dc.sincos_args()
    s, c = dm_eval("SINCOS2PI", u, two=True)
    hs, hc = oracle_lib.det_sincos2pi(u)
    _same(s, hs, u)
    _same(c, hc, u)


def test_expf(oracle_lib):
    """the grid over [-80, 80], the arguments the kernels form, rintf's ties, +-80 and +-0"""
    x = dc.expf_args(oracle_lib)
    _same(dm_eval("EXPF", x), oracle_lib.det_expf(x), x)


@pytest.mark.parametrize("j", range(dc.NORMAL2_B_SETS))
def test_normal2(oracle_lib, j):
    """every a with b set j: u1 = 1 (radius -0: signed zeros on both sides) and a < 256 (the largest radius) included"""
    a, b = dc.normal2_args(j)
    nc, ns = dm_eval("NORMAL2", a, b, two=True)
    hc, hs = oracle_lib.normal2(a, b)
    _same(nc, hc, a)
    _same(ns, hs, a)
    top = a >= 0xFFFFFF00
    assert np.all((nc[top] & 0x7FFFFFFF) == 0) and np.all((ns[top] & 0x7FFFFFFF) == 0)


def test_sleef_sinhf(oracle_lib):
    """the arguments held to torch.sinh on the host, then +-89, +-89.0001, +-104, +-0, +-inf, NaN and 2^16 subnormal and
    near-subnormal arguments: the double-float arithmetic there is where a device that flushed subnormals would differ"""
    x = np.concatenate([dc.sinhf_args(), dc.sinhf_edge_args()])
    _same(dm_eval("SLEEF_SINHF", x), oracle_lib.sleef_sinhf(x), x)


def test_philox(oracle_lib):
    """2^20 random counters and the three known answers, plain and key-schedule forms"""
    rng = np.random.Generator(np.random.PCG64(3))
    ctr = rng.integers(0, 1 << 32, (1 << 20, 4), dtype=np.uint32)
    key = np.asarray([0x85A308D3, 0x13198A2E], np.uint32)
    host = oracle_lib.philox_words(ctr, int(key[0]), int(key[1]))
    assert np.array_equal(host[:4096], dc.philox_ref(ctr[:4096], int(key[0]), int(key[1])))
    for fn in ("PHILOX", "PHILOX_KS"):
        _same(dm_eval(fn, ctr, key, width=4), host, ctr)
        for c, k, want in dc.KNOWN_ANSWERS:
            assert dm_eval(fn, np.asarray([c], np.uint32), np.asarray(k, np.uint32), width=4).tolist() == [list(want)], (fn, c)


def test_bijection(oracle_lib):
    """v2e_perm_apply and v2e_perm_invert for every index of ten domain sizes under two keys"""
    for n in (1, 2, 3, 5, 255, 256, 257, 4097, 35000, 131071):
        c = np.arange(n, dtype=np.uint32)
        for seed, clip, frame, it in ((3, 0, 17, 2), (SEED, 5, 123456, 0)):
            par = np.asarray([n, seed & 0xFFFFFFFF, seed >> 32, clip, frame, it], np.uint32)
            fwd = dm_eval("PERM_APPLY", c, par)
            _same(fwd, oracle_lib.perm_map(seed, clip, frame, it, n, c), c)
            _same(dm_eval("PERM_INVERT", c, par), oracle_lib.perm_map(seed, clip, frame, it, n, c, invert=True), c)
            assert np.array_equal(dm_eval("PERM_INVERT", fwd, par), c), n


def test_nth_set_bit_256(oracle_lib):
    m, r, want = dc.bit_select_cases()
    got = dm_eval("NTH_SET_BIT_256", m, r)
    _same(got, oracle_lib.nth_set_bit_256_arr(m, r), r)
    assert np.array_equal(got, want)


def test_ts_formula(oracle_lib):
    """the cases held to torch.linspace on the host, start / end / step formed as the kernels' TsGen forms them"""
    i, cnt, start, end, step = dc.ts_elements(dc.ts_cases())
    a = np.stack([i, cnt, _bits(start), _bits(end)], axis=1)
    _same(dm_eval("TS_FORMULA", a, step), oracle_lib.ts_formula_arr(i, cnt, start, end, step), i)


def test_draws_by_pixel(oracle_lib):
    """v2e_draw_init / _scidvs, _frame, _pnoise and _pair (plain and key-schedule) for pixels 0 .. 2^20, clip 5, a seed with a
    non-zero high word"""
    n = (1 << 20) + 1
    px = np.arange(n, dtype=np.uint32)
    key = [SEED & 0xFFFFFFFF, SEED >> 32, CLIP]
    host = np.stack(list(oracle_lib.draw_init(SEED, CLIP, 0, n)) + [oracle_lib.draw_scidvs(SEED, CLIP, 0, n)], axis=1)
    _same(dm_eval("DRAW_INIT", px, np.asarray(key, np.uint32), width=4), host, px)
    for frame in (1, 2, 7):
        leak, shot = dm_eval("DRAW_FRAME", px, np.asarray(key + [frame], np.uint32), two=True)
        h_leak, h_shot = oracle_lib.draw_frame(SEED, CLIP, frame, 0, n)
        _same(leak, h_leak, px)
        _same(shot, h_shot, px)
    for frame in (0, 3):
        _same(dm_eval("DRAW_PNOISE", px, np.asarray(key + [frame], np.uint32)), oracle_lib.draw_pnoise(SEED, CLIP, frame, 0, n), px)
    for fn, ks in (("DRAW_PAIR", False), ("DRAW_PAIR_KS", True)):
        for want_normal in (1, 0):
            got = dm_eval(fn, px, np.asarray(key + [2, want_normal], np.uint32), width=4)
            _same(got, oracle_lib.draw_pair(SEED, CLIP, 2, 0, n, want_normal=bool(want_normal), key_schedule=ks), px)


def test_first_frame_planes_in_situ_at_1280x720(oracle_lib):
    """The product kernels' own copies of the header: one first frame at 720 x 1280 in Philox mode under a seed with a non-zero high
    word.  pos_thres, neg_thres and noise_rate_array equal the oracle's bit for bit (pixel indices up to 921 599), and lie within the
    bounds of tests/test_detmath.py of an independent float64 computation: the independent Philox, float64 Box-Muller, numpy's exp."""
    from v2e_amd import EventEmulator
    H, W = 720, 1280
    kw = dict(seed=SEED, rng_mode="philox", cutoff_hz=300, leak_rate_hz=0.1, sigma_thres=0.03, refractory_period_s=0.0005)
    emu = EventEmulator(device="cuda", **kw)
    f = np.full((H, W), 100, np.uint8)
    emu.generate_events(f, 0.0)
    ora = oracle_lib.OracleEmulator(**kw)
    ora.generate_events(f, 0.0)
    pos, neg, rate = (t.cpu().numpy() for t in (emu.pos_thres, emu.neg_thres, emu.noise_rate_array))
    _same(_bits(pos).reshape(-1), ora.pos_thres_arr.reshape(-1))
    _same(_bits(neg).reshape(-1), ora.neg_thres_arr.reshape(-1))
    _same(_bits(rate).reshape(-1), ora.noise_rate_array.reshape(-1))
    px = np.arange(H * W, dtype=np.uint32)
    w = dc.stream_words(SEED, 0, dc.STREAM_THRES, 0, px)
    r = dc.stream_words(SEED, 0, dc.STREAM_RATE, 0, px)
    # threshold = max(n * (float)0.03 + (float)0.2, 0.01) in float32: the normal's error times sigma, and four float32 roundings (the
    # two constants, the product, the sum) of at most half a spacing of [0.25, 0.5) each
    tol = dc.NORMAL_ABS_BOUND * 0.03 + 4 * 2.0 ** -26
    for got, (wa, wb) in ((pos, (w[:, 0], w[:, 1])), (neg, (w[:, 2], w[:, 3]))):
        want = np.maximum(dc.box_muller_ref(wa, wb)[0] * 0.03 + 0.2, 0.01)
        assert got.max() < 0.5 and np.max(np.abs(got.reshape(-1) - want)) <= tol
    # rate = expf((float)(ln 10 * 0.1) * n): relative error EXPF_ULP_BOUND spacings (at most 2^-23 each) from the exponential, and the
    # argument's absolute error -- two roundings of relative 2^-24 on |argument| <= 0.2303 * 5.77 < 1.33, and the normal's 1e-6 * 0.2303
    n_rate = dc.box_muller_ref(r[:, 0], r[:, 1])[0]
    want = np.exp(np.log(10.0) * 0.1 * n_rate)
    rel = dc.EXPF_ULP_BOUND * 2.0 ** -23 + 2 * 2.0 ** -24 * 1.33 + dc.NORMAL_ABS_BOUND * 0.2303
    assert np.max(np.abs(rate.reshape(-1) - want) / want) <= rel * 1.0001   # (e^d - 1 for d <= 6e-7)
