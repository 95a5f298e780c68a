"""GPU: the SloMo kernels that run between the convolutions (v2e_amd/csrc/slomo_stream.h) and the byte / float conversions on
both sides of the network (resample.hip), one kernel at a time at the shapes where each takes another path.

Pooling and the bilinear x2 are float32 additions and multiplications in the same written order in the kernels and in the CPU
oracle, both built with -ffp-contract=off: they must agree bit for bit (a NaN -- 0 * inf at a clamped edge -- equals a NaN: the
payload is the processor's).  The reductions have exact answers from numpy.  Warp, blend and fusion are held to the reference's
own numbers at edge shapes (tests/golden/slomo_stream_edges.npz, whose census tests/test_slomo_stream.py checks on the CPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import slomo_stream_cases as sc
from fixtures import GOLDEN

pytestmark = pytest.mark.gpu

EINVAL = -22
GUARD = np.float32(-12345.678)
AVGPOOL2, AVGPOOL2_SCALAR, UPSAMPLE2, UPSAMPLE2_SCALAR, AMAX = range(5)


def _lib():
    from v2e_amd import _capi
    return _capi.lib()


def _check(rc, what):
    from v2e_amd._capi import check
    check(rc, what)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, guard):
    """a float32 device buffer of n + guard elements, all GUARD"""
    return torch.full((n + guard,), float(GUARD), dtype=torch.float32, device="cuda")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _first_difference(a, b):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b)))
    return "%d differ, first at %d: %r against %r" % (len(bad), bad[0], a[bad[0]], b[bad[0]]) if len(bad) else "equal"


def _stream_eval(op, x, shape):
    """v2e_slomo_stream_eval of x into [nc][h][w] with a guard plane of h * w behind it: the result (numpy)"""
    nc, h, w = shape
    n = nc * h * w
    y = _guarded(n, h * w)
    _check(_lib().v2e_slomo_stream_eval(op, _p(x), _p(y), nc, h, w, _stream()), "v2e_slomo_stream_eval")
    out = y.cpu().numpy()
    assert np.all(out[n:] == GUARD), "the guard plane behind the output was written"
    return out[:n].reshape(1, nc, h, w)


def _pool_checks(shape, x, oracle_lib):
    ref = oracle_lib.avgpool2(x)
    tx = _dev(x)
    got = _stream_eval(AVGPOOL2, tx, shape)
    assert _same_bits(got, ref), _first_difference(got, ref)
    if shape[2] % 4 == 0:   # the product took the four-outputs-per-thread kernel: the scalar twin gives its bits
        twin = _stream_eval(AVGPOOL2_SCALAR, tx, shape)
        assert _same_bits(twin, got), _first_difference(twin, got)
    return got


def _up_checks(shape, x, oracle_lib):
    ref = oracle_lib.upsample2(x)
    tx = _dev(x)
    got = _stream_eval(UPSAMPLE2, tx, shape)
    assert _same_bits(got, ref), _first_difference(got, ref)
    if shape[2] % 4 == 0:
        twin = _stream_eval(UPSAMPLE2_SCALAR, tx, shape)
        assert _same_bits(twin, got), _first_difference(twin, got)
    return got


@pytest.mark.parametrize("shape", sc.POOL_SHAPES, ids=str)
def test_avgpool2_equals_the_oracle_bit_for_bit(shape, oracle_lib):
    x = sc.pool_input(shape)
    got = _pool_checks(shape, x, oracle_lib)
    ref = torch.nn.functional.avg_pool2d(torch.from_numpy(x), 2).numpy()   # the operator the reference calls, on this machine
    assert sc.relerr(got, ref) <= sc.TOL


@pytest.mark.parametrize("shape", sc.UP_SHAPES, ids=str)
def test_upsample2_equals_the_oracle_bit_for_bit(shape, oracle_lib):
    x = sc.up_input(shape)
    got = _up_checks(shape, x, oracle_lib)
    ref = torch.nn.functional.interpolate(torch.from_numpy(x), scale_factor=2, mode="bilinear", align_corners=False).numpy()
    assert sc.relerr(got, ref) <= sc.TOL


@pytest.mark.parametrize("shape", [(5, 17, 12), (3, 2, 6)], ids=str)
def test_avgpool2_with_inf_negative_zero_and_the_largest_float_at_the_borders(shape, oracle_lib):
    x = sc.plant_specials(sc.pool_input(shape))
    got = _pool_checks(shape, x, oracle_lib)
    assert np.isinf(got).any() and got[0, 0, 0, 0] == np.inf


@pytest.mark.parametrize("shape", [(2, 6, 12), (5, 6, 10)], ids=str)
def test_upsample2_with_inf_negative_zero_and_the_largest_float_at_the_borders(shape, oracle_lib):
    x = sc.plant_specials(sc.up_input(shape))
    got = _up_checks(shape, x, oracle_lib)
    assert np.isinf(got).any() or np.isnan(got).any()


def test_stream_eval_refuses_bad_arguments():
    lib = _lib()
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    y = torch.zeros(64, dtype=torch.float32, device="cuda")
    s = _stream()
    bad = [(AVGPOOL2, None, _p(y), 1, 2, 2), (AVGPOOL2, _p(x), None, 1, 2, 2), (AVGPOOL2, _p(x), _p(y), 0, 2, 2),
           (AVGPOOL2_SCALAR, _p(x), _p(y), 1, 0, 2), (UPSAMPLE2_SCALAR, _p(x), _p(y), 1, 2, -2), (UPSAMPLE2, _p(x), _p(y), 1, 3, 4),
           (UPSAMPLE2_SCALAR, _p(x), _p(y), 1, 2, 3), (AMAX + 1, _p(x), _p(y), 1, 2, 2), (-1, _p(x), _p(y), 1, 2, 2)]
    for op, px, py, nc, h, w in bad:
        assert lib.v2e_slomo_stream_eval(op, px, py, nc, h, w, s) == EINVAL, (op, nc, h, w)
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0   # and nothing was launched


# ------------------------------------------------------------------ k_amax
def _amax(x, preload):
    """the slot (preloaded) after k_amax over device tensor x, and the guard word behind it"""
    slot = torch.tensor([preload, 0x1234], dtype=torch.int64).to(torch.int32).cuda()
    _check(_lib().v2e_slomo_stream_eval(AMAX, _p(x), _p(slot), x.numel(), 1, 1, _stream()), "v2e_slomo_stream_eval")
    got = slot.cpu().numpy().view(np.uint32)
    assert got[1] == 0x1234
    return int(got[0])


@pytest.mark.parametrize("n", sc.AMAX_SIZES)
def test_amax_finds_the_maximum_wherever_it_is(n):
    rng = np.random.Generator(np.random.PCG64(700 + n % 1000))
    base = sc.rand15(rng, (n,), 1.0)
    dev = {"random": _dev(base), "zero": torch.zeros(n, dtype=torch.float32, device="cuda")}
    values = [("random", np.float32(-3.5)), ("zero", np.float32(2.0 ** -126)), ("random", np.float32(np.inf))]
    for pos in sc.amax_positions(n):
        for kind, v in values:
            t = dev[kind]
            keep = t[pos].clone()
            t[pos] = float(v)
            host = base.copy() if kind == "random" else np.zeros(n, np.float32)
            host[pos] = v
            want = int(np.max(np.abs(host)).view(np.uint32))
            assert want == int(np.abs(v).view(np.uint32))   # the planted value is the unique maximum
            got = _amax(t, 0)
            t[pos] = keep
            assert got == want, (n, pos, float(v), hex(got), hex(want))
    assert np.float32(np.inf).view(np.uint32) == 0x7F800000


def test_amax_only_raises_the_slot():
    rng = np.random.Generator(np.random.PCG64(71))
    x = sc.rand15(rng, (1025,), 3.0)
    want = int(np.max(np.abs(x)).view(np.uint32))
    t = _dev(x)
    above, below = int(np.float32(100.0).view(np.uint32)), int(np.float32(0.001).view(np.uint32))
    assert below < want < above
    assert _amax(t, above) == above         # a larger slot stays
    assert _amax(t, below) == want          # a smaller one is raised
    assert _amax(t, want) == want
    zeros = torch.zeros(1025, dtype=torch.float32, device="cuda")
    zeros[7] = -0.0
    assert _amax(zeros, below) == below and _amax(zeros, 0) == 0   # an all-zero input leaves the slot as it was


@pytest.mark.parametrize("n,pos", [(5, 1), (5, 4), (1025, 1023), (1025, 1024), (262145, 131072), (4197378, 4197377), (4197378, 4194304)])
def test_amax_records_a_nan_of_the_network_input(n, pos):
    """include/v2e_amd.h (v2e_conv_set_range_flag): the network input is watched for inf AND NaN -- an input that holds a NaN and
    no inf must leave a slot with the all-ones exponent act_scale tests, in the vector loop and in the scalar tail"""
    rng = np.random.Generator(np.random.PCG64(72 + n % 1000))
    x = sc.rand15(rng, (n,), 2.0)
    x[pos] = np.nan
    assert not np.isinf(x).any()
    got = _amax(_dev(x), 0)
    assert got >> 23 == 255, hex(got)
    x[(pos + 1) % n] = -np.inf   # and an inf beside it changes nothing about that
    assert _amax(_dev(x), 0) >> 23 == 255


def test_nan_only_network_input_takes_the_exact_split_and_the_guard_does_not_stick():
    """the pattern of test_operand_scaling_and_range_guard_of_the_two_piece_math (tests/test_slomo_gpu.py) with a NaN and no inf
    in the input: conv math 'auto' counts one fallback and returns bf16x3's result"""
    from v2e_amd.slomo import HipUNet
    from v2e_amd.synth import portable_unet_state_dict
    sd = {k: torch.from_numpy(v) for k, v in portable_unet_state_dict(12, 5, 102).items()}
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(9)
    x = (torch.rand((2, 12, 64, 96), generator=g) - 0.4).to(dev)
    auto, exact = (HipUNet(sd, 12, 5, dev, m) for m in ("auto", "bf16x3"))
    y = auto.forward(x)
    assert auto.fallbacks == 0
    xb = x.clone()
    xb[1, 7, 33, 95] = float("nan")
    assert not torch.isinf(xb).any()
    yb = auto.forward(xb)
    assert auto.fallbacks == 1
    assert torch.isnan(yb).any()
    assert torch.equal(torch.nan_to_num(yb, nan=7.0), torch.nan_to_num(exact.forward(xb), nan=7.0))
    y2 = auto.forward(x)                # and the guard does not stick
    assert auto.fallbacks == 1 and torch.equal(y2, y)


# ------------------------------------------------------------------ k_max_speed2, k_max_speed2_seg
def _speed(flow):
    b, _, h, w = flow.shape
    out = torch.tensor([0x5555, 0x1234], dtype=torch.int32).cuda()
    _check(_lib().v2e_slomo_max_speed2(_p(flow), b, h, w, _p(out), _stream()), "v2e_slomo_max_speed2")
    got = out.cpu().numpy().view(np.uint32)
    assert got[1] == 0x1234
    return int(got[0])


def _speed_seg(flow, seg):
    b, _, h, w = flow.shape
    nseg = (b + seg - 1) // seg
    out = torch.full((nseg + 1,), 0x1234, dtype=torch.int32).cuda()
    _check(_lib().v2e_slomo_max_speed2_seg(_p(flow), b, seg, h, w, _p(out), _stream()), "v2e_slomo_max_speed2_seg")
    got = out.cpu().numpy().view(np.uint32)
    assert got[nseg] == 0x1234, "the slot behind the last batch was written"
    return [int(v) for v in got[:nseg]]


def _speed_checks(flow_host, flow_dev, what):
    b = flow_host.shape[0]
    want = sc.speed2_ref(flow_host)
    got = _speed(flow_dev)
    assert got == want, (what, hex(got), hex(want))
    for seg in sorted({1, 2, b}):
        per = [sc.speed2_ref(flow_host[j:j + seg]) for j in range(0, b, seg)]
        assert _speed_seg(flow_dev, seg) == per, (what, seg)
    return want


@pytest.mark.parametrize("shape", sc.SPEED_SHAPES, ids=str)
def test_max_speed2_equals_numpy_in_float32(shape):
    b, h, w = shape
    rng = np.random.Generator(np.random.PCG64(800 + b + h + w))
    base = sc.rand15(rng, (b, 4, h, w), 5.0)
    dev = _dev(base)                             # |component| < 5: every planted value below is the unique maximum
    _speed_checks(base, dev, "random")
    plants = [("the first vector", (0, 0, 0, 0), 100.25), ("the last vector of the last pair", (b - 1, 1, h - 1, w - 1), 99.75),
              ("the F10 pair only", (b // 2, 2, h // 2, w // 2), 101.5), ("a negative component", (b - 1, 3, h - 1, 0), -102.125)]
    for what, idx, v in plants:
        host = base.copy()
        host[idx] = v
        keep = dev[idx].clone()
        dev[idx] = v
        want = _speed_checks(host, dev, what)
        dev[idx] = keep
        lo = np.float32(v) * np.float32(v)
        assert np.uint32(want).view(np.float32) >= lo   # the planted component carries the maximum
    for what, v, want in (("a component of 1e20", 1e20, 0x7F800000), ("a NaN", float("nan"), 0xFFFFFFFF)):
        host = base.copy()
        idx = (b - 1, 2, h - 1, w // 2)
        host[idx] = v
        keep = dev[idx].clone()
        dev[idx] = v
        assert _speed_checks(host, dev, what) == want
        dev[idx] = keep
    zero = np.zeros_like(base)
    zero[0, 1, 0, 0] = -0.0
    assert _speed_checks(zero, _dev(zero), "all zero") == 0


# ------------------------------------------------------------------ k_prep, k_fuse and their _tab twins on the reference's fixture
@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(GOLDEN, sc.EDGE_FIXTURE))


def _prep(d, case, lib):
    from v2e_amd.planning import time_coefficients
    h, w, b, n_t = case
    t = dict(I0=_dev(d["I0"]), I1=_dev(d["I1"]), flow=_dev(d["flow"]), coef=_dev(time_coefficients(d["ts"])))
    n = n_t * b * 12 * h * w
    x12 = _guarded(n, 1)
    _check(lib.v2e_slomo_prep(_p(t["I0"]), _p(t["I1"]), _p(t["flow"]), _p(t["coef"]), n_t, b, h, w, _p(x12), _stream()), "v2e_slomo_prep")
    t["x12"] = x12
    return t, n


def _fuse(d, case, t, lib):
    h, w, b, n_t = case
    t["intrp"] = _dev(d["intrp"].reshape(n_t * b, 5, h, w))
    n = n_t * b * h * w
    out = _guarded(n, 1)
    _check(lib.v2e_slomo_fuse(_p(t["I0"]), _p(t["I1"]), _p(t["x12"]), _p(t["intrp"]), _p(t["coef"]), n_t, b, h, w, _p(out), _stream()),
           "v2e_slomo_fuse")
    return out, n


@pytest.mark.parametrize("case", sc.EDGE_CASES, ids=sc.case_name)
def test_prep_and_fuse_equal_the_reference_at_edge_shapes(edges, case):
    from v2e_amd.planning import time_coefficients
    lib = _lib()
    d = sc.load_case(edges, case)
    h, w, b, n_t = case
    t, n = _prep(d, case, lib)
    raw = t["x12"].cpu().numpy()
    assert raw[n] == GUARD, "the sample behind x12 was written"
    x12 = raw[:n].reshape(n_t, b, 12, h, w)
    e_prep = sc.relerr(x12[:, :, 6:12], d["x12_tail"])
    for ti in range(n_t):   # channels 0-5: bit copies of their sources for sample s = ti * b + bi
        assert _same_bits(x12[ti, :, 0], d["I0"][:, 0]) and _same_bits(x12[ti, :, 1], d["I1"][:, 0])
        assert _same_bits(x12[ti, :, 2:6], d["flow"])
    c = time_coefficients(d["ts"])
    F01, F10 = d["flow"][:, 0:2], d["flow"][:, 2:4]
    for ti in range(n_t):   # channels 6-9: the float32 blend, two rounded products and their rounded sum
        ft0 = (c[ti, 0] * F01) + (c[ti, 1] * F10)
        ft1 = (c[ti, 2] * F01) + (c[ti, 3] * F10)
        assert ft0.dtype == np.float32
        assert _same_bits(x12[ti, :, 6:8], ft1), _first_difference(x12[ti, :, 6:8], ft1)
        assert _same_bits(x12[ti, :, 8:10], ft0), _first_difference(x12[ti, :, 8:10], ft0)
    out, m = _fuse(d, case, t, lib)
    raw = out.cpu().numpy()
    assert raw[m] == GUARD, "the sample behind Ft was written"
    e_fuse = sc.relerr(raw[:m].reshape(n_t, b, 1, h, w), d["Ft"])
    print("%s: prep %.2e fuse %.2e" % (sc.case_name(case), e_prep, e_fuse))
    assert e_prep <= sc.TOL and e_fuse <= sc.TOL


@pytest.mark.parametrize("case", sc.EDGE_CASES, ids=sc.case_name)
def test_table_driven_prep_and_fuse_equal_the_reference_and_the_batch_kernels(edges, case):
    """a table whose rows are shuffled and repeat some (pair, time row) combinations: every sample is the fixture's for that pair
    and row within TOL, and k_prep's / k_fuse's own bit for bit"""
    lib = _lib()
    d = sc.load_case(edges, case)
    h, w, b, n_t = case
    hw = h * w
    t, n = _prep(d, case, lib)
    x12 = t["x12"].cpu().numpy()[:n].reshape(n_t, b, 12, h, w)
    out, m = _fuse(d, case, t, lib)
    Ft = out.cpu().numpy()[:m].reshape(n_t, b, 1, h, w)
    rng = np.random.Generator(np.random.PCG64(900 + hw))
    rows = [(bi, ti) for ti in range(n_t) for bi in range(b)]
    rows = rows + rows[:3] + [rows[-1]]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    if rows == sorted(rows):   # (five rows of two kinds can come out in order)
        rows.reverse()
    assert len(set(rows)) < len(rows) and rows != sorted(rows)
    ns = len(rows)
    tab = _dev(np.asarray([[bi, ti, s] for s, (bi, ti) in enumerate(rows)], np.int32))
    x12t = _guarded(ns * 12 * hw, 1)
    _check(lib.v2e_slomo_prep_tab(_p(t["I0"]), _p(t["I1"]), _p(t["flow"]), _p(t["coef"]), _p(tab), ns, h, w, _p(x12t), _stream()),
           "v2e_slomo_prep_tab")
    intrp_t = _dev(np.stack([d["intrp"][ti, bi] for bi, ti in rows]))
    outt = _guarded(ns * hw, 1)
    _check(lib.v2e_slomo_fuse_tab(_p(t["I0"]), _p(t["I1"]), _p(x12t), _p(intrp_t), _p(t["coef"]), _p(tab), ns, h, w, _p(outt), _stream()),
           "v2e_slomo_fuse_tab")
    rx, ro = x12t.cpu().numpy(), outt.cpu().numpy()
    assert rx[ns * 12 * hw] == GUARD and ro[ns * hw] == GUARD
    rx, ro = rx[:-1].reshape(ns, 12, h, w), ro[:-1].reshape(ns, 1, h, w)
    for s, (bi, ti) in enumerate(rows):
        assert sc.relerr(rx[s, 6:12], d["x12_tail"][ti, bi]) <= sc.TOL, s
        assert sc.relerr(ro[s], d["Ft"][ti, bi]) <= sc.TOL, s
        assert _same_bits(rx[s], x12[ti, bi]), (s, _first_difference(rx[s], x12[ti, bi]))
        assert _same_bits(ro[s], Ft[ti, bi]), (s, _first_difference(ro[s], Ft[ti, bi]))


def test_prep_and_fuse_refuse_more_samples_than_a_grid_holds():
    """n_t * b = 65 536 is one more than gridDim.y takes: V2E_EINVAL before any launch (65 535 runs)"""
    lib = _lib()
    b = 65535
    i0 = torch.full((b + 1, 1, 1, 1), 0.25, dtype=torch.float32, device="cuda")
    flow = torch.zeros((b + 1, 4, 1, 1), dtype=torch.float32, device="cuda")
    coef = _dev(sc.time_coefficients([0.5, 0.25]))
    x12 = _guarded((b + 1) * 12, 1)
    intrp = torch.zeros((b + 1, 5, 1, 1), dtype=torch.float32, device="cuda")
    out = _guarded(b + 1, 1)
    s = _stream()
    for n_t, bb in ((1, 65536), (65536, 1), (256, 256)):
        assert lib.v2e_slomo_prep(_p(i0), _p(i0), _p(flow), _p(coef), n_t, bb, 1, 1, _p(x12), s) == EINVAL
        assert b"too many samples" in lib.v2e_last_error()
        assert lib.v2e_slomo_fuse(_p(i0), _p(i0), _p(x12), _p(intrp), _p(coef), n_t, bb, 1, 1, _p(out), s) == EINVAL
        assert b"too many samples" in lib.v2e_last_error()
    for h, w in ((0, 1), (1, 0), (-1, 1)):
        assert lib.v2e_slomo_prep(_p(i0), _p(i0), _p(flow), _p(coef), 1, 1, h, w, _p(x12), s) == EINVAL
        assert lib.v2e_slomo_fuse(_p(i0), _p(i0), _p(x12), _p(intrp), _p(coef), 1, 1, h, w, _p(out), s) == EINVAL
    torch.cuda.synchronize()
    assert bool((x12 == float(GUARD)).all()) and bool((out == float(GUARD)).all())   # nothing was launched
    _check(lib.v2e_slomo_prep(_p(i0), _p(i0), _p(flow), _p(coef), 1, b, 1, 1, _p(x12), s), "v2e_slomo_prep")
    _check(lib.v2e_slomo_fuse(_p(i0), _p(i0), _p(x12), _p(intrp), _p(coef), 1, b, 1, 1, _p(out), s), "v2e_slomo_fuse")
    rx, ro = x12.cpu().numpy(), out.cpu().numpy()
    assert np.all(rx[:b * 12].reshape(b, 12)[:, 0] == np.float32(0.25)) and np.all(rx[b * 12:] == GUARD)
    assert np.all(ro[b:] == GUARD) and not np.any(ro[:b] == GUARD)


# ------------------------------------------------------------------ the conversions on both sides of the network
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_u8_to_f32_norm_equals_torch_cpu_for_every_byte(n):
    lib = _lib()
    seen = set()
    for start in range(0, 256, min(n, 256)):
        x = ((np.arange(n, dtype=np.int64) + start) % 256).astype(np.uint8)
        seen.update(int(v) for v in x[:256])
        want = (torch.from_numpy(x).float().div(255) - 0.428).numpy()
        out = _guarded(n, 1)
        _check(lib.v2e_u8_to_f32_norm(_p(_dev(x)), _p(out), n, 0.428, _stream()), "v2e_u8_to_f32_norm")
        got = out.cpu().numpy()
        assert got[n] == GUARD
        assert _same_bits(got[:n], want), (n, start, _first_difference(got[:n], want))
    assert len(seen) == 256


def _trunc_input(U, B, hw):
    """the value mix of test_quantisation_equals_torch_cpu_byte_conversion_out_of_range (tests/test_resample.py)"""
    rng = np.random.Generator(np.random.PCG64(77 + hw))
    x = (rng.integers(0, 1 << 16, size=(U, B, hw)).astype(np.float32) / np.float32(65536.0) * np.float32(2.6) - np.float32(1.2))
    x.flat[:6] = [-0.428, 1.0 - 0.428, 0.0, 1.0, -0.4280001, 255.9999 / 255 - 0.428]
    assert (x + 0.428 < 0).any() and (x + 0.428 > 1).any()
    return x


@pytest.mark.parametrize("U,B,hw", [(3, 2, 35), (2, 3, 261)])
def test_f32_to_u8_trunc_equals_torch_cpu_plain_and_reordered(U, B, hw):
    lib = _lib()
    x = _trunc_input(U, B, hw)
    want = (torch.from_numpy(x) + 0.428).mul(255).byte().numpy()
    tx = _dev(x)
    n = U * B * hw
    for reorder in (0, 1):
        q = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        _check(lib.v2e_f32_to_u8_trunc(_p(tx), _p(q), U, B, hw, 0.428, reorder, _stream()), "v2e_f32_to_u8_trunc")
        got = q.cpu().numpy()
        assert got[n] == 0xA5
        exp = want.transpose(1, 0, 2) if reorder else want   # [B][U][hw]: time order
        assert np.array_equal(got[:n].reshape(exp.shape), exp), reorder


@pytest.mark.parametrize("U,B,hw", [(3, 2, 35), (2, 3, 261)])
def test_f32_to_u8_trunc_tab_fills_the_named_frames_only(U, B, hw):
    lib = _lib()
    n = U * B
    x = _trunc_input(U, B, hw).reshape(n, hw)
    want = (torch.from_numpy(x) + 0.428).mul(255).byte().numpy()
    rng = np.random.Generator(np.random.PCG64(78 + hw))
    nframes = n + 3
    frames = rng.permutation(nframes)[:n]          # non-monotonic frame slots; three frames no row names
    assert not np.all(np.diff(frames) > 0)
    tab = _dev(np.stack([np.zeros(n, np.int64), np.zeros(n, np.int64), frames], axis=1).astype(np.int32))
    q = torch.full((nframes * hw + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    _check(lib.v2e_f32_to_u8_trunc_tab(_p(_dev(x)), _p(q), _p(tab), n, hw, 0.428, _stream()), "v2e_f32_to_u8_trunc_tab")
    got = q.cpu().numpy()
    assert got[nframes * hw] == 0xA5
    got = got[:-1].reshape(nframes, hw)
    for s, f in enumerate(frames):
        assert np.array_equal(got[f], want[s]), (s, f)
    for f in set(range(nframes)) - set(int(v) for v in frames):
        assert np.all(got[f] == 0xA5), f
