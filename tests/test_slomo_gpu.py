"""GPU parity tests of the SuperSloMo HIP path (f32 MFMA convolutions with fused
pool / upsample / concat loaders, backWarp, blend, fusion), through the C ABI, against golden
vectors from the reference's own modules and against the CPU oracle.
Tolerance (BASELINE north_star: float intermediates within 1e-5): |a-b| <= 1e-5*max(1,|b|)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from fixtures import GOLDEN

pytestmark = pytest.mark.gpu
TOL = 1e-5


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _rand(rng, shape, scale=1.0):
    return ((rng.integers(0, 1 << 16, size=shape).astype(np.float32) / 32768.0) - 1.0) * np.float32(scale)


def _conv_hip(x0, x1, pre, w, b, out_hw, split=False):
    """split: also hand the layer its split-bf16 weights, which makes v2e_conv2d_lrelu take the bf16-matrix-core kernel."""
    from v2e_amd import _capi
    from v2e_amd._capi import ConvDesc, check
    lib = _capi.lib()
    dev = torch.device("cuda")
    tw = torch.from_numpy(w).to(dev)
    co, ci, k, _ = w.shape
    wp = torch.empty((ci, k, k, co), dtype=torch.float32, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.v2e_pack_conv_weight(C.c_void_p(tw.data_ptr()), C.c_void_p(wp.data_ptr()), co, ci, k, s), "pack")
    tb = torch.from_numpy(b).to(dev)
    d = ConvDesc(wp.data_ptr(), tb.data_ptr(), ci, co, k)
    if split:
        w3 = torch.empty((ci + 15) // 16 * 16 * k * k * co * 6, dtype=torch.uint8, device=dev)
        check(lib.v2e_pack_conv_weight_s3(C.c_void_p(tw.data_ptr()), C.c_void_p(w3.data_ptr()), co, ci, k, s), "pack_s3")
        d.weight_s3 = w3.data_ptr()
    t0 = torch.from_numpy(x0).to(dev)
    t1 = torch.from_numpy(x1).to(dev) if x1 is not None else None
    n = x0.shape[0]
    h, wd = out_hw
    y = torch.full((n, co, h, wd), float("nan"), dtype=torch.float32, device=dev)
    check(lib.v2e_conv2d_lrelu(C.c_void_p(t0.data_ptr()), x0.shape[1], C.c_void_p(t1.data_ptr()) if t1 is not None else None,
                               0 if x1 is None else x1.shape[1], pre, C.byref(d), C.c_void_p(y.data_ptr()), n, h, wd, s), "conv")
    torch.cuda.synchronize()
    return y.cpu().numpy()


CONV_CASES = [
    # (k, cin0, cin1, cout, n, h, w, pre)
    (7, 2, 0, 32, 2, 32, 64, 0),      # flow UNet conv1 (cin=2 -> CI_T=2 variant)
    (7, 12, 0, 32, 1, 40, 72, 0),     # interp UNet conv1, ragged tile edges
    (7, 32, 0, 32, 1, 16, 32, 0),
    (5, 32, 0, 64, 2, 24, 40, 1),     # down1.conv1: fused avg_pool2d
    (5, 64, 0, 64, 1, 24, 40, 0),
    (3, 64, 0, 128, 2, 16, 48, 1),    # TW=16 path
    (3, 128, 0, 128, 3, 8, 40, 0),    # TW=8 path
    (3, 512, 0, 512, 2, 2, 3, 1),     # bottleneck, tiny image
    (3, 512, 0, 512, 2, 4, 6, 2),     # up1.conv1: fused bilinear x2
    (3, 256, 256, 256, 1, 8, 12, 0),  # up.conv2: fused concat
    (3, 32, 32, 32, 1, 32, 64, 0),    # up5.conv2
    (3, 64, 0, 32, 1, 32, 64, 2),     # up5.conv1
    (3, 32, 0, 5, 2, 32, 64, 0),      # conv3 (cout not a multiple of 32)
    (3, 128, 0, 128, 24, 32, 32, 0),  # many images
    (3, 8, 0, 128, 2048, 16, 16, 0),  # >= 16 workgroups per CU: wide (64-channel) tiles selected
    (3, 64, 0, 64, 3, 16, 20, 0),     # 16x20 level of a 320x256 input: 8x20 five-wave tiles
    (3, 64, 0, 64, 2, 8, 20, 0),
    (3, 64, 0, 64, 3, 8, 10, 0),      # 8x10 level: two samples stacked per tile, odd sample count
    (3, 32, 32, 96, 4, 8, 10, 0),     # ... with the fused concat
    # wide (64-channel, CT=2) tiles: conv_dispatch (slomo.hip) selects them once px_tiles * cout/64 >= 4096, which the
    # 80/100-sample batches of the bench line reach at the 160x128 level (down1, up4) -- same instantiations here
    (5, 64, 0, 64, 52, 128, 160, 0),  # k_conv<5,4,2,2,4,32,0>: down1.conv2 as the 80-sample batch runs it (52*80 tiles)
    (5, 8, 0, 64, 52, 128, 160, 1),   # k_conv<5,4,2,2,4,32,1>: fused avg_pool2d loader
    (5, 4, 0, 128, 300, 20, 96, 0),   # ... ragged tile rows, two channel blocks
    (3, 128, 0, 64, 52, 128, 160, 0), # launch_conv_tw<3,8,2,0> at TW=32: up4.conv1
    (3, 8, 8, 64, 52, 128, 160, 0),   # ... with the fused concat (up4.conv2)
    (3, 16, 0, 64, 52, 128, 160, 1),  # launch_conv_tw<3,8,2,1> at TW=32
    (3, 16, 0, 64, 52, 128, 160, 2),  # launch_conv_tw<3,8,2,2> at TW=32
    (3, 8, 0, 128, 300, 20, 96, 2),   # ... ragged tile rows
    (3, 16, 0, 128, 104, 64, 80, 0),  # wide at an 80-wide level (TW=16)
]


# the split-bf16 kernel (slomo_s3.h: plain loads, cin % 16 == 0, cout % 32 == 0): every tile shape conv_dispatch_s3
# selects, ragged edges, the fused concat, several weight groups per chunk (5x5, 7x7), several chunks
S3_CASES = [
    (3, 16, 0, 32, 3, 40, 72, 0),     # TW=8 (32x8 tiles), masked rows
    (3, 32, 0, 64, 2, 24, 32, 0),     # TW=32, masked rows
    (3, 64, 0, 32, 2, 64, 96, 0),     # up5.conv1 shape class
    (3, 32, 32, 32, 1, 32, 64, 0),    # up5.conv2: concat, one chunk per source... two chunks each
    (3, 16, 16, 64, 2, 16, 48, 0),    # TW=16, concat at a chunk boundary
    (3, 256, 256, 256, 1, 8, 40, 0),  # up.conv2 at a 40-wide level
    (3, 512, 0, 512, 3, 16, 20, 0),   # 16x20 level: 8x20 five-wave tiles
    (3, 64, 0, 64, 2, 8, 20, 0),
    (3, 128, 0, 128, 24, 32, 32, 0),  # many images
    (5, 32, 0, 64, 2, 24, 64, 0),     # down1.conv1
    (5, 64, 0, 64, 1, 40, 96, 0),     # down1.conv2, ragged rows
    (7, 32, 0, 32, 2, 24, 64, 0),     # conv2
    (7, 32, 0, 32, 1, 256, 320, 0),   # conv2 at the benchmark resolution
    (7, 12, 0, 32, 2, 24, 64, 0),     # interp UNet conv1: 12 channels, the 16-channel chunk padded with zeros
    (7, 8, 0, 32, 1, 40, 96, 0),      # ... a whole empty channel group, ragged rows
    (7, 24, 0, 64, 1, 32, 32, 0),     # ... second chunk partial, two channel blocks
    (3, 64, 0, 64, 3, 8, 10, 0),      # 8x10 level: the 16x10 five-wave tile <3,1,1,5,10>, its lower half masked
]


@pytest.mark.parametrize("case", S3_CASES)
def test_split_bf16_conv_layer_matches_oracle(case, oracle_lib):
    k, c0, c1, cout, n, h, w, pre = case
    rng = np.random.Generator(np.random.PCG64(77 + k * 1000 + c0 + cout + h))
    x0 = _rand(rng, (n, c0, h, w))
    x1 = _rand(rng, (n, c1, h, w)) if c1 else None
    cin = c0 + c1
    wt = _rand(rng, (cout, cin, k, k), 1.5 / np.sqrt(cin * k * k))
    b = _rand(rng, (cout,), 0.1)
    y = _conv_hip(x0, x1, 0, wt, b, (h, w), split=True)
    y32 = _conv_hip(x0, x1, 0, wt, b, (h, w), split=False)
    xin = x0 if x1 is None else np.concatenate((x0, x1), axis=1)
    ref = oracle_lib.conv2d_lrelu(xin, wt, b)
    assert not np.isnan(y).any(), "output not fully written"
    assert relerr(y, ref) < TOL
    assert relerr(y, y32) < TOL
    assert not np.array_equal(y, y32)  # and it is not the same kernel twice: every shape here has a three-piece tile


@pytest.mark.parametrize("shape", [(64, 32, 2, 24, 64), (32, 64, 3, 32, 48), (16, 32, 2, 40, 72)])
def test_presplit_input_gives_the_same_bits(shape):
    """pre = 3: the input handed over already split (v2e_split3_nchw: [piece][n][C/8][h][w][8 bf16]) -- the layout a
    producer could write directly.  Same pieces, same products, same order: bit-identical to splitting while staging.
    (Measured 2-6 % faster only: the conversion is not what bounds the kernel)"""
    from v2e_amd import _capi
    from v2e_amd._capi import ConvDesc, check
    cin, cout, n, h, w = shape
    rng = np.random.Generator(np.random.PCG64(cin + cout + h))
    x = _rand(rng, (n, cin, h, w))
    wt = _rand(rng, (cout, cin, 3, 3), 1.5 / np.sqrt(cin * 9))
    b = _rand(rng, (cout,), 0.1)
    y_ref = _conv_hip(x, None, 0, wt, b, (h, w), split=True)
    lib = _capi.lib()
    dev = torch.device("cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tw, tb, tx = torch.from_numpy(wt).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(x).to(dev)
    wp = torch.empty((cin, 3, 3, cout), dtype=torch.float32, device=dev)
    w3 = torch.empty(cin * 9 * cout * 6, dtype=torch.uint8, device=dev)
    xs = torch.empty(x.size * 6, dtype=torch.uint8, device=dev)
    check(lib.v2e_pack_conv_weight(C.c_void_p(tw.data_ptr()), C.c_void_p(wp.data_ptr()), cout, cin, 3, s), "pack")
    check(lib.v2e_pack_conv_weight_s3(C.c_void_p(tw.data_ptr()), C.c_void_p(w3.data_ptr()), cout, cin, 3, s), "pack_s3")
    check(lib.v2e_split3_nchw(C.c_void_p(tx.data_ptr()), C.c_void_p(xs.data_ptr()), n, cin, h, w, s), "split3")
    d = ConvDesc(wp.data_ptr(), tb.data_ptr(), cin, cout, 3)
    d.weight_s3 = w3.data_ptr()
    y = torch.full((n, cout, h, w), float("nan"), dtype=torch.float32, device=dev)
    check(lib.v2e_conv2d_lrelu(C.c_void_p(xs.data_ptr()), cin, None, 0, 3, C.byref(d), C.c_void_p(y.data_ptr()), n, h, w, s), "conv")
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), y_ref)


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_layer_matches_oracle(case, oracle_lib):
    k, c0, c1, cout, n, h, w, pre = case
    rng = np.random.Generator(np.random.PCG64(k * 1000 + c0 + cout + h))
    sh, sw = (2 * h, 2 * w) if pre == 1 else ((h // 2, w // 2) if pre == 2 else (h, w))
    x0 = _rand(rng, (n, c0, sh, sw))
    x1 = _rand(rng, (n, c1, h, w)) if c1 else None
    cin = c0 + c1
    wt = _rand(rng, (cout, cin, k, k), 1.5 / np.sqrt(cin * k * k))
    b = _rand(rng, (cout,), 0.1)
    y = _conv_hip(x0, x1, pre, wt, b, (h, w))
    xin = x0
    if pre == 1:
        xin = oracle_lib.avgpool2(x0)
    elif pre == 2:
        xin = oracle_lib.upsample2(x0)
    if x1 is not None:
        xin = np.concatenate((xin, x1), axis=1)
    ref = oracle_lib.conv2d_lrelu(xin, wt, b)
    assert not np.isnan(y).any(), "output not fully written"
    assert relerr(y, ref) < TOL


# the default (three bf16 pieces on the bf16 matrix cores), the f32 matrix-core kernels, and the opt-in two-float16-piece mode
CONV_MATHS = ("auto", "bf16x3", "f32", "fp16x2")


def _engine(seed_f=101, seed_i=102, conv_math=None):
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import portable_unet_state_dict
    sd_f, sd_i = portable_unet_state_dict(2, 4, seed_f), portable_unet_state_dict(12, 5, seed_i)
    eng = SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()},
                      {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda", conv_math=conv_math)
    return eng, sd_f, sd_i


def _pairs(z):
    fr = z["frames"]
    n = len(fr) - 1
    I0 = (fr[:n].astype(np.float32) / np.float32(255.0))[:, None] - np.float32(0.428)
    I1 = (fr[1:n + 1].astype(np.float32) / np.float32(255.0))[:, None] - np.float32(0.428)
    return I0, I1


@pytest.mark.parametrize("conv_math", CONV_MATHS)
def test_interpolation_matches_reference_golden(conv_math):
    z = np.load(os.path.join(GOLDEN, "slomo_unet_64x96.npz"))
    I0, I1 = _pairs(z)
    ts = list(z["ts"])
    eng, _, _ = _engine(conv_math=conv_math)
    assert eng.conv_math == conv_math and eng.interp_net.conv_math == conv_math
    Ft = eng.interpolate(torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda(), ts)
    nt, b = len(ts), I0.shape[0]
    assert relerr(eng.last["flow"].cpu().numpy(), z["flow"]) < TOL
    assert relerr(eng.last["intrp"].cpu().numpy().reshape(nt, b, 5, 64, 96), z["intrp"]) < TOL
    assert relerr(Ft.cpu().numpy(), z["Ft"]) < TOL


@pytest.mark.parametrize("conv_math", CONV_MATHS)
def test_interpolation_matches_reference_at_benchmark_shape(conv_math):
    """BASELINE configs[2] SloMo stage as bench.py runs it: 320x256 (346x260 source), U=10, batch of 8 pairs ->
    80 samples through the interpolation UNet (the wide k_conv<5,4,2,...> / <3,8,2,...,32> tiles are dispatched at
    the 160x128 level).  The fixture holds the reference's result for 2 pairs; they are tiled 4x, and every copy
    must match (flow, Ft in full; the interpolation UNet's raw output on the fixture's stride-8 lattice)."""
    from test_slomo_oracle_golden import bench_shape_inputs
    z = np.load(os.path.join(GOLDEN, "slomo_320x256.npz"))
    I0, I1 = bench_shape_inputs(z)
    ts = list(z["ts"])
    sf, si = (int(v) for v in z["seeds"])
    eng, _, _ = _engine(sf, si, conv_math)
    rep = 4
    tI0 = torch.from_numpy(np.tile(I0, (rep, 1, 1, 1))).cuda()
    tI1 = torch.from_numpy(np.tile(I1, (rep, 1, 1, 1))).cuda()
    Ft = eng.interpolate(tI0, tI1, ts).cpu().numpy()          # [10, 8, 1, 256, 320]
    nt, b = len(ts), I0.shape[0]
    assert Ft.shape == (nt, rep * b, 1, 256, 320)
    flow = eng.last["flow"].cpu().numpy()
    intrp = eng.last["intrp"].cpu().numpy().reshape(nt, rep * b, 5, 256, 320)
    for r in range(rep):
        sl = slice(r * b, (r + 1) * b)
        assert relerr(flow[sl], z["flow"]) < TOL
        assert relerr(intrp[:, sl, :, ::8, ::8], z["intrp_lattice"]) < TOL
        assert relerr(Ft[:, sl], z["Ft"]) < TOL
    # copies are the same arithmetic on the same data: bit-identical regardless of the sample's tile position
    assert np.array_equal(Ft[:, :b], Ft[:, b:2 * b]) and np.array_equal(intrp[:, :b], intrp[:, 3 * b:])


@pytest.mark.parametrize("conv_math", CONV_MATHS)
def test_interpolation_matches_reference_at_hd_shape(conv_math):
    """SURVEY 8(a) / BASELINE configs[3] size: 1280x720 source -> 1280x704 (tests/golden/make_golden_slomo_1280x704.py: the
    reference's model.UNet / backWarp, B = 1, U = 2).  Levels 1280x704 ... 40x22: none of the widths the 320x256 tile dispatch
    was tuned for, and the 40x22 level is ragged against every tile height.  `flow` and `Ft` in full, the interpolation
    UNet's raw output on two stride-16 lattices, every conv math."""
    from PIL import Image
    from v2e_amd.synth import int_gradient_frames
    z = np.load(os.path.join(GOLDEN, "slomo_1280x704.npz"))
    n, sh, sw, seed, noise = (int(v) for v in z["frame_args"])
    fr = int_gradient_frames(n, sh, sw, seed=seed, noise=noise, as_array=True)
    rs = np.stack([np.asarray(Image.fromarray(f).resize((1280, 704), Image.LANCZOS)) for f in fr])
    t = (rs.astype(np.float32) / np.float32(255.0))[:, None] - np.float32(0.428)
    I0, I1 = np.ascontiguousarray(t[:-1]), np.ascontiguousarray(t[1:])
    ts = list(z["ts"])
    sf, si = (int(v) for v in z["seeds"])
    eng, _, _ = _engine(sf, si, conv_math)
    Ft = eng.interpolate(torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda(), ts).cpu().numpy()
    assert Ft.shape == (len(ts), 1, 1, 704, 1280)
    flow = eng.last["flow"].cpu().numpy()
    intrp = eng.last["intrp"].cpu().numpy().reshape(len(ts), 1, 5, 704, 1280)
    e = dict(flow=relerr(flow, z["flow"]), lattice=relerr(intrp[:, :, :, ::16, ::16], z["intrp_lattice"]),
             lattice_5_3=relerr(intrp[:, :, :, 5::16, 3::16], z["intrp_lattice_5_3"]), Ft=relerr(Ft, z["Ft"]))
    print("1280x704 %s: %s" % (conv_math, {k: "%.2e" % v for k, v in e.items()}))
    assert max(e.values()) < TOL, e
    if eng.conv_math == "auto":
        assert eng.flow_net.fallbacks == 0 and eng.interp_net.fallbacks == 0


@pytest.mark.parametrize("conv_math", CONV_MATHS)
def test_interpolation_with_tiny_trunk_activations(conv_math):
    """The adversarial fixture for the ACTIVATION side of the two-float16-piece convolutions (round-3 review, weak 1): the
    same function as the seeds-101/102 network, but every trunk activation is 2^-17 of its usual size (4e-7 ... 4e-6 per layer:
    float16 subnormals, h1 pieces rounding to zero unless the kernel scales its operands).  Generated by the reference in
    float32 and float64 (make_golden_slomo_allscale.py smallact); the float32 reference result equals the unscaled network's
    bit for bit, so every conv math must meet the plain 1e-5 bar here and the two-piece maths must not need the fallback."""
    sys_path_golden()
    from make_golden_slomo_allscale import smallact_state_dicts
    from v2e_amd.slomo import SloMoEngine
    z = np.load(os.path.join(GOLDEN, "slomo_smallact_64x96.npz"))
    assert z["act_max"][:-1].max() < 1e-5
    I0, I1 = _pairs(z)
    ts = list(z["ts"])
    sd_f, sd_i = smallact_state_dicts(int(z["log2s"]))
    eng = SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()},
                      {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda", conv_math=conv_math)
    Ft = eng.interpolate(torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda(), ts).cpu().numpy()
    got = {"flow": eng.last["flow"].cpu().numpy(), "intrp": eng.last["intrp"].cpu().numpy().reshape(len(ts), I0.shape[0], 5, 64, 96),
           "Ft": Ft}
    e = {k: relerr(v, z[k]) for k, v in got.items()}
    e64 = {k: float(np.max(np.abs(v.astype(np.float64) - z[k + "_f64"]))) for k, v in got.items()}
    print("tiny activations %s: vs reference f32 %s, vs f64 %s, fallbacks %d" % (
        conv_math, {k: "%.2e" % v for k, v in e.items()}, {k: "%.2e" % v for k, v in e64.items()},
        eng.flow_net.fallbacks + eng.interp_net.fallbacks))
    assert max(e.values()) < TOL, e
    # and the same result as the unscaled network gives with the same math: powers of two cost nothing
    eng0, _, _ = _engine(conv_math=conv_math)
    Ft0 = eng0.interpolate(torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda(), ts).cpu().numpy()
    assert relerr(Ft, Ft0) < 2e-6
    if eng.conv_math == "auto":
        assert eng.flow_net.fallbacks == 0 and eng.interp_net.fallbacks == 0


def sys_path_golden():
    import sys
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)


@pytest.mark.parametrize("fixture", ["slomo_trained_scale_64x96", "slomo_allscale_64x96"])
@pytest.mark.parametrize("conv_math", CONV_MATHS)
def test_interpolation_within_reference_float32_noise(conv_math, fixture):
    """Two stress fixtures generated by the reference in float32 AND float64 (make_golden_slomo_allscale.py): the conv3
    heads scaled so that |flow| reaches 30 px and the visibility logit 100; every layer scaled so that the trunk's
    activations run to 20 .. 200.  Per tensor, both conv maths: the distance to the float64 result in units of the
    reference's own float32 distance (rms and max), bounded by what was measured (test_slomo_oracle_golden.GPU_NOISE_FACTOR:
    1.2 .. 1.5 in rms with the heads scaled, 3.1 .. 3.8 with every layer scaled -- both conv maths alike, so the split-bf16
    operands are not what it comes from), and by 1e-5 of the tensor's scale for the networks' outputs."""
    from test_slomo_oracle_golden import GPU_NOISE_FACTOR, GPU_NOISE_FACTOR_FP16X2, _scaled_state_dicts, noise_ratio, noise_ratio_rms
    from v2e_amd.slomo import SloMoEngine
    z = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    I0, I1 = _pairs(z)
    ts = list(z["ts"])
    sd_f, sd_i = _scaled_state_dicts(z)
    eng = SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()},
                      {k: torch.from_numpy(v) for k, v in sd_i.items()}, "cuda", conv_math=conv_math)
    Ft = eng.interpolate(torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda(), ts).cpu().numpy()
    got = {"flow": eng.last["flow"].cpu().numpy(), "intrp": eng.last["intrp"].cpu().numpy().reshape(len(ts), I0.shape[0], 5, 64, 96),
           "Ft": Ft}
    r = {k: (round(noise_ratio_rms(v, z, k), 3), round(noise_ratio(v, z, k), 3)) for k, v in got.items()}
    print("noise ratios (rms, max) %s %s: %s" % (fixture, conv_math, r))
    b_rms, b_max = GPU_NOISE_FACTOR[fixture] if conv_math not in ("fp16x2", "auto") else GPU_NOISE_FACTOR_FP16X2[fixture]
    assert max(v[0] for v in r.values()) <= b_rms and max(v[1] for v in r.values()) <= b_max, r
    for k in ("flow", "intrp"):  # the networks' outputs: within 1e-5 of the tensor's scale of the exact result
        assert np.max(np.abs(got[k].astype(np.float64) - z[k + "_f64"])) <= 1e-5 * np.max(np.abs(z[k + "_f64"])), k


def test_warp_blend_fusion_match_reference_golden():
    from v2e_amd import _capi
    from v2e_amd._capi import check
    from v2e_amd.slomo import time_coefficients
    lib = _capi.lib()
    z = np.load(os.path.join(GOLDEN, "slomo_warp_64x96.npz"))
    I0, I1 = _pairs(z)
    ts = list(z["ts"])
    nt, b, h, w = len(ts), 1, 64, 96
    dev = torch.device("cuda")
    tI0, tI1 = torch.from_numpy(I0).to(dev), torch.from_numpy(I1).to(dev)
    flow = torch.from_numpy(z["flow"]).to(dev)
    coef = torch.from_numpy(time_coefficients(ts)).to(dev)
    x12 = torch.empty((nt * b, 12, h, w), dtype=torch.float32, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(lib.v2e_slomo_prep(p(tI0), p(tI1), p(flow), p(coef), nt, b, h, w, p(x12), s), "prep")
    assert relerr(x12.cpu().numpy().reshape(nt, b, 12, h, w)[:, :, 6:12], z["x12_tail"]) < TOL
    intrp = torch.from_numpy(z["intrp"].reshape(nt * b, 5, h, w)).to(dev)
    out = torch.empty((nt * b, 1, h, w), dtype=torch.float32, device=dev)
    check(lib.v2e_slomo_fuse(p(tI0), p(tI1), p(x12), p(intrp), p(coef), nt, b, h, w, p(out), s), "fuse")
    assert relerr(out.cpu().numpy().reshape(nt, b, 1, h, w), z["Ft"]) < TOL


def test_interpolation_matches_oracle_other_shape(oracle_lib):
    from v2e_amd.synth import int_gradient_frames
    H, W, B = 32, 160, 3
    fr = int_gradient_frames(B + 1, H, W, seed=4, noise=12, as_array=True).astype(np.float32) / np.float32(255.0)
    I0, I1 = fr[:B, None] - np.float32(0.428), fr[1:, None] - np.float32(0.428)
    eng, sd_f, sd_i = _engine(301, 302)
    ts = [(k + 0.5) / 4 for k in range(4)]
    Ft = eng.interpolate(torch.from_numpy(I0).cuda(), torch.from_numpy(I1).cuda(), ts).cpu().numpy()
    ref = oracle_lib.slomo_interpolate(I0, I1, ts, sd_f, sd_i)
    assert relerr(eng.last["flow"].cpu().numpy(), ref["flow"]) < TOL
    assert relerr(eng.last["intrp"].cpu().numpy(), ref["intrp"]) < TOL
    assert relerr(Ft, ref["Ft"]) < TOL


def test_superslomo_class_writes_frames(tmp_path, oracle_lib):
    """Drop-in class end to end: npy frames + checkpoint file in, numbered PNGs + times out."""
    from PIL import Image
    from v2e_amd import SuperSloMo
    from v2e_amd.synth import int_gradient_frames, portable_unet_state_dict
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir(); dst.mkdir()
    Hs, Ws, n = 40, 70, 5           # resized to 32 x 64 for the network (dataloader.py:122-123)
    fr = int_gradient_frames(n, Hs, Ws, seed=9, noise=6)
    for i, f in enumerate(fr):
        np.save(str(src / ("%08d.npy" % i)), f)
    sd_f, sd_i = portable_unet_state_dict(2, 4, 401), portable_unet_state_dict(12, 5, 402)
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"state_dictFC": {k: torch.from_numpy(v) for k, v in sd_f.items()},
                "state_dictAT": {k: torch.from_numpy(v) for k, v in sd_i.items()}}, str(ckpt))
    U = 3
    sm = SuperSloMo(model=str(ckpt), auto_upsample=False, upsampling_factor=U, batch_size=2)
    times, avg = sm.interpolate(str(src), str(dst), (Ws, Hs))
    assert avg == U and len(times) == (n - 1) * U
    assert np.allclose(times, np.arange((n - 1) * U) / U)
    pngs = sorted(os.listdir(str(dst)), key=lambda s: int(s.split(".")[0]))
    assert pngs == ["%d.png" % i for i in range((n - 1) * U)]
    # frame (pair 1, k=2) against the oracle driven the same way
    dim = (64, 32)
    def prep(a):
        im = np.asarray(Image.fromarray(a).resize(dim, Image.LANCZOS)).astype(np.float32) / np.float32(255.0)
        return (im - np.float32(0.428))[None, None]
    ts = [(k + 0.5) / U for k in range(U)]
    ref = oracle_lib.slomo_interpolate(prep(fr[1]), prep(fr[2]), ts, sd_f, sd_i)["Ft"][2, 0, 0]
    ref_u8 = ((ref + np.float32(0.428)) * np.float32(255.0)).astype(np.uint8)
    ref_img = np.asarray(Image.fromarray(ref_u8, mode="L").resize((Ws, Hs), Image.BILINEAR))
    got = np.asarray(Image.open(str(dst / ("%d.png" % (1 * U + 2)))))
    assert got.shape == (Hs, Ws)
    diff = np.abs(got.astype(int) - ref_img.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.01
    with pytest.raises(ValueError):
        SuperSloMo(model=str(ckpt), auto_upsample=False, upsampling_factor=1)


def test_auto_upsample_follows_the_flow_magnitude(tmp_path, oracle_lib):
    """auto_upsample=True (slomo.py:352-379): per batch, upsampling factor = ceil(max flow speed over the batch, both
    directions), at least the requested factor and at least 2; frame numbering and interpTimes follow the varying factor.
    The flow net's head is scaled so that speeds of several pixels occur; expected factors from the oracle's flow."""
    from PIL import Image
    from v2e_amd import SuperSloMo
    from v2e_amd.synth import int_gradient_frames, portable_unet_state_dict
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir(); dst.mkdir()
    Hs, Ws, n = 40, 70, 7
    fr = int_gradient_frames(n, Hs, Ws, seed=19, noise=10)
    for i, f in enumerate(fr):
        np.save(str(src / ("%08d.npy" % i)), f)
    sd_f, sd_i = portable_unet_state_dict(2, 4, 401), portable_unet_state_dict(12, 5, 402)
    sd_f["conv3.weight"] = sd_f["conv3.weight"] * np.float32(25.0)
    sd_f["conv3.bias"] = sd_f["conv3.bias"] * np.float32(25.0)
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"state_dictFC": {k: torch.from_numpy(v) for k, v in sd_f.items()},
                "state_dictAT": {k: torch.from_numpy(v) for k, v in sd_i.items()}}, str(ckpt))
    B = 2
    sm = SuperSloMo(model=str(ckpt), auto_upsample=True, upsampling_factor=3, batch_size=B)
    times, avg = sm.interpolate(str(src), str(dst), (Ws, Hs))

    def prep(a):
        im = np.asarray(Image.fromarray(a).resize((64, 32), Image.LANCZOS)).astype(np.float32) / np.float32(255.0)
        return (im - np.float32(0.428))[None, None]

    exp_times, factors, counter = [], [], 0
    for b0 in range(0, n - 1, B):
        idx = list(range(b0, min(b0 + B, n - 1)))
        I0 = np.concatenate([prep(fr[i]) for i in idx]); I1 = np.concatenate([prep(fr[i + 1]) for i in idx])
        flow = oracle_lib.unet_forward(np.concatenate((I0, I1), axis=1), sd_f)
        sp = np.sqrt(np.maximum(flow[:, 0] ** 2 + flow[:, 1] ** 2, flow[:, 2] ** 2 + flow[:, 3] ** 2))
        U = max(int(np.ceil(sp.max())), 3, 2)
        factors.append(U)
        exp_times += list(counter + np.arange(U * len(idx)) / U)
        counter += len(idx)
    assert max(factors) > 3, "the scaled flow head must make some batch exceed the requested factor"
    assert avg == sum(factors) / len(factors)
    assert np.allclose(times, exp_times)
    nout = sum(U * min(B, n - 1 - b0) for U, b0 in zip(factors, range(0, n - 1, B)))
    assert sorted(os.listdir(str(dst)), key=lambda s: int(s.split(".")[0])) == ["%d.png" % i for i in range(nout)]


def test_operand_scaling_and_range_guard_of_the_two_piece_math():
    """conv_math 'auto' / 'fp16x2': every convolution stages its activations times the power of two that puts the largest one
    (tracked by the producing convolution's epilogue) in [2^13, 2^14), so neither a network whose activations are 3e5 times
    larger nor one whose activations are 1e-5 times smaller leaves float16's normal range: same accuracy, no second pass.
    What is left for the guard is an activation that is inf: such a pass is redone with the exact three-bf16-piece
    split -- bit-identical to conv_math 'bf16x3' -- and the guard does not stick."""
    from v2e_amd.slomo import HipUNet
    from v2e_amd.synth import portable_unet_state_dict
    sd = {k: torch.from_numpy(v) for k, v in portable_unet_state_dict(12, 5, 102).items()}
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(9)
    x = (torch.rand((2, 12, 64, 96), generator=g) - 0.4).to(dev)
    auto, exact, fast = (HipUNet(sd, 12, 5, dev, m) for m in ("auto", "bf16x3", "fp16x2"))
    y = auto.forward(x)
    assert auto.fallbacks == 0 and torch.equal(y, fast.forward(x))
    ye = exact.forward(x)
    for scale in (3.0e5, 2.0 ** -17, 1.0e-5):   # beyond 65 504 in the first layers / float16 subnormals throughout
        ys = auto.forward(x * scale)
        assert auto.fallbacks == 0 and torch.isfinite(ys).all()
        es = exact.forward(x * scale)
        tol = 1e-5 * max(1.0, float(es.abs().max()))
        assert float((ys - es).abs().max()) <= tol, (scale, float((ys - es).abs().max()), tol)
    assert float((y - ye).abs().max()) <= 1e-5 * max(1.0, float(ye.abs().max()))
    xb = x.clone()
    xb[0, 3, 10, 10] = float("inf")
    yb = auto.forward(xb)
    assert auto.fallbacks == 1
    assert torch.equal(torch.nan_to_num(yb, nan=7.0), torch.nan_to_num(exact.forward(xb), nan=7.0))
    y2 = auto.forward(x)                # and the guard does not stick
    assert auto.fallbacks == 1 and torch.equal(y2, y)


@pytest.mark.gpu
def test_flow_started_ahead_on_the_side_stream_changes_nothing():
    """SloMoEngine.interpolate(..., next_pair=): the next batch's flow UNet runs on the engine's side stream beside this batch's
    interpolation UNet, and the range flags are read once per batch behind the fusion -- same kernels on the same inputs, so the
    frames are bit-identical to the one-stream order; an unclaimed look-ahead is dropped; an inf in a batch whose flow was
    started ahead still takes the exact split (both networks), as it does in line."""
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import portable_unet_state_dict
    sd_f = {k: torch.from_numpy(v) for k, v in portable_unet_state_dict(2, 4, 101).items()}
    sd_i = {k: torch.from_numpy(v) for k, v in portable_unet_state_dict(12, 5, 102).items()}
    dev = torch.device("cuda")
    eng = SloMoEngine(sd_f, sd_i, dev)
    g = torch.Generator().manual_seed(21)
    batches = [((torch.rand((2, 1, 64, 96), generator=g) - 0.428).to(dev), (torch.rand((2, 1, 64, 96), generator=g) - 0.428).to(dev))
               for _ in range(3)]
    ts = [0.25, 0.75]
    ref = [eng.interpolate(a, b, ts).clone() for a, b in batches]
    for i, (a, b) in enumerate(batches):
        out = eng.interpolate(a, b, ts, next_pair=batches[i + 1] if i + 1 < len(batches) else None)
        assert torch.equal(out, ref[i]), i
    assert eng._ahead is None
    eng.flow_ahead(*batches[0])                      # never claimed: the next call is for other tensors
    assert torch.equal(eng.interpolate(*batches[1], ts), ref[1]) and eng._ahead is None
    assert eng.flow_net.fallbacks == 0 and eng.interp_net.fallbacks == 0
    bad = (batches[2][0].clone(), batches[2][1])
    bad[0][1, 0, 5, 7] = float("inf")
    want = eng.interpolate(bad[0], bad[1], ts).clone()
    f0, i0 = eng.flow_net.fallbacks, eng.interp_net.fallbacks
    assert f0 >= 1
    eng.interpolate(*batches[0], ts, next_pair=bad)
    got = eng.interpolate(bad[0], bad[1], ts)
    assert eng.flow_net.fallbacks == 2 * f0 and eng.interp_net.fallbacks == 2 * i0
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))
    assert torch.equal(eng.interpolate(*batches[1], ts), ref[1])   # and nothing sticks


@pytest.mark.gpu
def test_pooled_copy_from_the_convolution_epilogue_equals_the_pooling_pass(tmp_path):
    """conv2 and down1.conv2 leave avg_pool2d(2) of their output beside it (slomo_s3.h epilogue: the window is two registers of a
    lane and of its neighbour lane, added in k_avgpool2's order); V2E_AMD_FUSE_POOL=0 restores the separate pooling passes.  Same
    numbers either way, in every conv math that has the tiles (and trivially in f32, which never takes the request)."""
    import subprocess, sys, os
    code = (
        "import sys, numpy as np, torch\n"
        "from v2e_amd.slomo import HipUNet\n"
        "from v2e_amd.synth import portable_unet_state_dict\n"
        "sd = {k: torch.from_numpy(v) for k, v in portable_unet_state_dict(12, 5, 102).items()}\n"
        "g = torch.Generator().manual_seed(5)\n"
        "x = (torch.rand((3, 12, 64, 96), generator=g) - 0.4).cuda()\n"
        "np.savez(sys.argv[1], **{m: HipUNet(sd, 12, 5, torch.device('cuda'), m).forward(x).cpu().numpy() for m in ('auto', 'bf16x3', 'f32')})\n")
    outs = {}
    for flag in ("1", "0"):
        env = dict(os.environ, V2E_AMD_FUSE_POOL=flag, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        path = str(tmp_path / ("pool%s.npz" % flag))
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env, timeout=600)
        outs[flag] = np.load(path)
    for m in ("auto", "bf16x3", "f32"):
        assert np.array_equal(outs["1"][m], outs["0"][m]), m
