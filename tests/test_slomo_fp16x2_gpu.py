"""The default SuperSloMo convolution math (conv_math "auto" / "fp16x2": two float16 pieces per operand, v2e_amd/csrc/slomo_s3.h
with NP = 2) pinned layer by layer and range slot by range slot.

Layers: every k_conv_s3<..., 2> instantiation that conv_dispatch_h2 (v2e_amd/csrc/slomo.hip) can select, through the public v2e_conv2d_lrelu with split_kind = 2 | (scale_log2 << 8), against the float64-accumulating CPU
oracle at the project's bar (test_slomo_gpu.TOL), inside guard bands, and sample by sample.  A whole UNet pass cannot reach
several of them (its 32-channel layers sit at full resolution, h % 32 == 0 and w % 32 == 0).

Range slots: what v2e_unet_forward leaves in its 32 slot words (the float32 bits of the largest |value| of the input and of every
convolution's output), bit for bit against the tensors of the same pass, and the power of two a two-piece layer derives from them.
"""
import numpy as np
import pytest
import torch

from slomo_layers import _Layer, _case_tensors
from test_slomo_gpu import TOL, relerr

pytestmark = pytest.mark.gpu

# (k, cin0, cin1, cout, n, h, w): every `return launch_conv_s3<KS, CT, PT, WP, TW, NB, MODE, RG, 2>` of conv_dispatch_h2, the two-piece
# tile selection.  A tile is WP * PT * 32 / TW rows of TW pixels; "ragged" = the last tile row partly masked.
H2_CASES = [
    # 3x3, cout % 64 == 0: 64 x 64 register tiles, one kernel row of weights resident (RG)
    (3, 32, 0, 64, 2, 20, 32),      # <3,2,2,4,32,1,0,1,2>: 8 x 32 tiles, ragged (20 = 2 * 8 + 4)
    (3, 64, 0, 128, 1, 16, 64),     # <3,2,2,4,32,1,0,1,2>: two tiles across, two channel blocks, n = 1
    (3, 16, 0, 64, 3, 24, 48),      # <3,2,2,4,16,1,0,1,2>: 16 x 16 tiles, ragged, odd n
    (3, 16, 16, 64, 2, 16, 48),     # <3,2,2,4,16,1,0,1,2>: fused concat at the chunk boundary
    (3, 32, 0, 64, 1, 40, 24),      # <3,2,2,4,8,1,0,1,2>: 32 x 8 tiles, ragged (40 = 32 + 8)
    (3, 256, 256, 256, 1, 8, 40),   # <3,2,2,4,8,1,0,1,2>: up.conv2 at a 40-wide level: concat, 4 channel blocks (1-D grid in XCD order,
                                    #                      5 pixel tiles padded to 8), three quarters of the tile masked
    (3, 16, 0, 64, 33, 16, 32),     # <3,2,2,4,32,1,0,1,2>: many samples
    # 3x3, cout = 32 / 96 at w % 32 == 0: the 32-channel x 128-pixel PT = 4 tile (h % 16 == 0) and its neighbour
    (3, 64, 0, 32, 2, 32, 64),      # <3,1,4,4,32,1,0,1,2>: up5.conv1's shape class
    (3, 32, 32, 32, 1, 16, 32),     # <3,1,4,4,32,1,0,1,2>: up5.conv2, fused concat, one tile
    (3, 16, 0, 96, 3, 16, 32),      # <3,1,4,4,32,1,0,1,2>: cout 96, odd n
    (3, 64, 0, 32, 2, 24, 64),      # <3,1,2,4,32,1,0,0,2>: h % 16 != 0; cin 64: the two-chunks-in-flight steady state
    (3, 16, 0, 96, 1, 12, 32),      # <3,1,2,4,32,1,0,0,2>: ragged (12 = 8 + 4), one chunk, cout 96
    (3, 48, 0, 32, 1, 8, 32),       # <3,1,2,4,32,1,0,0,2>: three chunks (the tail of the chunk pipeline)
    (3, 32, 0, 32, 2, 24, 48),      # <3,1,2,4,16,1,0,0,2>: ragged
    (3, 16, 16, 96, 1, 16, 16),     # <3,1,2,4,16,1,0,0,2>: fused concat, cout 96
    (3, 32, 0, 96, 3, 40, 24),      # <3,1,2,4,8,1,0,0,2>: ragged, odd n
    (3, 16, 0, 32, 1, 32, 8),       # <3,1,2,4,8,1,0,0,2>: a single column of tiles
    # 20- and 10-wide levels (of a 320 x 256 input): five-wave tiles; cout % 64 == 0 comes here too when w % 8 != 0
    (3, 64, 0, 64, 3, 16, 20),      # <3,1,2,5,20,1,0,0,2>: 16 x 20, one sample per workgroup, two pixel tiles per wave
    (3, 32, 0, 32, 2, 32, 60),      # <3,1,2,5,20,1,0,0,2>: three tiles across, two down
    (3, 16, 16, 32, 1, 16, 20),     # <3,1,2,5,20,1,0,0,2>: fused concat
    (3, 64, 0, 64, 2, 8, 20),       # <3,1,1,5,20,1,0,0,2>: 8 x 20
    (3, 32, 0, 96, 3, 24, 60),      # <3,1,1,5,20,1,0,0,2>: h = 24 (h % 8 == 0, h % 16 != 0), nine tiles per sample
    (3, 32, 0, 32, 2, 16, 10),      # <3,1,1,5,10,1,0,0,2>: the whole 16 x 10 tile
    (3, 64, 0, 64, 3, 8, 10),       # <3,1,1,5,10,1,0,0,2>: the 8 x 10 level, lower half masked
    (3, 32, 32, 96, 4, 8, 10),      # <3,1,1,5,10,1,0,0,2>: ... with the fused concat
    (3, 16, 0, 64, 5, 5, 10),       # <3,1,1,5,10,1,0,0,2>: eleven rows masked
    (3, 512, 0, 512, 1, 2, 10),     # <3,1,1,5,10,1,0,0,2>: the 2 x 10 level of a 32 x 160 input, 32 chunks
    # 5x5
    (5, 32, 0, 64, 2, 24, 64),      # <5,2,2,4,32,1,0,1,2>: down1.conv1
    (5, 64, 0, 64, 1, 12, 32),      # <5,2,2,4,32,1,0,1,2>: ragged
    (5, 64, 0, 32, 2, 20, 32),      # <5,1,2,4,32,1,0,0,2>: cout 32, ragged
    (5, 16, 0, 96, 3, 16, 96),      # <5,1,2,4,32,1,0,0,2>: cout 96, odd n
    # 7x7
    (7, 32, 0, 32, 2, 16, 64),      # <7,1,2,4,32,1,0,0,2>: conv2, h % 16 == 0
    (7, 32, 0, 32, 1, 20, 32),      # <7,1,2,4,32,1,0,0,2>: h % 16 != 0, ragged
    (7, 12, 0, 32, 2, 16, 64),      # <7,1,2,4,32,1,1,0,2>: the interpolation UNet's conv1: 12 channels, the chunk padded with zeros
    (7, 12, 0, 32, 1, 12, 32),      # <7,1,2,4,32,1,1,0,2>: ... ragged
    (7, 8, 0, 32, 1, 40, 96),       # <7,1,2,4,32,1,1,0,2>: a whole empty channel group
    (7, 24, 0, 64, 3, 32, 32),      # <7,1,2,4,32,1,1,0,2>: second chunk partial, two channel blocks, odd n
]

# shapes with no two-piece tile: conv_dispatch_s3 returns 1 (or v2e_conv2d_lrelu does not ask it) and the f32 matrix-core kernel runs
H2_FALLBACK_CASES = [
    (3, 64, 0, 64, 2, 8, 12),       # w = 12
    (3, 32, 0, 32, 3, 4, 20),       # 4 x 20: 20-wide but not whole 8-row tiles
    (3, 16, 0, 32, 2, 24, 10),      # 10-wide but taller than the 16-row tile
    (3, 8, 8, 32, 2, 16, 32),       # concat that is not at a 16-channel chunk boundary
    (5, 32, 0, 64, 1, 12, 48),      # 5x5 at w % 32 != 0
    (7, 32, 0, 32, 1, 16, 48),      # 7x7 at w % 32 != 0
]


def test_the_oracle_stays_affordable():
    """No layer case costs the oracle more than the largest of test_slomo_gpu.S3_CASES (7x7 32 -> 32 at 256 x 320)."""
    for k, c0, c1, cout, n, h, w in H2_CASES + H2_FALLBACK_CASES:
        assert n * h * w * (c0 + c1) * cout * k * k <= 256 * 320 * 32 * 32 * 49


@pytest.mark.parametrize("case", H2_CASES + H2_FALLBACK_CASES)
def test_two_piece_conv_layer_matches_oracle(case, oracle_lib):
    k, c0, c1, cout, n, h, w = case
    has_tile = case in H2_CASES
    x0, x1, wt, b = _case_tensors(case)
    layer = _Layer(wt, b)
    y = layer.run(x0, x1, "fp16x2")          # guard bands are checked inside, for all three kernels
    y32 = layer.run(x0, x1, "f32")
    y3 = layer.run(x0, x1, "bf16x3")
    xin = x0 if x1 is None else np.concatenate((x0, x1), axis=1)
    ref = oracle_lib.conv2d_lrelu(xin, wt, b)
    assert not np.isnan(y).any(), "output not fully written (or a NaN from beyond the input was consumed)"
    e_ref, e_32 = relerr(y, ref), relerr(y, y32)
    print("fp16x2 layer %s%s: relerr vs oracle %.3e, vs f32 kernel %.3e (f32 kernel vs oracle %.3e, bf16x3 %.3e), sl2 %d" % (
        case, "" if has_tile else " [f32 fallback]", e_ref, e_32, relerr(y32, ref), relerr(y3, ref), layer.sl2))
    assert e_ref < TOL
    assert e_32 < TOL
    assert relerr(y3, ref) < TOL
    if has_tile:   # it is not the same kernel three times
        assert not np.array_equal(y, y32) and not np.array_equal(y, y3)
    else:          # by design: the very kernel the f32 math runs
        assert np.array_equal(y, y32)
    # sample independence: the dispatch does not look at n and every output's accumulation chain is fixed, so a sample of a batch
    # is bit for bit the sample run alone -- on the tiles that split a sample over waves or mask half of themselves too
    if n > 1:
        for i in range(n):
            yi = layer.run(x0[i:i + 1], None if x1 is None else x1[i:i + 1], "fp16x2")
            assert np.array_equal(yi[0], y[i]), "sample %d of %d differs from the same sample run alone" % (i, n)


# ---------------------------------------------------------------- the range slots of a forward pass

def _bits(v):
    """float32 bit pattern of a 0-d tensor / number, as int."""
    return int(np.asarray(float(v), np.float32).view(np.uint32))


def _amax_bits(t):
    return _bits(t.abs().max())


def act_scale_exponent(m_bits, sl2):
    """Model of act_scale (v2e_amd/csrc/slomo.hip): the k of the power of two 2^k a two-piece layer stages its activations times,
    from the float32 bits of the largest |input| and the layer's weight exponent sl2 (split_kind >> 8).  k = 140 - biased
    exponent puts the maximum in [2^13, 2^14); it is clamped so that 2^-(k + sl2) stays a normal float32."""
    e = m_bits >> 23
    assert 0 < e < 255, "the model covers finite, normal, non-zero maxima"
    return min(126 - max(sl2, 0), max(-126, 140 - e))


# conv i reads the slot of what produced its x0 (the convolution before it -- avg_pool2d and the bilinear x2 in between cannot
# exceed their input's maximum -- or slot 0, the network input) and, with a fused concat, the slot of the skip tensor's producer
_SKIP_OF = {13: 9, 15: 7, 17: 5, 19: 3, 21: 1}               # up<u>.conv2 <- down<5-u>.conv2 / conv2
_SURVIVORS = {1: "s1", 3: "s2", 5: "s3", 7: "s4", 9: "s5", 20: "tA", 21: "tB"}   # convolution -> where its output still is afterwards


def _check_pass(unet, x, tag):
    n, _, h, w = x.shape
    am = unet.range_slots(n, h, w)
    ten = unet.workspace_tensors(n, h, w)
    assert int(am[0]) == _amax_bits(x), "%s: slot 0 is not max|x|" % tag
    for i, name in _SURVIVORS.items():
        want = _amax_bits(ten[name])
        assert int(am[1 + i]) == want, "%s: slot of convolution %d is %#x, max|%s| is %#x" % (tag, i, int(am[1 + i]), name, want)
    for i in range(22):   # (convolution 22's slot has no reader; the 4- / 5-channel conv3 kernel does not write it)
        v = am[1 + i:2 + i].view(np.float32)[0]
        assert np.isfinite(v) and v > 0.0, "%s: slot of convolution %d holds %r" % (tag, i, v)
    assert not am[24:].any(), "%s: the unused slot words are zeroed at the start of every pass" % tag
    # the scale every layer of this pass picks from its slots is the documented one (include/v2e_amd.h,
    # v2e_conv_set_range_flag: the largest activation staged in [2^13, 2^14)) -- act_scale_exponent is a model of act_scale
    for i in range(23):
        m = int(am[i])   # slot 1 + (i - 1), or the input's slot 0 for conv1
        if i in _SKIP_OF:
            m = max(m, int(am[1 + _SKIP_OF[i]]))
        k = act_scale_exponent(m, int(unet.descs[i].split_kind) >> 8)
        staged = float(np.array([m], np.uint32).view(np.float32)[0]) * 2.0 ** k
        assert 2.0 ** 13 <= staged < 2.0 ** 14, "%s: convolution %d would stage its largest input at %g" % (tag, i, staged)
    return am


def test_a_pass_leaves_nothing_behind_for_a_stand_alone_layer():
    """What a forward pass hands its layers (range slots, a pooled-copy request) ends with the pass: the same stand-alone
    convolution before and after a tracked pass in the same process gives the same bits inside intact guard bands (with a
    slot left over it would scale its operands and write the slot), and it leaves the pass's 32 slot words as they were."""
    from v2e_amd.slomo import HipUNet
    from v2e_amd.synth import portable_unet_state_dict
    x0, x1, wt, b = _case_tensors((3, 16, 0, 64, 1, 16, 32))
    layer = _Layer(wt, b)
    before = layer.run(x0, x1, "fp16x2")
    dev = torch.device("cuda")
    sd = {k: torch.from_numpy(v) for k, v in portable_unet_state_dict(12, 5, 512).items()}
    unet = HipUNet(sd, 12, 5, dev, "fp16x2")
    x = (torch.rand((1, 12, 32, 32), generator=torch.Generator().manual_seed(1232)) - 0.4).to(dev)
    y = unet.forward(x)
    assert unet.fallbacks == 0 and bool(torch.isfinite(y).all())
    am = _check_pass(unet, x, "fp16x2 1x32x32 cin 12")     # the pass was tracked: its slots hold its maxima
    after = layer.run(x0, x1, "fp16x2")                     # guard bands are checked inside
    assert np.array_equal(before, after), "a stand-alone layer changed after a forward pass in the same process"
    assert np.array_equal(unet.range_slots(1, 32, 32), am), "a stand-alone layer wrote a range slot of the pass before it"


SLOT_SHAPES = [(2, 64, 96), (3, 256, 320), (2, 32, 160), (1, 96, 64)]   # (n, h, w)


@pytest.mark.parametrize("conv_math", ("fp16x2", "auto"))
@pytest.mark.parametrize("cin,cout", ((2, 4), (12, 5)))
@pytest.mark.parametrize("shape", SLOT_SHAPES)
def test_range_slots_hold_the_maxima_of_the_pass(shape, cin, cout, conv_math):
    """64 x 96: the 12-, 6- and 3-wide levels run the f32 fallback kernels, which must feed the slots too; 320 x 256 with 3
    samples: the 16 x 20 and 8 x 10 tiles with masked halves; 32 x 160: the 4 x 20 fallback and the 2 x 10 tile; 96 x 64."""
    from v2e_amd.slomo import HipUNet
    from v2e_amd.synth import portable_unet_state_dict
    n, h, w = shape
    sd = {k: torch.from_numpy(v) for k, v in portable_unet_state_dict(cin, cout, 500 + cin).items()}
    dev = torch.device("cuda")
    unet = HipUNet(sd, cin, cout, dev, conv_math)
    g = torch.Generator().manual_seed(n * 1000 + h + w + cin)
    x = (torch.rand((n, cin, h, w), generator=g) - 0.4).to(dev)
    y = unet.forward(x)
    assert unet.fallbacks == 0 and bool(torch.isfinite(y).all())
    tag = "%s %dx%dx%d cin %d" % (conv_math, n, h, w, cin)
    am1 = _check_pass(unet, x, tag)
    # no stale slots: a second, smaller pass on the same object leaves the maxima of THAT pass (a slot kept would be larger)
    x2 = x * 2.0 ** -6
    unet.forward(x2)
    assert unet.fallbacks == 0
    am2 = _check_pass(unet, x2, tag + " second pass")
    assert _bits(np.float32(2.0 ** -6) * am1[0:1].view(np.float32)[0]) == int(am2[0])
    assert int(am2[0]) < int(am1[0])
