"""The SuperSloMo convolutions beside the default math, pinned tile by tile: the three-bf16-piece kernels k_conv_s3 / k_conv_s3p
(conv_math "bf16x3": slomo_s3.h, slomo_s3p.h), the f32 matrix-core kernel k_conv (slomo_conv.h) every mode falls back to, and the
VALU kernel of the 4- / 5-channel head, k_conv3x3_small (slomo_stream.h).  test_slomo_fp16x2_gpu.py does the same for the default.

Three tables, keyed by the instantiation a case is meant to reach, the template argument list spelled as the dispatch source
spells it: "s3p<16>", "s3<3,1,1,5,10>", "conv<3,8,2,1,5,20,1>", "conv_stacked<3,8,1,1,5,10>", "small<4>".  Every case runs through
the public v2e_conv2d_lrelu inside guard bands (slomo_layers._Layer) and is held to test_slomo_gpu.TOL against the CPU oracle.

test_tables_name_every_tile_the_dispatch_can_select needs no GPU.  It maps every case to its key with a Python model of
conv_dispatch, launch_conv_tw, conv_dispatch_s3 (three pieces), conv_dispatch_s3p and the head branch of conv_layer, and it
compares the keys with the launch_conv*<...> instantiations a regular expression finds in the bodies of those functions: a tile
added to the dispatch without a case here fails it.  profiles/r23_slomo_conv_tile_kernels.txt lists the kernels a profiled run
of this module launched, the evidence that the model routes as the C++ does.

The f32 kernel's CT = 2 ("wide") tiles are selected once n * ceil(h * w / 256) * (cout / 64) >= 4096, so their cases have
thousands of tiny samples; the oracle then runs on four of them, and every sample is compared with the GPU's own CT = 1 result
on batches of 8.  That comparison is for EQUAL bits: in k_conv every output is one accumulator element of one chain of
v_mfma_f32_32x32x2_f32 over (channel chunk, ky, kx, channel pair) in that order; CT only sets how many independent chains of
32 output channels a wave carries, so the arithmetic of an output does not depend on it (nor on the tile width).

The `wgs64 < 2048` branch of launch_conv_tw's 20-wide tile (a wide layer sent to the CT = 1 tile after all) is reachable only
at widths such as 100 with h = 8; 1024 samples of 8 x 100 with 8 -> 64 channels fit the cost cap and are in the table.
"""
import os
import re

import numpy as np
import pytest

from slomo_layers import _Layer, _case_tensors
from test_slomo_gpu import CONV_CASES, TOL, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_MAC_CAP = 5e8   # multiply-adds one case may ask of the oracle
WIDE_CHECKED = 4       # samples of a wide case the oracle computes


def _cc(*case):
    """A case test_slomo_gpu.CONV_CASES already has (and keeps running in its own test), by reference."""
    assert case in CONV_CASES, "%r is no longer one of test_slomo_gpu.CONV_CASES" % (case,)
    return case


# ---------------------------------------------------------------- the tables
# bf16x3: (k, c0, c1, cout, n, h, w).  A k_conv_s3 tile is WP * PT * 32 / TW rows of TW pixels, a k_conv_s3p tile 256 / TW rows;
# with two or more 64-channel blocks k_conv_s3p's grid is 1-D in XCD order, (ntiles + 7) / 8 * 8 * ncb workgroups.
S3_TILES = {
    "s3p<32>": [
        (3, 32, 0, 64, 1, 8, 32),       # one tile, one chunk pair, 2-D grid
        (3, 32, 0, 64, 3, 20, 64),      # ragged rows (20 = 2 * 8 + 4), odd n
        (3, 96, 0, 128, 3, 12, 32),     # three chunk pairs, ncb = 2, 6 pixel tiles padded to 8
        (3, 48, 16, 64, 2, 8, 32),      # a chunk pair that straddles the concat
        (3, 32, 32, 256, 1, 16, 32),    # ncb = 4, 2 tiles padded to 8
    ],
    "s3p<16>": [
        (3, 64, 0, 64, 2, 24, 48),      # ragged rows (24 = 16 + 8), three tiles across
        (3, 16, 16, 128, 3, 16, 16),    # first concat source an odd multiple of 16 channels, ncb = 2, 3 tiles padded to 8
    ],
    "s3p<8>": [
        (3, 32, 0, 64, 2, 40, 24),      # ragged rows (40 = 32 + 8)
        (3, 64, 64, 128, 1, 8, 40),     # three quarters of the tile masked, 5 tiles padded to 8
    ],
    # k_conv_s3 with three pieces: where k_conv_s3p refuses (cout % 64 != 0 or cin % 32 != 0) or has no tile width
    "s3<3,1,2,4,32>": [(3, 16, 0, 32, 2, 20, 32), (3, 48, 0, 96, 1, 8, 64), (3, 16, 16, 32, 1, 12, 32)],
    "s3<3,1,2,4,16>": [(3, 32, 0, 32, 3, 24, 48), (3, 16, 16, 96, 1, 16, 16)],
    "s3<3,1,2,4,8>": [(3, 32, 0, 96, 3, 40, 24), (3, 16, 0, 32, 1, 32, 8)],
    "s3<3,1,1,5,20>": [(3, 64, 0, 64, 3, 16, 20), (3, 32, 0, 32, 2, 24, 60), (3, 16, 16, 32, 1, 8, 20)],
    "s3<3,1,1,5,10>": [
        (3, 32, 0, 32, 2, 16, 10),      # the whole 16 x 10 tile
        (3, 64, 0, 64, 3, 8, 10),       # lower half masked
        (3, 32, 32, 96, 4, 8, 10),      # ... with the fused concat
        (3, 16, 0, 64, 5, 5, 10),       # eleven rows masked
        (3, 512, 0, 512, 1, 2, 10),     # 32 chunks
    ],
    "s3<5,1,2,4,32>": [(5, 32, 0, 64, 2, 24, 64), (5, 64, 0, 32, 2, 20, 32), (5, 16, 0, 96, 3, 16, 96)],
    "s3<7,1,2,4,32>": [(7, 32, 0, 32, 2, 16, 64), (7, 32, 0, 32, 1, 20, 32)],
    "s3<7,1,2,4,32,1,1>": [(7, 12, 0, 32, 2, 16, 64), (7, 8, 0, 32, 1, 40, 96), (7, 24, 0, 64, 3, 32, 32)],
}

# shapes a bf16x3 layer has no tile for: the f32 kernel under the key runs, and its very bits come out
S3_FALLBACKS = {
    "conv<3,8,1,2,4,32,0>": [
        (3, 64, 0, 64, 2, 8, 12),       # w = 12: no width fits, the masked 32-wide tile
        (3, 8, 8, 32, 2, 16, 32),       # concat that is not at a 16-channel chunk boundary
        (3, 24, 0, 32, 1, 8, 32),       # cin % 16 != 0
    ],
    "conv<3,8,1,1,5,10,0>": [
        (3, 32, 0, 32, 3, 4, 20),       # 20-wide but not whole 8-row tiles: for k_conv too, which takes two 10-wide tiles across
        (3, 16, 0, 32, 2, 24, 10),      # 10-wide but taller than the 16-row tile
    ],
    "conv<5,4,1,2,4,32,0>": [(5, 32, 0, 64, 1, 12, 48)],   # 5x5 at w % 32 != 0
    "conv<7,4,1,2,4,32,0>": [(7, 32, 0, 32, 1, 16, 48)],   # 7x7 at w % 32 != 0
    "conv<7,2,1,2,4,32,0>": [(7, 2, 0, 32, 1, 16, 32)],    # the flow UNet's conv1: fewer than 8 channels
}

# f32: (k, c0, c1, cout, n, h, w, pre).  Tiles are WP * PT * 32 / TW rows of TW pixels: 8 x 32, 16 x 16, 32 x 8, 8 x 20, 16 x 10.
_W = (3, 8, 0, 128, 2048)   # 2048 samples x two 64-channel blocks: wide at any image of at most 256 pixels
F32_TILES = {
    "conv<7,4,1,2,4,32,0>": [_cc(7, 12, 0, 32, 1, 40, 72, 0)],
    "conv<7,2,1,2,4,32,0>": [_cc(7, 2, 0, 32, 2, 32, 64, 0)],
    "conv<5,4,1,2,4,32,0>": [_cc(5, 64, 0, 64, 1, 24, 40, 0)],
    "conv<5,4,1,2,4,32,1>": [_cc(5, 32, 0, 64, 2, 24, 40, 1)],
    "conv<5,4,2,2,4,32,0>": [(5, 4, 0, 128, 2048, 4, 32, 0)],
    "conv<5,4,2,2,4,32,1>": [(5, 4, 0, 128, 2048, 4, 32, 1)],
    "conv<3,8,1,2,4,32,0>": [_cc(3, 32, 32, 32, 1, 32, 64, 0),
                             _cc(3, 256, 256, 256, 1, 8, 12, 0),     # masked: 12 is no multiple of 8, 10 or 20
                             (3, 8, 0, 32, 3, 9, 27, 0)],           # masked and ragged, odd n
    "conv<3,8,1,2,4,32,1>": [(3, 16, 0, 32, 2, 12, 32, 1), _cc(3, 512, 0, 512, 2, 2, 3, 1)],
    "conv<3,8,1,2,4,32,2>": [_cc(3, 64, 0, 32, 1, 32, 64, 2), _cc(3, 512, 0, 512, 2, 4, 6, 2)],
    "conv<3,8,1,2,4,16,0>": [(3, 16, 0, 32, 2, 24, 48, 0)],
    "conv<3,8,1,2,4,16,1>": [_cc(3, 64, 0, 128, 2, 16, 48, 1)],
    "conv<3,8,1,2,4,16,2>": [(3, 8, 0, 32, 3, 12, 16, 2)],
    "conv<3,8,1,2,4,8,0>": [_cc(3, 128, 0, 128, 3, 8, 40, 0)],
    "conv<3,8,1,2,4,8,1>": [(3, 16, 0, 64, 2, 20, 24, 1)],
    "conv<3,8,1,2,4,8,2>": [(3, 8, 0, 32, 1, 34, 8, 2)],
    "conv<3,8,1,1,5,20,0>": [_cc(3, 64, 0, 64, 3, 16, 20, 0),
                             (3, 8, 0, 64, 1024, 8, 100, 0)],        # wide, but wgs64 = 1024 < 2048: the CT = 1 tile after all
    "conv<3,8,1,1,5,20,1>": [(3, 16, 0, 32, 2, 8, 20, 1)],
    "conv<3,8,1,1,5,20,2>": [(3, 8, 0, 32, 3, 16, 60, 2)],
    "conv_stacked<3,8,1,1,5,10>": [_cc(3, 64, 0, 64, 3, 8, 10, 0),   # odd n: the last tile's second sample masked
                                   _cc(3, 32, 32, 96, 4, 8, 10, 0),  # the fused concat
                                   (3, 16, 0, 32, 1, 8, 10, 0)],     # n = 1
    "conv<3,8,1,1,5,10,0>": [(3, 16, 0, 32, 3, 20, 30, 0)],          # h != 8: ragged rows, three tiles across
    "conv<3,8,1,1,5,10,1>": [(3, 8, 0, 32, 2, 8, 10, 1)],            # h == 8 but pre != 0
    "conv<3,8,1,1,5,10,2>": [(3, 16, 0, 64, 3, 8, 10, 2)],
    "conv<3,8,2,2,4,32,0>": [_W + (2, 32, 0)],
    "conv<3,8,2,2,4,32,1>": [_W + (2, 32, 1)],
    "conv<3,8,2,2,4,32,2>": [_W + (2, 32, 2)],
    "conv<3,8,2,2,4,16,0>": [_cc(3, 8, 0, 128, 2048, 16, 16, 0)],
    "conv<3,8,2,2,4,16,1>": [_W + (4, 16, 1)],
    "conv<3,8,2,2,4,16,2>": [_W + (4, 16, 2)],
    "conv<3,8,2,2,4,8,0>": [_W + (8, 8, 0)],
    "conv<3,8,2,2,4,8,1>": [_W + (8, 8, 1)],
    "conv<3,8,2,2,4,8,2>": [_W + (8, 8, 2)],
    "conv<3,8,2,1,5,20,0>": [_W + (8, 20, 0)],                       # wgs64 = 4096
    "conv<3,8,2,1,5,20,1>": [_W + (8, 20, 1)],
    "conv<3,8,2,1,5,20,2>": [_W + (8, 20, 2)],
    "conv<3,8,2,1,5,10,0>": [_W + (4, 10, 0)],                       # h != 8, or it would be the stacked tile
    "conv<3,8,2,1,5,10,1>": [_W + (8, 10, 1)],
    "conv<3,8,2,1,5,10,2>": [_W + (4, 10, 2)],
}

# the head: (k, c0, c1, cout, n, h, w, pre).  k_conv3x3_small tiles are 16 rows of 64 pixels, four pixels along x per thread,
# 8-channel chunks; a float4 store where w % 4 == 0.
HEAD_TILES = {
    "small<%d>" % co: [
        (3, 8, 0, co, 1, 1, 4, 0),      # one 4-pixel group of one row
        (3, 32, 0, co, 2, 16, 64, 0),   # one whole tile per sample
        (3, 40, 0, co, 3, 20, 70, 0),   # scalar stores (w % 4 != 0), ragged both ways, five chunks
        (3, 8, 0, co, 1, 33, 132, 0),   # third tile column with one 4-pixel group, third tile row with one row
    ] for co in (4, 5)
}
# a narrow layer with a concat or a fused pool skips that kernel: k_conv with cout no multiple of 32
HEAD_TILES["conv<3,8,1,2,4,32,0>"] = [(3, 8, 8, 5, 2, 16, 32, 0)]
HEAD_TILES["conv<3,8,1,2,4,32,1>"] = [(3, 16, 0, 4, 2, 16, 32, 1)]


def _flat(table):
    return [(key, case) for key, cases in table.items() for case in cases]


def _id(kc):
    key, c = kc
    return "%s-%dx%d+%d>%d-n%d-%dx%d%s" % ((key,) + tuple(c[:7]) + ("-pre%d" % c[7] if len(c) > 7 else "",))


# ---------------------------------------------------------------- a model of the dispatch (v2e_amd/csrc/slomo.hip, slomo_conv.h, slomo_s3p.h)
def is_wide(cout, n, h, w):
    """conv_dispatch: 64-channel tiles once that still leaves 16 workgroups per CU."""
    return cout >= 64 and n * ((h * w + 255) // 256) * (cout // 64) >= 4096


def model_conv_tw(ct, pre, cout, n, h, w):
    """launch_conv_tw<3, 8, CT, PRE>."""
    if w % 32 == 0:
        return "conv<3,8,%d,2,4,32,%d>" % (ct, pre)
    if w % 16 == 0:
        return "conv<3,8,%d,2,4,16,%d>" % (ct, pre)
    if w % 8 == 0:
        return "conv<3,8,%d,2,4,8,%d>" % (ct, pre)
    if w % 20 == 0 and h % 8 == 0:
        if ct == 2 and n * (h // 8) * (cout // 64) < 2048:
            ct = 1
        return "conv<3,8,%d,1,5,20,%d>" % (ct, pre)
    if w % 10 == 0:
        if pre == 0 and h == 8:
            return "conv_stacked<3,8,1,1,5,10>"
        return "conv<3,8,%d,1,5,10,%d>" % (ct, pre)
    return "conv<3,8,%d,2,4,32,%d>" % (ct, pre)


def model_conv_dispatch(k, cin, cout, n, h, w, pre):
    ct = 2 if is_wide(cout, n, h, w) else 1
    if k == 7:
        assert pre == 0
        return "conv<7,%d,1,2,4,32,0>" % (4 if cin % 4 == 0 else 2)
    if k == 5:
        assert pre in (0, 1)
        return "conv<5,4,%d,2,4,32,%d>" % (ct, pre)
    assert k == 3
    return model_conv_tw(ct, pre, cout, n, h, w)


def model_conv_dispatch_s3p(k, c0, c1, cout, w):
    if k != 3 or cout % 64 or (c0 + c1) % 32 or c0 % 16 or c1 % 16:
        return None
    for tw in (32, 16, 8):
        if w % tw == 0:
            return "s3p<%d>" % tw
    return None


def model_conv_dispatch_s3(k, c0, c1, cout, h, w):
    """conv_dispatch_s3 with three pieces; None where it returns 1."""
    cin = c0 + c1
    if k == 3:
        key = model_conv_dispatch_s3p(k, c0, c1, cout, w)
        if key:
            return key
        for tw in (32, 16, 8):
            if w % tw == 0:
                return "s3<3,1,2,4,%d>" % tw
        if w % 20 == 0 and h % 8 == 0:
            return "s3<3,1,1,5,20>"
        if w == 10 and h <= 16:
            return "s3<3,1,1,5,10>"
        return None
    if k == 5 and w % 32 == 0:
        return "s3<5,1,2,4,32>"
    if k == 7 and w % 32 == 0:
        return "s3<7,1,2,4,32>" if cin % 16 == 0 else "s3<7,1,2,4,32,1,1>"
    return None


def model_conv_layer(case, split):
    """conv_layer for pre 0 / 1 / 2: its argument checks, the head branch, then the split-operand tiles (split: the layer has
    three-piece weights) and the f32 kernel."""
    k, c0, c1, cout, n, h, w = case[:7]
    pre = case[7] if len(case) > 7 else 0
    cin = c0 + c1
    assert pre == 0 or c1 == 0
    assert pre != 2 or (h % 2 == 0 and w % 2 == 0)
    assert c1 == 0 or c0 % 8 == 0
    assert (k == 3 and cin % 8 == 0) or (k == 5 and cin % 4 == 0) or (k == 7 and cin % 2 == 0)
    if k == 3 and pre == 0 and c1 == 0 and cout in (4, 5):
        return "small<%d>" % cout
    s3_cin = cin % 16 == 0 or (k == 7 and c1 == 0 and cin >= 8)
    if split and pre == 0 and s3_cin and cout % 32 == 0 and (c1 == 0 or c0 % 16 == 0):
        key = model_conv_dispatch_s3(k, c0, c1, cout, h, w)
        if key:
            return key
    return model_conv_dispatch(k, cin, cout, n, h, w, pre)


def case_is_wide(case):
    k, c0, c1, cout, n, h, w = case[:7]
    return k != 7 and is_wide(cout, n, h, w)


# ---------------------------------------------------------------- what the dispatch source can launch
def _function_body(src, signature):
    i = src.index(signature)
    j = src.index("{", i)
    depth, e = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(src[e], 0)
        if depth == 0:
            return src[j:e + 1]
        e += 1


_LAUNCH = re.compile(r"\blaunch_(conv\w*)\s*<([^<>]*)>\s*\(")
_NAMES = {"conv": "conv", "conv_stacked": "conv_stacked", "conv_s3": "s3", "conv_s3p": "s3p", "conv3x3_small": "small"}


def instantiations_in_the_dispatch():
    """Keys of every launch_conv*<...>(...) in the bodies of conv_dispatch, launch_conv_tw, conv_dispatch_s3 (conv_dispatch_h2, the
    two-piece part, is a function of its own), conv_dispatch_s3p and conv_layer (whose only launches are the head's), with
    launch_conv_tw's template parameters replaced by the arguments conv_dispatch instantiates it with."""
    def read(name):
        with open(os.path.join(ROOT, "v2e_amd", "csrc", name)) as f:
            return re.sub(r"//[^\n]*", "", f.read())
    conv_h, s3p_h, hip = read("slomo_conv.h"), read("slomo_s3p.h"), read("slomo.hip")

    def launches(src, signature):
        return [(name, [a.strip() for a in args.split(",")]) for name, args in _LAUNCH.findall(_function_body(src, signature))]
    tw_params = [p.split()[-1] for p in re.search(r"template\s*<([^<>]*)>\s*static void launch_conv_tw\(", conv_h).group(1).split(",")]
    tw_body = launches(conv_h, "static void launch_conv_tw(")
    found = []
    for name, args in (launches(conv_h, "static int conv_dispatch(") + launches(hip, "static int conv_dispatch_s3(")
                       + launches(s3p_h, "static int conv_dispatch_s3p(") + launches(hip, "static int conv_layer(")):
        if name == "conv_tw":
            bind = dict(zip(tw_params, args))
            found += [(n2, [bind.get(a, a) for a in a2]) for n2, a2 in tw_body]
        else:
            found.append((name, args))
    return {"%s<%s>" % (_NAMES[name], ",".join(args)) for name, args in found}


def test_tables_name_every_tile_the_dispatch_can_select():
    # every case sits under the key the model routes it to, and asks the oracle for no more than the cap
    for table, split in ((S3_TILES, True), (S3_FALLBACKS, True), (F32_TILES, False), (HEAD_TILES, False)):
        for key, case in _flat(table):
            assert model_conv_layer(case, split) == key, "%r is filed under %s" % (case, key)
            k, c0, c1, cout, n, h, w = case[:7]
            checked = WIDE_CHECKED if case_is_wide(case) else n
            assert checked * h * w * (c0 + c1) * cout * k * k <= ORACLE_MAC_CAP, "%r is too dear for the oracle" % (case,)
    # a fallback case is the f32 kernel with or without split weights; a tile case is not
    for key, case in _flat(S3_FALLBACKS):
        assert model_conv_layer(case, False) == key and key.startswith("conv")
    for key, case in _flat(S3_TILES):
        assert key.startswith("s3") and model_conv_layer(case, False).startswith("conv")
    # a wide case run in batches of 8 takes the CT = 1 instantiation of the same tile
    for key, case in _flat(F32_TILES):
        if case_is_wide(case):
            assert case[4] % 8 == 0 and not case_is_wide(case[:4] + (8,) + case[5:])
            want = re.sub(r"^(conv<\d,\d),2,", r"\1,1,", key)
            assert model_conv_layer(case[:4] + (8,) + case[5:], False) == want
    # the keys are the instantiations the dispatch source names, no more and no fewer
    keys = set(S3_TILES) | set(F32_TILES) | set(HEAD_TILES)
    in_source = instantiations_in_the_dispatch()
    assert keys == in_source, "no case for %s; no such tile: %s" % (sorted(in_source - keys), sorted(keys - in_source))
    assert set(S3_FALLBACKS) <= set(F32_TILES)


# ---------------------------------------------------------------- the GPU tests
def _oracle(oracle_lib, x0, x1, wt, b, pre):
    xin = oracle_lib.avgpool2(x0) if pre == 1 else (oracle_lib.upsample2(x0) if pre == 2 else x0)
    if x1 is not None:
        xin = np.concatenate((xin, x1), axis=1)
    return oracle_lib.conv2d_lrelu(xin, wt, b)


def _alone(layer, x0, x1, i, math, pre=0):
    return layer.run(x0[i:i + 1], None if x1 is None else x1[i:i + 1], math, pre)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kc", _flat(S3_TILES) + _flat(S3_FALLBACKS), ids=_id)
def test_three_piece_conv_layer(kc, oracle_lib):
    key, case = kc
    n = case[4]
    x0, x1, wt, b = _case_tensors(case)
    layer = _Layer(wt, b)
    y = layer.run(x0, x1, "bf16x3")          # guard bands and inputs are checked inside, at every launch
    y32 = layer.run(x0, x1, "f32")
    ref = _oracle(oracle_lib, x0, x1, wt, b, 0)
    assert not np.isnan(y).any(), "output not fully written (or a NaN from beyond the input was consumed)"
    e, e32 = relerr(y, ref), relerr(y32, ref)
    print("bf16x3 %s %s: relerr vs oracle %.3e (f32 kernel %.3e)" % (key, case, e, e32))
    assert e < TOL
    assert e32 < TOL
    if key.startswith("s3"):   # which kernel ran: a three-piece tile does not give the f32 kernel's bits, a fallback does
        assert not np.array_equal(y, y32)
    else:
        assert np.array_equal(y, y32)
    # the dispatch does not look at n and every output's accumulation chain is fixed: a sample of a batch is the sample run alone
    if n > 1:
        for i in range(n):
            assert np.array_equal(_alone(layer, x0, x1, i, "bf16x3"), y[i]), "sample %d of %d differs from the same sample run alone" % (i, n)
    # slomo_s3p.h: k_conv_s3p gives k_conv_s3's bits.  The pre-split entry runs k_conv_s3 (MODE 2: same pieces, same products,
    # same order as splitting while staging) on the same shape.
    if key.startswith("s3p") and x1 is None:
        assert np.array_equal(layer.run(x0, None, "bf16x3", pre=3), y), "k_conv_s3p and k_conv_s3 differ"


def _check_f32_case(key, case, oracle_lib):
    k, c0, c1, cout, n, h, w, pre = case
    x0, x1, wt, b = _case_tensors(case[:7], pre)
    layer = _Layer(wt, b)
    y = layer.run(x0, x1, "f32", pre)
    assert not np.isnan(y).any(), "output not fully written (or a NaN from beyond the input was consumed)"
    if not case_is_wide(case):
        e = relerr(y, _oracle(oracle_lib, x0, x1, wt, b, pre))
        print("f32 %s %s: relerr vs oracle %.3e" % (key, case, e))
        assert e < TOL
        if n > 1:   # a single sample selects the same instantiation (a stacked tile's second sample is then masked)
            for i in range(n):
                assert np.array_equal(_alone(layer, x0, x1, i, "f32", pre), y[i]), "sample %d of %d differs from the same sample run alone" % (i, n)
        return
    # wide: the oracle on the first and the last sample, an odd and an even one in between
    some = [0, n // 3 | 1, (2 * n // 3) & ~1, n - 1]
    e = relerr(y[some], _oracle(oracle_lib, x0[some], None, wt, b, pre))
    print("f32 %s %s: relerr vs oracle on samples %s %.3e" % (key, case, some, e))
    assert e < TOL
    # ... and every sample against the CT = 1 kernel, which batches of 8 select: equal bits (module docstring)
    for i in range(0, n, 8):
        assert np.array_equal(layer.run(x0[i:i + 8], None, "f32", pre), y[i:i + 8]), "samples %d..%d differ from the CT = 1 kernel's" % (i, i + 7)


@pytest.mark.gpu
@pytest.mark.parametrize("kc", _flat(F32_TILES), ids=_id)
def test_f32_conv_layer(kc, oracle_lib):
    _check_f32_case(kc[0], kc[1], oracle_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("kc", _flat(HEAD_TILES), ids=_id)
def test_head_conv_layer(kc, oracle_lib):
    _check_f32_case(kc[0], kc[1], oracle_lib)
