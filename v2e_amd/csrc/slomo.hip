// slomo.hip -- SuperSloMo frame interpolation (two UNets + backWarp + fusion) for gfx950.
//
// Reference (SensorsINI/v2e): v2ecore/model.py:10-226 (UNet/down/up), :229-300 (backWarp),
// v2ecore/slomo.py:338-345 (flow UNet), :404-433 (per-t blend, 4 warps, interp UNet, fusion).
//
// One translation unit: slomo_conv.h (the convolution arguments, the range slots, the f32 matrix-core kernel), slomo_tile.h (the
// steps the convolution kernels share beside their multiplies: tile decode, concat source, staging plan, epilogue, grid), slomo_s3.h
// and slomo_s3p.h (the split-operand kernels), slomo_stream.h (pooling, upsampling, prep, fuse and the other streaming kernels); here
// the tile selection of the split-operand kernels, one layer, the UNet pass and the C entry points.
#include "common.h"
#include <cstdlib>

namespace {

// where the two-float16-piece convolutions report an activation beyond float16's range (v2e_conv_set_range_flag), or nullptr
static thread_local int *g_conv_range_flag = nullptr;

#include "slomo_conv.h"
#include "slomo_s3.h"
#include "slomo_s3p.h"
#include "slomo_stream.h"

// ---------------------------------------------------------------- tile selection of the split-operand kernels
// The first tile whose shape condition holds is launched; 1 = none fits (the caller falls back to the f32-MFMA kernel).  What the
// rejected alternatives measured is in DESIGN.md section 7.

// pre-split input (pre == 3): 3x3 layers only (dev: measured against in-kernel splitting by scripts/conv_s3_check)
static int conv_dispatch_s3_presplit(const ConvArgs &a, int ks, hipStream_t s, LayerCtx &ctx)
{
    if (ks != 3) return 1;
    if (a.w_ % 32 == 0) return launch_conv_s3<3, 1, 2, 4, 32, 1, 2>(a, s, ctx);
    if (a.w_ % 16 == 0) return launch_conv_s3<3, 1, 2, 4, 16, 1, 2>(a, s, ctx);
    if (a.w_ % 8 == 0) return launch_conv_s3<3, 1, 2, 4, 8, 1, 2>(a, s, ctx);
    return 1;
}

// two float16 pieces, three products (conv_math "fp16x2"): half the multiplies of the three-piece math, so the matrix pipe is far
// from the rate at which four accumulator chains x two waves per SIMD are slow (slomo_s3p.h) and every tile keeps two workgroups per CU
static int conv_dispatch_h2(const ConvArgs &a, int ks, hipStream_t s, LayerCtx &ctx)
{
    if (ks == 3) {
        if (a.cout % 64 == 0) {
            // 64 x 64 register tiles, one kernel row of weights resident (34 KB of LDS): a third fewer LDS operand bytes per multiply
            // than the 32 x 64 tile, bit-identical output; the 32 x 64 tile here lost 4 % per forward, 64 x 128 tiles 3-5 %
            if (a.w_ % 32 == 0) return launch_conv_s3<3, 2, 2, 4, 32, 1, 0, 1, 2>(a, s, ctx);
            if (a.w_ % 16 == 0) return launch_conv_s3<3, 2, 2, 4, 16, 1, 0, 1, 2>(a, s, ctx);
            if (a.w_ % 8 == 0) return launch_conv_s3<3, 2, 2, 4, 8, 1, 0, 1, 2>(a, s, ctx);
            // (64 channels on the 20-wide five-wave tiles lost 2.5 % per forward: those levels take the 32-channel tiles below)
        }
        // 32 channels x 128 pixels per wave, one kernel row of weights resident (up5.*: 64 -> 32 at full resolution): a weight operand
        // read feeds four multiplies; the 32 x 64 tile lost 9 % per layer, all weights resident with this tile lost to both
        if (a.w_ % 32 == 0 && a.h % 16 == 0) return launch_conv_s3<3, 1, 4, 4, 32, 1, 0, 1, 2>(a, s, ctx);
        if (a.w_ % 32 == 0) return launch_conv_s3<3, 1, 2, 4, 32, 1, 0, 0, 2>(a, s, ctx);
        if (a.w_ % 16 == 0) return launch_conv_s3<3, 1, 2, 4, 16, 1, 0, 0, 2>(a, s, ctx);
        if (a.w_ % 8 == 0) return launch_conv_s3<3, 1, 2, 4, 8, 1, 0, 0, 2>(a, s, ctx);
        // the 16 x 20 level of a 320 x 256 input: one whole sample per five-wave workgroup, two pixel tiles per wave (8 x 20 tiles lost
        // 1.3 % per forward, 64 output channels on top of this tile 2 %)
        if (a.w_ % 20 == 0 && a.h % 16 == 0) return launch_conv_s3<3, 1, 2, 5, 20, 1, 0, 0, 2>(a, s, ctx);
        if (a.w_ % 20 == 0 && a.h % 8 == 0) return launch_conv_s3<3, 1, 1, 5, 20, 1, 0, 0, 2>(a, s, ctx);
        if (a.w_ == 10 && a.h <= 16) return launch_conv_s3<3, 1, 1, 5, 10, 1, 0, 0, 2>(a, s, ctx); // the 8 x 10 level: half of a 16-row tile masked
        return 1;
    }
    if (ks == 5 && a.w_ % 32 == 0) {
        if (a.cout % 64 == 0) return launch_conv_s3<5, 2, 2, 4, 32, 1, 0, 1, 2>(a, s, ctx); // 64 x 64 tiles: the 32 x 64 tile lost 1.5 %
        return launch_conv_s3<5, 1, 2, 4, 32, 1, 0, 0, 2>(a, s, ctx);
    }
    if (ks == 7 && a.w_ % 32 == 0) return a.cin % 16 == 0 ? launch_conv_s3<7, 1, 2, 4, 32, 1, 0, 0, 2>(a, s, ctx) : launch_conv_s3<7, 1, 2, 4, 32, 1, 1, 0, 2>(a, s, ctx);
    return 1;
}

// three bf16 pieces, six products (conv_math "bf16x3"): 32-channel tiles (60 KB of LDS: two workgroups per CU, so one stages while
// the other multiplies); 64-channel tiles lost 15 % at every level (16 samples: 3x3 143-174 vs 121-153 TF/s, 5x5 172-183 vs 146-160)
static int conv_dispatch_s3(const ConvArgs &a, int ks, hipStream_t s, LayerCtx &ctx)
{
    if (a.np == 2) return conv_dispatch_h2(a, ks, s, ctx);
    if (ks == 3) {
        // the software-pipelined one-wave-per-SIMD kernel where the layer has one of its shapes (slomo_s3p.h: bit-identical output,
        // 3-6 % less time per layer than the tiles below, 1.5 % per forward)
        if (conv_dispatch_s3p(a, ks, s) == 0) return 0;
        if (a.w_ % 32 == 0) return launch_conv_s3<3, 1, 2, 4, 32>(a, s, ctx);
        if (a.w_ % 16 == 0) return launch_conv_s3<3, 1, 2, 4, 16>(a, s, ctx);
        if (a.w_ % 8 == 0) return launch_conv_s3<3, 1, 2, 4, 8>(a, s, ctx);
        // (the 16 x 20 tile of the two-piece math lost 2 % per forward here: 26.4 -> 27.0 ms)
        if (a.w_ % 20 == 0 && a.h % 8 == 0) return launch_conv_s3<3, 1, 1, 5, 20>(a, s, ctx);
        // the 8 x 10 level: a 16 x 10 tile with its lower half masked is still 1.5x the f32 matrix-core kernel's two stacked samples
        if (a.w_ == 10 && a.h <= 16) return launch_conv_s3<3, 1, 1, 5, 10>(a, s, ctx);
        return 1;
    }
    if (ks == 5 && a.w_ % 32 == 0) return launch_conv_s3<5, 1, 2, 4, 32>(a, s, ctx);
    if (ks == 7 && a.w_ % 32 == 0) return a.cin % 16 == 0 ? launch_conv_s3<7, 1, 2, 4, 32>(a, s, ctx) : launch_conv_s3<7, 1, 2, 4, 32, 1, 1>(a, s, ctx);
    return 1;
}

// ---------------------------------------------------------------- one layer
// y = leaky_relu(conv(pre(x0) ++ x1), 0.1): what v2e_conv2d_lrelu documents (include/v2e_amd.h), with the context of a UNet pass.
// pre == 3 (x0 pre-split by v2e_split3_nchw) writes its output slot and reads no input slots; the VALU kernel of the 4- / 5-channel
// head writes no slot.
static int conv_layer(const float *x0, int c0, const float *x1, int c1, int pre, const v2e_conv_desc *conv, float *y, int n, int h,
                      int w, hipStream_t s, LayerCtx &ctx)
{
    V2E_REQUIRE(x0 && conv && conv->weight && conv->bias && y, "null conv arg");
    V2E_REQUIRE(c0 + c1 == conv->cin && (c1 == 0 || x1), "channel split does not match the layer");
    V2E_REQUIRE(pre == 0 || c1 == 0, "fused pool/upsample takes a single source");
    const int ks = conv->ksize, cin = conv->cin, cout = conv->cout;
    if (pre == 3) {
        V2E_REQUIRE(conv->weight_s3 && cin % 16 == 0 && cout % 32 == 0, "pre-split input needs split weights, cin % 16 == 0, cout % 32 == 0");
        V2E_REQUIRE((conv->split_kind & 0xFF) != 2, "pre-split input is three bf16 pieces");
    } else {
        V2E_REQUIRE(pre != 2 || (h % 2 == 0 && w % 2 == 0), "upsample target must be even");
        V2E_REQUIRE(cin % 2 == 0, "cin must be even");
        V2E_REQUIRE(c1 == 0 || c0 % 8 == 0, "first concat source must be a multiple of 8 channels");
        V2E_REQUIRE(h < 4096 && w < 4096, "image too large for the staging plan");
        V2E_REQUIRE((ks == 3 && cin % 8 == 0) || (ks == 5 && cin % 4 == 0) || (ks == 7 && cin % 2 == 0),
                    "cin must be a multiple of the channel chunk (8 for 3x3, 4 for 5x5, 2 for 7x7)");
    }
    ConvArgs a = {}; // (tiles_x, tiles_y, ncb, tl_on and ypool are the launchers')
    a.x0 = x0; a.c0 = c0;
    a.w = conv->weight; a.bias = conv->bias; a.y = y;
    a.n = n; a.h = h; a.w_ = w; a.cin = cin; a.cout = cout;
    a.ws3 = conv->weight_s3;
    a.am_out = ctx.am_out;
    if (pre == 3) {
        a.xs_plane = (long long)n * (c0 / 8) * h * w; a.np = 3; a.out_scale = 1.0f;
        V2E_REQUIRE(conv_dispatch_s3_presplit(a, ks, s, ctx) == 0, "no pre-split tile for this layer shape");
    } else if (ks == 3 && pre == 0 && c1 == 0 && (cout == 4 || cout == 5)) {
        if (cout == 4) launch_conv3x3_small<4>(x0, conv->weight, conv->bias, y, n, cin, h, w, s);
        else launch_conv3x3_small<5>(x0, conv->weight, conv->bias, y, n, cin, h, w, s);
    } else {
        a.x1 = x1; a.c1 = c1;
        a.np = (conv->split_kind & 0xFF) == 2 ? 2 : 3;
        a.out_scale = ldexpf(1.0f, -(conv->split_kind >> 8));
        a.ovf = g_conv_range_flag;
        a.am_in0 = ctx.am_in0; a.am_in1 = ctx.am_in1;
        // split-operand kernel: whole 16-channel chunks -- or the 12-channel 7x7 conv1, whose last chunk is padded with zeros
        // (a third of its multiplies wasted and still 1.4x the f32 kernel; the 2-channel conv1 of the flow UNet is not worth it)
        const bool s3_cin = cin % 16 == 0 || (ks == 7 && c1 == 0 && cin >= 8);
        int r3 = 1; // 1: no split-operand tile takes this layer
        if (a.ws3 && pre == 0 && s3_cin && cout % 32 == 0 && (c1 == 0 || c0 % 16 == 0)) r3 = conv_dispatch_s3(a, ks, s, ctx);
        if (r3 != 0 && r3 != 1) return r3;
        if (r3 == 1 && conv_dispatch(a, ks, pre, s)) { v2e_set_error("unsupported conv: k=%d pre=%d", ks, pre); return V2E_EINVAL; }
    }
    V2E_HIP(hipGetLastError());
    return 0;
}

} // namespace

extern "C" {

// dev tool (not part of the public header; scripts/conv_s3_check): switch k_conv_s3p's per-step timeline of workgroup 0 on
// (out == NULL) or read it back: pairs (shader clock, 100 MHz wall clock), terminated by a zero
int v2e_slomo_debug_s3p_timeline(unsigned long long *out, int n_pairs)
{
    if (!out) {
        g_s3p_timeline_on = 1;
        return 0;
    }
    V2E_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_s3p_timeline), sizeof(unsigned long long) * 2 * (size_t)(n_pairs < 512 ? n_pairs : 512)));
    return 0;
}

int v2e_pack_conv_weight_s3(const float *w_oihw, void *w_s3, int cout, int cin, int k, void *stream)
{
    V2E_REQUIRE(w_oihw && w_s3 && cout > 0 && cin > 0 && k > 0, "bad pack args");
    const size_t total = (size_t)((cin + 15) / 16) * 2 * k * k * cout; // [ceil(cin/16)][k*k][3][2][cout] 16-byte units / 3
    k_pack_weight_s3<3><<<v2e_cdiv((int64_t)total, 256), 256, 0, (hipStream_t)stream>>>(w_oihw, (uint4 *)w_s3, cout, cin, k * k);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_conv_set_range_flag(int *device_flag)
{
    g_conv_range_flag = device_flag;
    return 0;
}

int v2e_pack_conv_weight_h2(const float *w_oihw, void *w_h2, int cout, int cin, int k, int scale_log2, void *stream)
{
    V2E_REQUIRE(w_oihw && w_h2 && cout > 0 && cin > 0 && k > 0 && scale_log2 >= 0 && scale_log2 <= 60, "bad pack args");
    const size_t total = (size_t)((cin + 15) / 16) * 2 * k * k * cout; // one thread per (chunk, tap, channel group, cout): NP units
    k_pack_weight_s3<2><<<v2e_cdiv((int64_t)total, 256), 256, 0, (hipStream_t)stream>>>(w_oihw, (uint4 *)w_h2, cout, cin, k * k,
                                                                                        ldexpf(1.0f, scale_log2));
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_split3_nchw(const float *x, void *xs, int n, int c, int h, int w, void *stream)
{
    V2E_REQUIRE(x && xs && n > 0 && c > 0 && c % 8 == 0 && h > 0 && w > 0, "bad split args (channels must be a multiple of 8)");
    const long long nc8 = (long long)n * (c / 8);
    k_split3_nchw<<<v2e_cdiv(nc8 * h * w, 256), 256, 0, (hipStream_t)stream>>>(x, (uint4 *)xs, nc8, h * w);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_pack_conv_weight(const float *w_oihw, float *w_packed, int cout, int cin, int k, void *stream)
{
    V2E_REQUIRE(w_oihw && w_packed && cout > 0 && cin > 0 && k > 0, "bad pack args");
    launch_pack_weight(w_oihw, w_packed, cout, cin, k * k, (hipStream_t)stream);
    V2E_HIP(hipGetLastError());
    return 0;
}

// (the argument checks are conv_layer's: a UNet pass makes the same ones for every layer)
int v2e_conv2d_lrelu(const float *x0, int c0, const float *x1, int c1, int pre, const v2e_conv_desc *conv, float *y,
                     int n, int h, int w, void *stream)
{
    LayerCtx none; // outside a pass: no range slots, no pooled copy
    return conv_layer(x0, c0, x1, c1, pre, conv, y, n, h, w, (hipStream_t)stream, none);
}

// workspace layout (floats): s1 s2 s3 s4 s5 | tA tB tU | range slots   (model.py:198-226)
int64_t v2e_unet_workspace_bytes(int n, int h, int w, int cin)
{
    const int64_t hw = (int64_t)h * w;
    // s1 32hw, s2 16hw, s3 8hw, s4 4hw, s5 2hw, two temporaries of 32hw, one of 64hw for the
    // pooled / upsampled input of the first conv of each down / up block
    // + the range slots of the forward pass (32 words: the input's and every convolution's largest |output|)
    return (int64_t)n * hw * (32 + 16 + 8 + 4 + 2 + 32 + 32 + 64) * (int64_t)sizeof(float) + 256;
}

int v2e_unet_forward(const float *x, int cin, const v2e_conv_desc *cv, int cout, float *y, int n, int h, int w,
                     void *workspace, void *stream)
{
    V2E_REQUIRE(x && cv && y && workspace, "null unet arg");
    V2E_REQUIRE(h % 32 == 0 && w % 32 == 0, "UNet input must be a multiple of 32 (dataloader.py:122-123)");
    V2E_REQUIRE(cv[0].cin == cin && cv[22].cout == cout, "descriptor list does not match cin/cout");
    const int64_t hw = (int64_t)h * w;
    float *ws = (float *)workspace;
    float *s1 = ws; float *s2 = s1 + n * hw * 32; float *s3 = s2 + n * hw * 16; float *s4 = s3 + n * hw * 8;
    float *s5 = s4 + n * hw * 4; float *tA = s5 + n * hw * 2; float *tB = tA + n * hw * 32; float *tU = tB + n * hw * 32;
    float *const skip[5] = {s1, s2, s3, s4, s5};
    hipStream_t st = (hipStream_t)stream;
    // range slots: am[0] = the input, am[1 + i] = the output of convolution i.  Tracked only when some layer runs on two
    // float16 pieces (it is what their operand scaling reads).
    uint32_t *am = (uint32_t *)(tU + n * hw * 64);
    bool track = false;
    for (int i = 0; i < 23; ++i) track = track || ((cv[i].split_kind & 0xFF) == 2 && cv[i].weight_s3);
    if (track) {
        launch_zero_u32(am, 32, st);
        launch_amax(x, (long long)n * cin * hw, am, st);
    }
    // V2E_AMD_FUSE_POOL=1: the pooled copy of a skip tensor comes out of the producing convolution's epilogue where its tile allows
    // (the two largest of the five poolings: 0.28 of the 0.33 ms the pooling passes take at 80 samples).  Built and bit-identical
    // (tests/test_slomo_gpu.py), measured round 4, A/B x 3 at 80 samples: 17.83 ms fused against 17.80 ms with the separate
    // passes (bf16x3: 26.30 both) -- the convolutions are at the chip's power limit, and what the epilogue adds costs what the
    // streaming pass did.  Off by default.
    static const int fuse_pool = getenv("V2E_AMD_FUSE_POOL") ? atoi(getenv("V2E_AMD_FUSE_POOL")) : 0;
    static const int fuse_up = getenv("V2E_AMD_FUSE_UP") ? atoi(getenv("V2E_AMD_FUSE_UP")) : 0; // dev: bit u-1 = fuse the bilinear x2 of up<u> into its conv loader

    // an activation of the pass: where it is, its channels, and the range slot of the convolution behind it (0: the network input).
    // avg_pool2d and the bilinear x2 cannot exceed their input's maximum, so what they return keeps their input's slot.
    struct Act { const float *p; int c, slot; };
    const Act none = {nullptr, 0, 0};
    int rc = 0; // the first failure: nothing is launched after it
    // convolution i (UNET_LAYERS order) of x0 ++ x1 into out[n][co][hh][ww]; pool_out / pooled: LayerCtx
    const auto conv = [&](int i, Act x0, Act x1, int pre, float *out, int co, int hh, int ww, float *pool_out = nullptr, bool *pooled = nullptr) {
        LayerCtx ctx;
        if (track) { ctx.am_in0 = am + x0.slot; ctx.am_in1 = x1.p ? am + x1.slot : nullptr; ctx.am_out = am + 1 + i; }
        ctx.pool_out = pool_out;
        if (!rc) rc = conv_layer(x0.p, x0.c, x1.p, x1.c, pre, &cv[i], out, n, hh, ww, st, ctx);
        if (pooled) *pooled = ctx.pooled;
        return Act{out, co, 1 + i};
    };
    // producer ops as their own streaming passes into tU[n][c][hh][ww]: measured faster than fusing them into the conv
    // loader (the fused bilinear fetch costs 4 gathers + address math per staged element)
    const auto pool = [&](Act a, int hh, int ww) {
        if (!rc) launch_avgpool2(a.p, tU, (long long)n * a.c, hh, ww, st);
        return Act{tU, a.c, a.slot};
    };
    const auto upsample = [&](Act a, int hh, int ww) {
        if (!rc) launch_upsample2(a.p, tU, (long long)n * a.c, hh, ww, st);
        return Act{tU, a.c, a.slot};
    };

    // conv1 + conv2, down1 .. down4: two convolutions, the second into skip tensor s<d+1>, whose avg_pool2d(2) feeds the next block
    Act cur = {x, cin, 0}, skips[5];
    for (int d = 0; d < 5; ++d) {
        const int co = 32 << d, hh = h >> d, ww = w >> d;
        cur = conv(2 * d, cur, none, 0, tA, co, hh, ww);
        bool pooled = false;
        skips[d] = conv(2 * d + 1, cur, none, 0, skip[d], co, hh, ww, fuse_pool && d < 2 ? tU : nullptr, &pooled);
        cur = pooled ? Act{tU, co, skips[d].slot} : pool(skips[d], hh / 2, ww / 2);
    }
    // down5
    cur = conv(10, cur, none, 0, tA, 512, h / 32, w / 32);
    cur = conv(11, cur, none, 0, tB, 512, h / 32, w / 32);
    // up1 .. up5: bilinear x2, conv1; conv2 with the skip concat fused (x first, skip second)
    for (int u = 1; u <= 5; ++u) {
        const int co = 512 >> (u - 1), hh = h >> (5 - u), ww = w >> (5 - u);
        if (fuse_up & (1 << (u - 1))) cur = conv(10 + 2 * u, cur, none, 2, tA, co, hh, ww);
        else cur = conv(10 + 2 * u, upsample(cur, hh, ww), none, 0, tA, co, hh, ww);
        cur = conv(11 + 2 * u, cur, skips[5 - u], 0, tB, co, hh, ww);
    }
    // conv3 (+ leaky relu, model.py:225)
    conv(22, cur, none, 0, y, cout, h, w);
    return rc;
}

int v2e_slomo_prep(const float *i0, const float *i1, const float *flow, const float *tcoef, int n_t, int b, int h, int w,
                   float *x12, void *stream)
{
    V2E_REQUIRE(i0 && i1 && flow && tcoef && x12 && n_t > 0 && b > 0 && h > 0 && w > 0, "bad prep args");
    V2E_REQUIRE((long long)n_t * b <= 65535, "too many samples for one prep launch");
    return launch_per_pixel(k_prep, n_t * b, h, w, (hipStream_t)stream, i0, i1, flow, tcoef, n_t, b, h, w, x12);
}

int v2e_slomo_fuse(const float *i0, const float *i1, const float *x12, const float *intrp, const float *tcoef, int n_t,
                   int b, int h, int w, float *out, void *stream)
{
    V2E_REQUIRE(i0 && i1 && x12 && intrp && tcoef && out && n_t > 0 && b > 0 && h > 0 && w > 0, "bad fuse args");
    V2E_REQUIRE((long long)n_t * b <= 65535, "too many samples for one fuse launch");
    return launch_per_pixel(k_fuse, n_t * b, h, w, (hipStream_t)stream, i0, i1, x12, intrp, tcoef, n_t, b, h, w, out);
}

int v2e_slomo_max_speed2(const float *flow, int b, int h, int w, uint32_t *out_bits, void *stream)
{
    V2E_REQUIRE(flow && out_bits && b > 0 && h > 0 && w > 0, "bad max_speed args");
    return launch_max_speed2(k_max_speed2, (long long)b * h * w, 1, out_bits, (hipStream_t)stream, flow, b, h * w, out_bits);
}

int v2e_slomo_max_speed2_seg(const float *flow, int b, int seg, int h, int w, uint32_t *out_bits, void *stream)
{
    V2E_REQUIRE(flow && out_bits && b > 0 && seg > 0 && h > 0 && w > 0, "bad max_speed_seg args");
    const int nseg = v2e_cdiv(b, seg);
    V2E_REQUIRE(nseg <= 65535, "too many batches for one max_speed_seg launch");
    return launch_max_speed2(k_max_speed2_seg, (long long)seg * h * w, nseg, out_bits, (hipStream_t)stream, flow, b, seg, h * w, out_bits);
}

int v2e_slomo_prep_tab(const float *i0, const float *i1, const float *flow, const float *tcoef, const int32_t *tab, int n,
                       int h, int w, float *x12, void *stream)
{
    V2E_REQUIRE(i0 && i1 && flow && tcoef && tab && x12 && n > 0 && n <= 65535 && h > 0 && w > 0, "bad prep_tab args");
    return launch_per_pixel(k_prep_tab, n, h, w, (hipStream_t)stream, i0, i1, flow, tcoef, tab, h, w, x12);
}

int v2e_slomo_fuse_tab(const float *i0, const float *i1, const float *x12, const float *intrp, const float *tcoef,
                       const int32_t *tab, int n, int h, int w, float *out, void *stream)
{
    V2E_REQUIRE(i0 && i1 && x12 && intrp && tcoef && tab && out && n > 0 && n <= 65535 && h > 0 && w > 0, "bad fuse_tab args");
    return launch_per_pixel(k_fuse_tab, n, h, w, (hipStream_t)stream, i0, i1, x12, intrp, tcoef, tab, h, w, out);
}

// diagnostics (include/v2e_amd.h): the streaming passes of a UNet forward on their own, through the launchers the pass uses
int v2e_slomo_stream_eval(int op, const float *x, void *y, int64_t nc, int h, int w, void *stream)
{
    V2E_REQUIRE(x && y && nc > 0 && h > 0 && w > 0, "bad stream_eval args");
    V2E_REQUIRE(op >= V2E_SS_AVGPOOL2 && op <= V2E_SS_AMAX, "unknown stream_eval op");
    const bool up = op == V2E_SS_UPSAMPLE2 || op == V2E_SS_UPSAMPLE2_SCALAR;
    V2E_REQUIRE(!up || (h % 2 == 0 && w % 2 == 0), "upsample target must be even");
    V2E_REQUIRE(nc * h * w < ((int64_t)1 << 38), "stream_eval tensor too large");
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)nc * h * w;
    switch (op) {
    case V2E_SS_AVGPOOL2: launch_avgpool2(x, (float *)y, nc, h, w, s); break;
    case V2E_SS_AVGPOOL2_SCALAR: k_avgpool2_scalar<<<v2e_cdiv(total, 256), 256, 0, s>>>(x, (float *)y, nc, h, w); break;
    case V2E_SS_UPSAMPLE2: launch_upsample2(x, (float *)y, nc, h, w, s); break;
    case V2E_SS_UPSAMPLE2_SCALAR: k_upsample2_scalar<<<v2e_cdiv(total, 256), 256, 0, s>>>(x, (float *)y, nc, h, w); break;
    default: launch_amax(x, total, (uint32_t *)y, s); break;
    }
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
