// slomo_conv.h -- the convolution arguments every UNet kernel takes, the activation range slots, and the f32 matrix-core kernel
// with its tile selection (included by slomo.hip).
//
// Convolutions are implicit GEMMs on the exact-f32 matrix cores:
//   D[co][pixel] += W[co][k] * X[k][pixel],  k = (ci, ky, kx)
// with v_mfma_f32_32x32x2_f32 (A = 32 output channels x 2 k, B = 2 k x 32 pixels).  The pixel
// axis is the MFMA column axis, so every accumulator register is 32 consecutive x of one
// output channel: NCHW stores are 128-byte coalesced.  The f32 MFMA is bit-identical to an
// fmaf chain in k order, and the k order here is fixed (ci-chunk, ky, kx, ci-pair), so results
// are deterministic run to run; parity with torch-CPU (different summation order) is checked
// at 1e-5 * max(1,|y|).
//
// Per workgroup: WP waves; each wave owns CT x PT tiles of 32 channels x 32 pixels.  Per
// ci-chunk the input patch (with halo, zero padding, and optionally the preceding
// avg_pool2d / bilinear x2 upsample / channel concat applied on the fly) and the weight
// slice are staged in LDS; both operand reads are then `lane base + immediate` ds_read_b32
// over 32 consecutive dwords per half-wave (conflict-free).
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
    const float *x0, *x1; // x1: second concat source or nullptr
    int c0, c1;           // channels of x0 / x1
    const float *w;       // packed [Cin][KS][KS][Cout]
    const float *bias;
    float *y;
    int n, h, w_, cin, cout;
    int tiles_x, tiles_y;
    const void *ws3; // split-bf16 weights (slomo_s3.h) or nullptr
    int ncb;         // slomo_s3.h: channel blocks when the grid is 1-D in XCD order, else 0
    long long xs_plane; // slomo_s3.h, pre-split input: 16-byte units per piece plane (n * C/8 * h * w)
    int tl_on;          // slomo_s3p.h, dev: record workgroup 0's per-step timeline
    int np;             // pieces the split weights ws3 hold: 3 (bf16) or 2 (float16)
    float out_scale;    // np == 2: 2^-s, the inverse of the power of two the weights were packed times
    int *ovf;           // np == 2: device flag set when an activation is beyond float16's range (or NaN), or nullptr
    // Activation range tracking (v2e_unet_forward): every convolution leaves the largest |output| it wrote in *am_out (float32
    // bits: non-negative floats, inf and NaN order like their bit patterns; atomicMax per wave), and a two-float16-piece
    // convolution reads the maxima of its input's producer(s) and stages its activations times the power of two that puts that
    // maximum in [2^13, 2^14): no piece of an activation that matters falls into float16's subnormals however small the
    // layer's activations are, nothing overflows however large; the epilogue divides the power out again (exact).
    const uint32_t *am_in0, *am_in1;
    uint32_t *am_out;
    // avg_pool2d(2) of the output, written beside it by the epilogue ([n][cout][h/2][w/2]; k_conv_s3 tiles of 32-pixel rows, two
    // rows per wave: the 2 x 2 window is two registers of a lane and its neighbour lane), or nullptr
    float *ypool;
};

// What v2e_unet_forward hands a layer beside its tensors (host side; empty outside a pass): the range slots of the producers of
// x0 / x1, the layer's own slot, and where avg_pool2d(2) of the output is wanted too.  The launcher whose tile can write that
// pooled copy says so in `pooled`; where it stays false the pass pools in a launch of its own.
struct LayerCtx {
    const uint32_t *am_in0 = nullptr, *am_in1 = nullptr;
    uint32_t *am_out = nullptr;
    float *pool_out = nullptr;
    bool pooled = false;
};

// |v| folded into a running maximum kept as float32 bits: one v_max_f32 with the |.| source modifier.  Non-negative floats and
// +inf order like their bit patterns, so the per-wave / per-slot reductions are integer maxima.  A NaN is ignored by the
// maximum: a NaN activation gives a NaN result in every conv math alike (as in the reference); what the range guard needs to
// see in a convolution's output is inf, and it does.  (A NaN of the network input itself is recorded by k_amax's own fold,
// slomo_stream.h.)
__device__ __forceinline__ void amax_fold(uint32_t &m, float v)
{
    m = __float_as_uint(fmaxf(__uint_as_float(m), fabsf(v)));
}
// one atomicMax per wave AT MOST: a layer is tens of thousands of workgroups and an atomic to one address is serialised where
// it is performed (measured: +1.3 ms per forward pass, 8 %, with an unconditional atomic per wave), so the wave first reads
// the slot -- a plain load; a stale (smaller) value only costs an atomic that was not needed, never a wrong maximum -- and
// only a wave that would raise it goes to the atomic unit: a few hundred per layer instead of 100 000
__device__ __forceinline__ void amax_commit(uint32_t *slot, uint32_t m)
{
    // wave maximum on the VALU data-parallel-primitive path (no LDS crossbar round trips at the tail of every wave)
#define V2E_S_DPP(v, ctrl) __builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xf, 0xf, true)
    m = max(m, (uint32_t)V2E_S_DPP(m, 0xB1));  // quad_perm [1,0,3,2]   (bit patterns of non-negative floats: all below 2^31)
    m = max(m, (uint32_t)V2E_S_DPP(m, 0x4E));  // quad_perm [2,3,0,1]
    m = max(m, (uint32_t)V2E_S_DPP(m, 0x141)); // row_half_mirror
    m = max(m, (uint32_t)V2E_S_DPP(m, 0x140)); // row_mirror
#undef V2E_S_DPP
    const uint32_t w = max(max((uint32_t)__builtin_amdgcn_readlane((int)m, 0), (uint32_t)__builtin_amdgcn_readlane((int)m, 16)),
                           max((uint32_t)__builtin_amdgcn_readlane((int)m, 32), (uint32_t)__builtin_amdgcn_readlane((int)m, 48)));
    if ((threadIdx.x & 63) == 0 && w != 0u) {
        if (w > *(volatile uint32_t *)slot) atomicMax(slot, w);
    }
}
// the power of two a two-float16-piece convolution stages its activations times: in_scale = 2^k with amax * 2^k in [2^13, 2^14),
// inv = 2^-k (both normal float32 numbers: |k| <= 126); bad = the producer wrote an inf or a NaN
__device__ __forceinline__ void act_scale(const ConvArgs &a, float &in_scale, float &inv, bool &bad)
{
    in_scale = 1.0f; inv = 1.0f; bad = false;
    if (!a.am_in0) return;
    uint32_t m = *a.am_in0;
    if (a.am_in1) { const uint32_t m1 = *a.am_in1; m = m1 > m ? m1 : m; }
    const int e = (int)(m >> 23); // biased exponent of the maximum (sign bit is clear)
    if (e == 255) { bad = true; return; }
    if (m == 0u) return; // an all-zero input
    int k = 140 - e;     // amax in [2^(e-127), 2^(e-126)) -> [2^13, 2^14)
    // ... as far as 2^-k times the weights' 2^-s (a.out_scale) stays a normal float32, so that the epilogue divides both out
    // with ONE exact multiply: s <= 40, i.e. maxima down to 2^-73 are scaled all the way
    const int sl2 = 127 - (int)((__float_as_uint(a.out_scale) >> 23) & 0xFF);
    const int kmax = 126 - (sl2 > 0 ? sl2 : 0);
    k = k > kmax ? kmax : (k < -126 ? -126 : k);
    in_scale = __uint_as_float((uint32_t)(127 + k) << 23);
    inv = __uint_as_float((uint32_t)(127 - k) << 23);
}

#include "slomo_tile.h"

// element fetch with the producer op fused: PRE 0 plain, 1 avg_pool2d(2) of a [2H][2W] source,
// 2 bilinear x2 upsample (align_corners=False) of a [H/2][W/2] source.
template <int PRE>
__device__ __forceinline__ float fetch(const ConvArgs &a, int n, int c, int gy, int gx)
{
    if (PRE == 0) {
        return concat_chunk(a, c, n, a.h * a.w_)[gy * a.w_ + gx];
    } else if (PRE == 1) { // F.avg_pool2d(x, 2): (((a+b)+c)+d) / 4
        const int sw = 2 * a.w_;
        const float *p = concat_chunk(a, c, n, 2 * a.h * sw) + 2 * gy * sw + 2 * gx;
        return (((p[0] + p[1]) + p[sw]) + p[sw + 1]) * 0.25f;
    } else { // F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)
        const int sh = a.h >> 1, sw = a.w_ >> 1;
        float ry = ((float)gy + 0.5f) * 0.5f - 0.5f;
        float rx = ((float)gx + 0.5f) * 0.5f - 0.5f;
        ry = ry < 0.f ? 0.f : ry;
        rx = rx < 0.f ? 0.f : rx;
        const int y0 = (int)ry, x0 = (int)rx;
        const int y1 = y0 + (y0 < sh - 1 ? 1 : 0), x1 = x0 + (x0 < sw - 1 ? 1 : 0);
        const float ly = ry - (float)y0, lx = rx - (float)x0;
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float *p = concat_chunk(a, c, n, sh * sw);
        return hy * (hx * p[y0 * sw + x0] + lx * p[y0 * sw + x1]) + ly * (hx * p[y1 * sw + x0] + lx * p[y1 * sw + x1]);
    }
}

// STK = 2: the tile is two whole samples stacked (levels whose sample is half a tile, 8x10 of a 320x256 input);
// in the LDS patch the two share ONE zero row between them: [0][A rows][0][B rows][0].
template <int KS, int CI_T, int CT, int PT, int WP, int TW, int PRE, int STK = 1>
__global__ __launch_bounds__(WP * 64) void k_conv(ConvArgs a)
{
    constexpr int NT = WP * 64;
    constexpr int PAD = KS / 2;
    constexpr int NPX = WP * PT * 32;
    constexpr int TH = NPX / TW;
    constexpr int THS = TH / STK; // rows per sample
    constexpr int PH = TH + KS - 1 + (STK - 1), PW = TW + KS - 1;
    static_assert(STK == 1 || (STK == 2 && KS == 3 && PRE == 0 && TH % 2 == 0), "stacked tiles: 3x3, plain fetch");
    constexpr int COT = CT * 32;
    constexpr int KK = KS * KS;
    constexpr int PATCH = CI_T * PH * PW;
    constexpr int PATCH_PAD = (PATCH + 3) / 4 * 4; // keeps the weight slice 16-byte aligned in LDS
    constexpr int WTS = CI_T * KK * COT;
    constexpr int NPE = (PATCH + NT - 1) / NT;     // patch elements staged per thread
    constexpr int NWE = (WTS / 4 + NT - 1) / NT;   // weight float4s staged per thread
    static_assert(NPX % TW == 0, "tile");
    static_assert(CI_T % 2 == 0, "ci pairs");
    __shared__ __attribute__((aligned(16))) float smem[PATCH_PAD + WTS];
    float *sp = smem, *sw = smem + PATCH_PAD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hsel = lane >> 5, l31 = lane & 31;
    ConvTile tile; // (the grid is 2-D: no padding workgroups)
    conv_tile<TH, TW, COT, STK>(a, tile);
    const int n = tile.n, oy0 = tile.oy0, ox0 = tile.ox0, cobase = tile.cobase;
    const int hw = a.h * a.w_;
    const bool vecw = (a.cout & 3) == 0; // float4 weight rows (every layer but the 4/5-channel heads)

    int bofs[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int m = (wave * PT + pt) * 32 + l31;
        const int row = m / TW;
        bofs[pt] = (hsel * PH + row + ((STK == 2 && row >= THS) ? 1 : 0)) * PW + (m % TW);
    }
    const int aofs = hsel * KK * COT + l31;

    // ---- per-thread staging plan, computed once: which patch elements / weight rows this thread
    // moves every chunk.  Patch element idx -> (ci, py, px) is the same in every chunk.
    int pinfo[NPE]; // PRE == 0: ci*hw + gy*w + gx within one sample (or -1: zero padding / unused);
                    // PRE != 0: packed (ci << 24 | py << 12 | px) (or -1)
#pragma unroll
    for (int j = 0; j < NPE; ++j) {
        const int idx = tid + j * NT;
        int v = -1;
        if (idx < PATCH) {
            const int ci = idx / (PH * PW);
            const int r = idx - ci * (PH * PW);
            const int py = r / PW, px = r - py * PW;
            const int gx = ox0 + px - PAD;
            if (STK == 2) { // bit 30: second sample of the tile
                const int sidx = py > THS + 1 ? 1 : 0;
                const int gy = sidx ? py - (THS + 2) : py - PAD;
                if (py != THS + 1 && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w_ && n + sidx < a.n) v = (sidx << 30) | (ci * hw + gy * a.w_ + gx);
            } else {
                const int gy = oy0 + py - PAD;
                if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w_) v = PRE == 0 ? ci * hw + gy * a.w_ + gx : ((ci << 24) | (gy << 12) | gx);
            }
        }
        pinfo[j] = v;
    }
    int woff[NWE]; // float4 slot q -> offset of its row start inside one chunk's weight block (or -1)
#pragma unroll
    for (int j = 0; j < NWE; ++j) {
        const int q = tid + j * NT;
        int v = -1;
        if (q < WTS / 4) {
            const int kk = (q * 4) / COT, co4 = (q * 4) - kk * COT;
            if (cobase + co4 < a.cout) v = kk * a.cout + cobase + co4;
        }
        woff[j] = v;
    }

    f32x16 acc[CT][PT];
    acc_zero(acc);

    float pv[NPE];
    float4 wv[NWE];
    // fetch chunk `cb` into registers (global loads stay in flight while the MFMAs of the previous chunk run)
    auto prefetch = [&](int cb) {
        if (PRE == 0) {
            // all CI_T channels of a chunk come from one concat source (c0 is a multiple of CI_T)
            const float *base = concat_chunk(a, cb, n, hw);
            const float *base1 = STK == 2 ? concat_chunk(a, cb, n + 1, hw) : base; // the tile's second sample
#pragma unroll
            for (int j = 0; j < NPE; ++j) {
                const int pi = pinfo[j];
                if (STK == 2) pv[j] = pi >= 0 ? (pi >> 30 ? base1 : base)[pi & 0x3FFFFFFF] : 0.f;
                else pv[j] = pi >= 0 ? base[pi] : 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NPE; ++j) {
                const int pi = pinfo[j];
                pv[j] = pi >= 0 ? fetch<PRE>(a, n, cb + (pi >> 24), (pi >> 12) & 0xFFF, pi & 0xFFF) : 0.f;
            }
        }
        const float *wb = a.w + (size_t)cb * KK * a.cout;
        if (vecw) {
#pragma unroll
            for (int j = 0; j < NWE; ++j) wv[j] = woff[j] >= 0 ? *(const float4 *)(wb + woff[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int j = 0; j < NWE; ++j) {
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if (woff[j] >= 0) {
                    const int kk = woff[j] / a.cout, co = woff[j] - kk * a.cout;
                    const float *wr = wb + woff[j];
                    t.x = wr[0];
                    if (co + 1 < a.cout) t.y = wr[1];
                    if (co + 2 < a.cout) t.z = wr[2];
                    if (co + 3 < a.cout) t.w = wr[3];
                }
                wv[j] = t;
            }
        }
    };

    prefetch(0);
    for (int cb = 0; cb < a.cin; cb += CI_T) {
        __syncthreads(); // everyone is done reading the previous chunk from LDS
#pragma unroll
        for (int j = 0; j < NPE; ++j) {
            const int idx = tid + j * NT;
            if (idx < PATCH) sp[idx] = pv[j];
        }
#pragma unroll
        for (int j = 0; j < NWE; ++j) {
            const int q = tid + j * NT;
            if (q < WTS / 4) *(float4 *)(sw + q * 4) = wv[j];
        }
        __syncthreads();
        if (cb + CI_T < a.cin) prefetch(cb + CI_T);
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
#pragma unroll
                for (int cp = 0; cp < CI_T / 2; ++cp) {
                    const int koff_w = ((cp * 2) * KK + ky * KS + kx) * COT;
                    const int koff_p = (cp * 2) * PH * PW + ky * PW + kx;
                    float av[CT], bv[PT];
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) av[ct] = sw[aofs + koff_w + ct * 32];
#pragma unroll
                    for (int pt = 0; pt < PT; ++pt) bv[pt] = sp[bofs[pt] + koff_p];
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                        for (int pt = 0; pt < PT; ++pt)
                            acc[ct][pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
                }
            }
        }
    }
    // epilogue: conv_store's, with the second sample of a stacked tile and cout that is no multiple of 32.  Its own copy: through
    // conv_store / acc_channel the two five-wave PRE = 1 instantiations took 105 VGPRs instead of 95 (occupancy 5 -> 4)
    uint32_t omax = 0u;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int m = (wave * PT + pt) * 32 + l31;
        const int row = m / TW, sidx = STK == 2 ? row / THS : 0;
        const int oy = oy0 + row - sidx * THS, ox = ox0 + (m % TW);
        const bool pok = oy < a.h && ox < a.w_ && n + sidx < a.n;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = cobase + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
                if (pok && ch < a.cout) {
                    const float v = lrelu_bias(acc[ct][pt][r], a.bias[ch]);
                    amax_fold(omax, v);
                    a.y[(((size_t)(n + sidx) * a.cout + ch) * a.h + oy) * a.w_ + ox] = v;
                }
            }
        }
    }
    if (a.am_out) amax_commit(a.am_out, omax);
}

// ---------------------------------------------------------------- dispatch
template <int KS, int CI_T, int CT, int PT, int WP, int TW, int PRE>
static void launch_conv(const ConvArgs &a0, hipStream_t s)
{
    ConvArgs a = a0;
    launch_tiles<k_conv<KS, CI_T, CT, PT, WP, TW, PRE>>(a, WP * PT * 32 / TW, TW, (a.cout + CT * 32 - 1) / (CT * 32), false, WP * 64, 0, s);
}

// two whole samples per tile (sample height == half the tile height)
template <int KS, int CI_T, int CT, int PT, int WP, int TW>
static void launch_conv_stacked(const ConvArgs &a0, hipStream_t s)
{
    ConvArgs a = a0;
    a.tiles_x = (a.w_ + TW - 1) / TW;
    a.tiles_y = 1;
    dim3 grid((unsigned)(((a.n + 1) / 2) * a.tiles_x), (unsigned)((a.cout + CT * 32 - 1) / (CT * 32)));
    k_conv<KS, CI_T, CT, PT, WP, TW, 0, 2><<<grid, WP * 64, 0, s>>>(a);
}

template <int KS, int CI_T, int CT, int PRE>
static void launch_conv_tw(const ConvArgs &a, hipStream_t s)
{
    // pixel tile: prefer power-of-two widths that divide W (4 waves, one per SIMD); exact 20- / 10-wide
    // tiles for the 16x20 and 8x10 levels of a 320x256 input; 32-wide with masking otherwise
    if (a.w_ % 32 == 0) launch_conv<KS, CI_T, CT, 2, 4, 32, PRE>(a, s);
    else if (a.w_ % 16 == 0) launch_conv<KS, CI_T, CT, 2, 4, 16, PRE>(a, s);
    else if (a.w_ % 8 == 0) launch_conv<KS, CI_T, CT, 2, 4, 8, PRE>(a, s);
    else if (a.w_ % 20 == 0 && a.h % 8 == 0) {
        // 20-wide levels (16x20 of a 320x256 input): 8x20-pixel tiles, 5 waves.  What decides here is how evenly
        // the workgroups spread over 256 CUs: 40 samples x 8 blocks of 64 channels = 320 ten-wave workgroups
        // leave a quarter of the CUs with twice the work (68 TF/s); 1280 five-wave workgroups of 32 channels
        // reach 92 TF/s.  The wider channel block only pays once there are >= 8 workgroups per CU.
        const long wgs64 = (long)a.n * (a.h / 8) * (a.cout / 64);
        if (CT == 2 && wgs64 < 2048) launch_conv<KS, CI_T, 1, 1, 5, 20, PRE>(a, s);
        else launch_conv<KS, CI_T, CT, 1, 5, 20, PRE>(a, s);
    }
    else if (a.w_ % 10 == 0) {
        // 10-wide levels (8x10 of a 320x256 input): a 16x10 five-wave tile is two samples; one sample per tile
        // would leave half of every MFMA column masked
        if (KS == 3 && PRE == 0 && a.h == 8) launch_conv_stacked<3, CI_T, 1, 1, 5, 10>(a, s);
        else launch_conv<KS, CI_T, CT, 1, 5, 10, PRE>(a, s);
    }
    else launch_conv<KS, CI_T, CT, 2, 4, 32, PRE>(a, s);
}

static int conv_dispatch(const ConvArgs &a, int ks, int pre, hipStream_t s)
{
    // 64-channel tiles only when that still leaves >= 16 workgroups per CU: measured on the 40-sample interpolation
    // UNet, 32-channel tiles (twice the workgroups, ~30 fewer VGPRs) are faster at every level (forward 96.6 -> 104 TF/s)
    const long px_tiles = (long)a.n * ((a.h * a.w_ + 255) / 256);
    const bool wide = a.cout >= 64 && px_tiles * (a.cout / 64) >= 4096;
    if (ks == 7) {
        if (pre != 0) return V2E_EINVAL;
        if (a.cin % 4 == 0) launch_conv<7, 4, 1, 2, 4, 32, 0>(a, s);
        else launch_conv<7, 2, 1, 2, 4, 32, 0>(a, s);
    } else if (ks == 5) {
        if (pre == 2) return V2E_EINVAL;
        if (wide) { if (pre) launch_conv<5, 4, 2, 2, 4, 32, 1>(a, s); else launch_conv<5, 4, 2, 2, 4, 32, 0>(a, s); }
        else { if (pre) launch_conv<5, 4, 1, 2, 4, 32, 1>(a, s); else launch_conv<5, 4, 1, 2, 4, 32, 0>(a, s); }
    } else if (ks == 3) {
        if (wide) {
            if (pre == 0) launch_conv_tw<3, 8, 2, 0>(a, s);
            else if (pre == 1) launch_conv_tw<3, 8, 2, 1>(a, s);
            else launch_conv_tw<3, 8, 2, 2>(a, s);
        } else {
            if (pre == 0) launch_conv_tw<3, 8, 1, 0>(a, s);
            else if (pre == 1) launch_conv_tw<3, 8, 1, 1>(a, s);
            else launch_conv_tw<3, 8, 1, 2>(a, s);
        }
    } else {
        return V2E_EINVAL;
    }
    return 0;
}
