// slomo_stream.h -- the streaming kernels beside the UNet convolutions (included by slomo.hip): avg_pool2d and the bilinear x2 as
// their own passes, the VALU convolution of the 4- / 5-channel head, weight packing, backWarp input preparation and fusion, the
// range slot of the network input, the flow speed maximum; and a host launcher for each.

// ... one output per thread, for widths that are not a multiple of 4
__global__ __launch_bounds__(256) void k_avgpool2_scalar(const float *__restrict__ x, float *__restrict__ y, long long nc, int h, int w)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nc * h * w) return;
    const int ox = (int)(q % w);
    const long long r = q / w;
    const int oy = (int)(r % h);
    const long long c = r / h;
    const float *p = x + ((c * (2 * h) + 2 * oy) * (long long)(2 * w)) + 2 * ox;
    y[q] = (((p[0] + p[1]) + p[2 * w]) + p[2 * w + 1]) * 0.25f;
}

// F.avg_pool2d(x, 2) as its own pass: [nc][2h][2w] -> [nc][h][w]; 4 outputs per thread
__global__ __launch_bounds__(256) void k_avgpool2(const float *__restrict__ x, float *__restrict__ y, long long nc, int h, int w)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x; // group of 4 outputs along x
    const int wq = w >> 2;
    const long long total = nc * h * wq;
    if (q >= total) return;
    const int xq = (int)(q % wq);
    const long long r = q / wq;
    const int oy = (int)(r % h);
    const long long c = r / h;
    const float *p = x + ((c * (2 * h) + 2 * oy) * (long long)(2 * w)) + 8 * xq;
    const float4 a0 = *(const float4 *)p, a1 = *(const float4 *)(p + 4);
    const float4 b0 = *(const float4 *)(p + 2 * w), b1 = *(const float4 *)(p + 2 * w + 4);
    float4 o;
    o.x = (((a0.x + a0.y) + b0.x) + b0.y) * 0.25f;
    o.y = (((a0.z + a0.w) + b0.z) + b0.w) * 0.25f;
    o.z = (((a1.x + a1.y) + b1.x) + b1.y) * 0.25f;
    o.w = (((a1.z + a1.w) + b1.z) + b1.w) * 0.25f;
    *(float4 *)(y + (c * h + oy) * (long long)w + 4 * xq) = o;
}

// F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) as its own pass:
// [nc][h/2][w/2] -> [nc][h][w].  One thread = 2 rows x 4 consecutive outputs (two float4 stores) from 2 source rows x 4
// columns: output rows 2t-1 and 2t both lie between source rows t-1 and t (weights 0.75/0.25 and 0.25/0.75; at the
// top edge the clamped coordinate gives weight 0 to the second row), and the source coordinates of outputs 4j..4j+3 are
// 2j-0.25, 2j+0.25, 2j+0.75, 2j+1.25, so the fractional weights are the exact constants that fetch<2> computes, and
// the products/sums are evaluated in the same order.
__global__ __launch_bounds__(256) void k_upsample2(const float *__restrict__ x, float *__restrict__ y, long long nc, int h, int w)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const int wq = w >> 2;
    const int sh = h >> 1, sw = w >> 1;
    const long long total = nc * (sh + 1) * wq;
    if (q >= total) return;
    const int j = (int)(q % wq);
    const long long r = q / wq;
    const int t = (int)(r % (sh + 1)); // output rows 2t-1 (t >= 1) and 2t (t < sh)
    const long long c = r / (sh + 1);
    const int ya = t - 1 < 0 ? 0 : t - 1, yb = t == 0 ? (sh > 1 ? 1 : 0) : (t < sh ? t : sh - 1); // t == 0: the reference's y1 (weight 0)
    const float *p0 = x + (c * sh + ya) * (long long)sw, *p1 = x + (c * sh + yb) * (long long)sw;
    // source columns 2j-1 .. 2j+2, clamped
    const int cm = 2 * j - 1 < 0 ? 0 : 2 * j - 1, c0 = 2 * j, c1 = 2 * j + 1 < sw ? 2 * j + 1 : sw - 1,
              c2 = 2 * j + 2 < sw ? 2 * j + 2 : sw - 1;
    const float a_m = p0[cm], a_0 = p0[c0], a_1 = p0[c1], a_2 = p0[c2];
    const float b_m = p1[cm], b_0 = p1[c0], b_1 = p1[c1], b_2 = p1[c2];
    const float lx0 = j == 0 ? 0.f : 0.75f, hx0 = 1.f - lx0; // output 4j: x0 = 2j-1 (0 when clamped), x1 = x0+1
    // when j == 0 the reference has x0 = 0, x1 = min(1, sw-1); a_m == a_0 there and lx = 0
    const float t00 = j == 0 ? a_0 : a_m, t01 = j == 0 ? a_1 : a_0, u00 = j == 0 ? b_0 : b_m, u01 = j == 0 ? b_1 : b_0;
    // the four horizontal blends of each source row (same for both output rows)
    const float ax = hx0 * t00 + lx0 * t01, ay = 0.75f * a_0 + 0.25f * a_1, az = 0.25f * a_0 + 0.75f * a_1, aw = 0.75f * a_1 + 0.25f * a_2;
    const float bx = hx0 * u00 + lx0 * u01, by = 0.75f * b_0 + 0.25f * b_1, bz = 0.25f * b_0 + 0.75f * b_1, bw = 0.75f * b_1 + 0.25f * b_2;
    if (t >= 1) { // row 2t-1: ry = t - 0.75 -> y0 = t-1, ly = 0.25
        const float ly = ((float)(2 * t - 1) + 0.5f) * 0.5f - 0.5f - (float)(t - 1), hy = 1.f - ly;
        float4 o;
        o.x = hy * ax + ly * bx; o.y = hy * ay + ly * by; o.z = hy * az + ly * bz; o.w = hy * aw + ly * bw;
        *(float4 *)(y + (c * h + 2 * t - 1) * (long long)w + 4 * j) = o;
    }
    if (t < sh) { // row 2t: ry = t - 0.25 (clamped to 0 at the top) -> y0 = max(t-1, 0), ly = 0.75 (0 at the top)
        float ry = ((float)(2 * t) + 0.5f) * 0.5f - 0.5f;
        ry = ry < 0.f ? 0.f : ry;
        const float ly = ry - (float)ya, hy = 1.f - ly;
        float4 o;
        o.x = hy * ax + ly * bx; o.y = hy * ay + ly * by; o.z = hy * az + ly * bz; o.w = hy * aw + ly * bw;
        *(float4 *)(y + (c * h + 2 * t) * (long long)w + 4 * j) = o;
    }
}

// same, one output per thread, for widths that are not a multiple of 4
__global__ __launch_bounds__(256) void k_upsample2_scalar(const float *__restrict__ x, float *__restrict__ y, long long nc, int h, int w)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = nc * h * w;
    if (i >= total) return;
    const int gx = (int)(i % w);
    const long long r = i / w;
    const int gy = (int)(r % h);
    const long long c = r / h;
    const int sh = h >> 1, sw = w >> 1;
    float ry = ((float)gy + 0.5f) * 0.5f - 0.5f;
    float rx = ((float)gx + 0.5f) * 0.5f - 0.5f;
    ry = ry < 0.f ? 0.f : ry;
    rx = rx < 0.f ? 0.f : rx;
    const int y0 = (int)ry, x0 = (int)rx;
    const int y1 = y0 + (y0 < sh - 1 ? 1 : 0), x1 = x0 + (x0 < sw - 1 ? 1 : 0);
    const float ly = ry - (float)y0, lx = rx - (float)x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float *p = x + c * sh * sw;
    y[i] = hy * (hx * p[y0 * sw + x0] + lx * p[y0 * sw + x1]) + ly * (hx * p[y1 * sw + x0] + lx * p[y1 * sw + x1]);
}

// Final UNet layer (32 -> 4/5 channels, 3x3): too few output channels for a 32-wide MFMA tile (84 % of it would be padding: at the
// ~190 TF/s the 32-channel full-resolution layers reach, a padded tile would take longer than this), so it runs on the VALU from an
// LDS-staged input patch with wave-uniform scalar weight loads.  Round 6: FOUR pixels along x per thread -- a row of the patch is read
// as 6 floats (one 16-byte and one 8-byte LDS read) for 3 taps x 4 pixels x COUT = 60 multiply-adds, where one pixel per thread read
// 9 floats for 45 (the kernel was bound by its LDS reads: 33 TF/s); same accumulation order (ci, ky, kx) per output.
template <int COUT>
__global__ __launch_bounds__(256) void k_conv3x3_small(const float *__restrict__ x, const float *__restrict__ wp /* [cin][3][3][COUT] */,
                                                       const float *__restrict__ bias, float *__restrict__ y, int n_img, int cin,
                                                       int h, int w, int tiles_x, int tiles_y)
{
    constexpr int PXT = 4, TW = 64, TH = 16, PH = TH + 2, PW = 68 /* 66 padded: rows start 16-byte aligned */, CI_T = 8;
    __shared__ __attribute__((aligned(16))) float sp[CI_T * PH * PW];
    const int tid = threadIdx.x;
    int bx = blockIdx.x;
    const int tx_i = bx % tiles_x; bx /= tiles_x;
    const int ty_i = bx % tiles_y;
    const int n = bx / tiles_y;
    const int oy0 = ty_i * TH, ox0 = tx_i * TW;
    const int ty = tid / (TW / PXT), tx = (tid % (TW / PXT)) * PXT; // this thread's row and first column inside the tile
    const int hw = h * w;
    float acc[PXT][COUT];
#pragma unroll
    for (int q = 0; q < PXT; ++q)
#pragma unroll
        for (int co = 0; co < COUT; ++co) acc[q][co] = 0.f;
    for (int cb = 0; cb < cin; cb += CI_T) {
        // the chunk's patch: every load of a thread in flight before the first LDS store (a rolled loop waits for each load in turn)
        constexpr int NPATCH = CI_T * PH * (TW + 2), NLD = (NPATCH + 255) / 256;
        float stg[NLD];
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + j * 256;
            const int ci = idx / (PH * (TW + 2));
            const int r = idx - ci * (PH * (TW + 2));
            const int py = r / (TW + 2), px = r - py * (TW + 2);
            const int gy = oy0 + py - 1, gx = ox0 + px - 1;
            stg[j] = 0.f;
            if (idx < NPATCH && cb + ci < cin && gy >= 0 && gy < h && gx >= 0 && gx < w) stg[j] = x[((size_t)n * cin + cb + ci) * hw + gy * w + gx];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + j * 256;
            const int ci = idx / (PH * (TW + 2));
            const int r = idx - ci * (PH * (TW + 2));
            const int py = r / (TW + 2), px = r - py * (TW + 2);
            if (idx < NPATCH) sp[(ci * PH + py) * PW + px] = stg[j];
        }
        __syncthreads();
#pragma unroll
        for (int ci = 0; ci < CI_T; ++ci) {
            if (cb + ci >= cin) break;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const float *row = sp + (ci * PH + ty + ky) * PW + tx;
                const float4 va = *(const float4 *)row;
                const float2 vb = *(const float2 *)(row + 4);
                const float v[6] = {va.x, va.y, va.z, va.w, vb.x, vb.y};
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float *wr = wp + ((size_t)(cb + ci) * 9 + ky * 3 + kx) * COUT;
#pragma unroll
                    for (int co = 0; co < COUT; ++co) {
                        const float wv = wr[co];
#pragma unroll
                        for (int q = 0; q < PXT; ++q) acc[q][co] = fmaf(wv, v[q + kx], acc[q][co]);
                    }
                }
            }
        }
    }
    const int oy = oy0 + ty;
    if (oy < h) {
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            const float bv = bias[co];
            float o[PXT];
#pragma unroll
            for (int q = 0; q < PXT; ++q) {
                const float t = acc[q][co] + bv;
                o[q] = t > 0.f ? t : t * 0.1f;
            }
            float *dst = y + ((size_t)n * COUT + co) * hw + oy * w + ox0 + tx;
            if (ox0 + tx + PXT <= w && (w & 3) == 0) {
                *(float4 *)dst = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int q = 0; q < PXT; ++q)
                    if (ox0 + tx + q < w) dst[q] = o[q];
            }
        }
    }
}

__global__ void k_pack_weight(const float *__restrict__ w, float *__restrict__ wp, int cout, int cin, int kk)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)cout * cin * kk;
    if (i >= total) return;
    // wp[(ci*kk + k)*cout + co] = w[(co*cin + ci)*kk + k]
    const int co = (int)(i % cout);
    const size_t r = i / cout;
    const int k = (int)(r % kk);
    const int ci = (int)(r / kk);
    wp[i] = w[((size_t)co * cin + ci) * kk + k];
}

// torch.nn.functional.grid_sample(img, grid) as used by backWarp (model.py:289-299):
// bilinear, zeros padding, align_corners=False.  x,y already include the flow.
__device__ __forceinline__ float warp_sample(const float *__restrict__ img, int h, int w, float x, float y)
{
    // model.py:294-295: range -1..1, same float32 operation sequence
    float gx = 2.f * (x / (float)w - 0.5f);
    float gy = 2.f * (y / (float)h - 0.5f);
    // grid_sampler unnormalize, align_corners=False: ((g + 1) * size - 1) / 2
    float ix = ((gx + 1.f) * (float)w - 1.f) / 2.f;
    float iy = ((gy + 1.f) * (float)h - 1.f) / 2.f;
    float fx0 = floorf(ix), fy0 = floorf(iy);
    int x0 = (int)fx0, y0 = (int)fy0;
    int x1 = x0 + 1, y1 = y0 + 1;
    float tx = ix - fx0, ty = iy - fy0;
    // weights as in ATen grid_sampler_2d: nw = (x1-ix)*(y1-iy) ...
    float wx1 = tx, wx0 = 1.f - tx, wy1 = ty, wy0 = 1.f - ty;
    float nw = wx0 * wy0, ne = wx1 * wy0, sw_ = wx0 * wy1, se = wx1 * wy1;
    float out = 0.f;
    if (y0 >= 0 && y0 < h) {
        if (x0 >= 0 && x0 < w) out += img[y0 * w + x0] * nw;
        if (x1 >= 0 && x1 < w) out += img[y0 * w + x1] * ne;
    }
    if (y1 >= 0 && y1 < h) {
        if (x0 >= 0 && x0 < w) out += img[y1 * w + x0] * sw_;
        if (x1 >= 0 && x1 < w) out += img[y1 * w + x1] * se;
    }
    return out;
}

// slomo.py:405-419: x12[s] = [I0, I1, F01(2), F10(2), Ft1(2), Ft0(2), g(I1,Ft1), g(I0,Ft0)] of pair bi at time row c
// (k_prep: sample s = ti*b + bi; k_prep_tab: the pair and the row from a per-sample table)
__device__ __forceinline__ void prep_sample(const float *__restrict__ i0, const float *__restrict__ i1,
                                            const float *__restrict__ flow, const float *__restrict__ c, int bi, int s,
                                            int h, int w, int p, float *__restrict__ x12)
{
    const int hw = h * w;
    // fCoeff of slomo.py:406-407, evaluated by the host in Python doubles and rounded to float32
    const float c00 = c[0], c01 = c[1], c10 = c[2], c11 = c[3];
    const float *fl = flow + (size_t)bi * 4 * hw;
    const float f01x = fl[p], f01y = fl[hw + p], f10x = fl[2 * hw + p], f10y = fl[3 * hw + p];
    const float ft0x = c00 * f01x + c01 * f10x, ft0y = c00 * f01y + c01 * f10y;
    const float ft1x = c10 * f01x + c11 * f10x, ft1y = c10 * f01y + c11 * f10y;
    const int py = p / w, px = p - py * w;
    const float *im0 = i0 + (size_t)bi * hw, *im1 = i1 + (size_t)bi * hw;
    const float g0 = warp_sample(im0, h, w, (float)px + ft0x, (float)py + ft0y);
    const float g1 = warp_sample(im1, h, w, (float)px + ft1x, (float)py + ft1y);
    float *o = x12 + (size_t)s * 12 * hw + p;
    o[0] = im0[p];
    o[hw] = im1[p];
    o[2 * hw] = f01x; o[3 * hw] = f01y;
    o[4 * hw] = f10x; o[5 * hw] = f10y;
    o[6 * hw] = ft1x; o[7 * hw] = ft1y;
    o[8 * hw] = ft0x; o[9 * hw] = ft0y;
    o[10 * hw] = g1;
    o[11 * hw] = g0;
}

__global__ __launch_bounds__(256) void k_prep(const float *__restrict__ i0, const float *__restrict__ i1,
                                              const float *__restrict__ flow, const float *__restrict__ coef, int n_t,
                                              int b, int h, int w, float *__restrict__ x12)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y; // ti*b + bi
    if (p >= h * w) return;
    const int ti = s / b, bi = s - ti * b;
    prep_sample(i0, i1, flow, coef + ti * 6, bi, s, h, w, p, x12);
}

// tab[s] = {pair, coefficient row, output frame} (the frame is k_f32_to_u8_tab's)
__global__ __launch_bounds__(256) void k_prep_tab(const float *__restrict__ i0, const float *__restrict__ i1,
                                                  const float *__restrict__ flow, const float *__restrict__ coef,
                                                  const int *__restrict__ tab, int h, int w, float *__restrict__ x12)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (p >= h * w) return;
    prep_sample(i0, i1, flow, coef + tab[3 * s + 1] * 6, tab[3 * s], s, h, w, p, x12);
}

// slomo.py:421-433 for sample s of pair bi at time row c
__device__ __forceinline__ void fuse_sample(const float *__restrict__ i0, const float *__restrict__ i1,
                                            const float *__restrict__ x12, const float *__restrict__ intrp,
                                            const float *__restrict__ c, int bi, int s, int h, int w, int p,
                                            float *__restrict__ out)
{
    const int hw = h * w;
    const float *x = x12 + (size_t)s * 12 * hw + p;
    const float *q = intrp + (size_t)s * 5 * hw + p;
    const float ft0x = q[0] + x[8 * hw], ft0y = q[hw] + x[9 * hw];
    const float ft1x = q[2 * hw] + x[6 * hw], ft1y = q[3 * hw] + x[7 * hw];
    const float v0 = 1.f / (1.f + expf(-q[4 * hw])); // torch.sigmoid
    const float v1 = 1.f - v0;
    const int py = p / w, px = p - py * w;
    const float g0 = warp_sample(i0 + (size_t)bi * hw, h, w, (float)px + ft0x, (float)py + ft0y);
    const float g1 = warp_sample(i1 + (size_t)bi * hw, h, w, (float)px + ft1x, (float)py + ft1y);
    const float w0 = c[4], w1 = c[5]; // wCoeff = [1 - t, t]
    out[(size_t)s * hw + p] = (w0 * v0 * g0 + w1 * v1 * g1) / (w0 * v0 + w1 * v1);
}

__global__ __launch_bounds__(256) void k_fuse(const float *__restrict__ i0, const float *__restrict__ i1,
                                              const float *__restrict__ x12, const float *__restrict__ intrp,
                                              const float *__restrict__ coef, int n_t, int b, int h, int w,
                                              float *__restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (p >= h * w) return;
    const int ti = s / b, bi = s - ti * b;
    fuse_sample(i0, i1, x12, intrp, coef + ti * 6, bi, s, h, w, p, out);
}

__global__ __launch_bounds__(256) void k_fuse_tab(const float *__restrict__ i0, const float *__restrict__ i1,
                                                  const float *__restrict__ x12, const float *__restrict__ intrp,
                                                  const float *__restrict__ coef, const int *__restrict__ tab, int h, int w,
                                                  float *__restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (p >= h * w) return;
    fuse_sample(i0, i1, x12, intrp, coef + tab[3 * s + 1] * 6, tab[3 * s], s, h, w, p, out);
}

// amax_fold for the network input, where a NaN must be seen too (fmaxf drops it): a NaN counts as the quiet-NaN pattern, which
// orders above +inf as an unsigned word and has the all-ones exponent act_scale tests.  (The convolution epilogues keep amax_fold:
// a NaN in a convolution's output needs an inf or a NaN upstream, and that one was flagged at the first layer.)
__device__ __forceinline__ void amax_fold_nan(uint32_t &m, float v)
{
    const uint32_t b = v != v ? 0x7fc00000u : __float_as_uint(fabsf(v));
    m = b > m ? b : m;
}

// largest |x| of a tensor into a range slot (the network input of v2e_unet_forward); the slot is only ever raised
__global__ __launch_bounds__(256) void k_amax(const float *__restrict__ x, long long n, uint32_t *__restrict__ slot)
{
    uint32_t m = 0u;
    const long long n4 = n >> 2;
    const float4 *x4 = (const float4 *)x;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = x4[i];
        amax_fold_nan(m, v.x); amax_fold_nan(m, v.y); amax_fold_nan(m, v.z); amax_fold_nan(m, v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) amax_fold_nan(m, x[(n4 << 2) + threadIdx.x]);
    amax_commit(slot, m);
}

__global__ void k_zero_u32(unsigned *__restrict__ p, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// slomo.py:359-368 (auto_upsample): the largest flow magnitude of a batch.  sqrt is monotone, so the kernel reduces the
// squared speed vx*vx + vy*vy (two products and one sum, each rounded: contraction is off for this file) of both flow pairs
// and the host takes ONE float32 sqrt of the maximum -- the same number as max(sqrt(...)) over the planes.  Non-negative floats
// order like their bit patterns: one atomicMax per wave.
// one workgroup's share (workgroup `blk` of `nblk`) of the squared-speed maximum of flow [b][4][hw], into *out_bits
__device__ __forceinline__ void max_speed2_part(const float *__restrict__ flow, int b, int hw, int blk, int nblk,
                                                unsigned *__restrict__ out_bits)
{
    float m = 0.f;
    const long long n = (long long)b * hw;
    for (long long i = (long long)blk * 256 + threadIdx.x; i < n; i += (long long)nblk * 256) {
        const int bi = (int)(i / hw);
        const int p = (int)(i - (long long)bi * hw);
        const float *fl = flow + (size_t)bi * 4 * hw + p;
        const float x0 = fl[0], y0 = fl[hw], x1 = fl[2 * (size_t)hw], y1 = fl[3 * (size_t)hw];
        const float s0 = x0 * x0 + y0 * y0;
        const float s1 = x1 * x1 + y1 * y1;
        // torch.max propagates NaN; a NaN flow makes int(np.ceil(nan)) raise in the reference: report it as NaN too
        if (s0 != s0 || s1 != s1) m = __int_as_float(0x7fc00000);
        else if (m == m) m = fmaxf(m, fmaxf(s0, s1));
    }
    unsigned bits = (m != m) ? 0xffffffffu : __float_as_uint(m);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)bits, o, 64);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0u) atomicMax(out_bits, bits);
}

__global__ __launch_bounds__(256) void k_max_speed2(const float *__restrict__ flow, int b, int hw, unsigned *__restrict__ out_bits)
{
    max_speed2_part(flow, b, hw, blockIdx.x, gridDim.x, out_bits);
}

// the same per batch of `seg` pairs: blockIdx.y = batch (the last one may hold fewer pairs), one result slot each.  A maximum is
// the same whichever workgroups fold it: bit for bit k_max_speed2 over that batch alone.
__global__ __launch_bounds__(256) void k_max_speed2_seg(const float *__restrict__ flow, int b, int seg, int hw,
                                                        unsigned *__restrict__ out_bits)
{
    const int j = blockIdx.y;
    const int b0 = j * seg;
    const int nb = min(seg, b - b0);
    max_speed2_part(flow + (size_t)b0 * 4 * hw, nb, hw, blockIdx.x, gridDim.x, out_bits + j);
}

// ---------------------------------------------------------------- host launchers
// y[nc][h][w] = avg_pool2d(x[nc][2h][2w], 2)
static void launch_avgpool2(const float *x, float *y, long long nc, int h, int w, hipStream_t s)
{
    if (w % 4 == 0) k_avgpool2<<<v2e_cdiv(nc * h * (w / 4), 256), 256, 0, s>>>(x, y, nc, h, w);
    else k_avgpool2_scalar<<<v2e_cdiv(nc * h * w, 256), 256, 0, s>>>(x, y, nc, h, w);
}

// y[nc][h][w] = bilinear x2 of x[nc][h/2][w/2]
static void launch_upsample2(const float *x, float *y, long long nc, int h, int w, hipStream_t s)
{
    if (w % 4 == 0) k_upsample2<<<v2e_cdiv(nc * (h / 2 + 1) * (w / 4), 256), 256, 0, s>>>(x, y, nc, h, w);
    else k_upsample2_scalar<<<v2e_cdiv(nc * h * w, 256), 256, 0, s>>>(x, y, nc, h, w);
}

template <int COUT>
static void launch_conv3x3_small(const float *x, const float *wp, const float *bias, float *y, int n, int cin, int h, int w, hipStream_t s)
{
    const int tiles_x = (w + 63) / 64, tiles_y = (h + 15) / 16;
    k_conv3x3_small<COUT><<<dim3((unsigned)(n * tiles_x * tiles_y)), 256, 0, s>>>(x, wp, bias, y, n, cin, h, w, tiles_x, tiles_y);
}

static void launch_pack_weight(const float *w, float *wp, int cout, int cin, int kk, hipStream_t s) { k_pack_weight<<<v2e_cdiv((int64_t)cout * cin * kk, 256), 256, 0, s>>>(w, wp, cout, cin, kk); }
static void launch_zero_u32(unsigned *p, int n, hipStream_t s) { k_zero_u32<<<v2e_cdiv(n, 64), 64, 0, s>>>(p, n); }

static void launch_amax(const float *x, long long n, uint32_t *slot, hipStream_t s)
{
    const long long nb = (n / 4 + 255) / 256;
    k_amax<<<(unsigned)(nb < 1 ? 1 : (nb > 4096 ? 4096 : nb)), 256, 0, s>>>(x, n, slot);
}

// the prep / fuse kernels: one thread per pixel, blockIdx.y = sample
template <typename... KA, typename... A>
static int launch_per_pixel(void (*k)(KA...), int samples, int h, int w, hipStream_t s, A... args)
{
    k<<<dim3(v2e_cdiv((int64_t)h * w, 256), samples), 256, 0, s>>>(args...);
    V2E_HIP(hipGetLastError());
    return 0;
}

// the max-speed kernels: `nseg` result slots zeroed, then at most 2048 workgroups over the `per_seg` flow vectors of each
template <typename... KA, typename... A>
static int launch_max_speed2(void (*k)(KA...), long long per_seg, int nseg, unsigned *out_bits, hipStream_t s, A... args)
{
    launch_zero_u32(out_bits, nseg, s);
    int blocks = v2e_cdiv(per_seg, 256);
    if (blocks > 2048) blocks = 2048;
    k<<<dim3(blocks, nseg), 256, 0, s>>>(args...);
    V2E_HIP(hipGetLastError());
    return 0;
}
