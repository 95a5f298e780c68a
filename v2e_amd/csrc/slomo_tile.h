// slomo_tile.h -- the steps k_conv, k_conv_s3 and k_conv_s3p share beside their multiplies, each written once (included by
// slomo_conv.h behind ConvArgs): workgroup -> tile, the concat source of a channel chunk, the staging plan of the split-operand
// kernels, the accumulators' C/D register layout with the epilogue that stores through it, and the launchers' grid.

// ---------------------------------------------------------------- workgroup -> tile
struct ConvTile { int n, oy0, ox0, cobase; }; // first sample, top left output pixel, first output channel

// false: the workgroup is padding of the 1-D grid.  a.ncb > 0: that grid, in XCD order.  Workgroups go to the 8 XCDs round-robin
// by linear id and each XCD has its own L2, so the channel blocks of ONE pixel tile are consecutive on ONE XCD (ids L, L+8, L+16,
// ...): the tile's input patch crosses the fabric once instead of once per channel block, and since the workgroups of an XCD
// walk the input-channel chunks roughly in step, the weight slices they share stay L2-resident too (measured: DESIGN.md 4).
// Otherwise x = pixel tile, y = channel block.  STK: samples per tile (k_conv's stacked tiles: tiles_y is 1).
template <int TH, int TW, int COT, int STK = 1>
__device__ __forceinline__ bool conv_tile(const ConvArgs &a, ConvTile &t)
{
    int bx, cblk;
    if (a.ncb > 0) {
        const int L = blockIdx.x, j = L >> 3;
        cblk = j % a.ncb;
        bx = (j / a.ncb) * 8 + (L & 7);
        if (bx >= a.n * a.tiles_x * a.tiles_y) return false; // padding of the last group of 8 pixel tiles
    } else {
        bx = blockIdx.x;
        cblk = blockIdx.y;
    }
    const int tx_i = bx % a.tiles_x; bx /= a.tiles_x;
    const int ty_i = bx % a.tiles_y;
    t.n = (bx / a.tiles_y) * STK;
    t.oy0 = ty_i * TH; t.ox0 = tx_i * TW;
    t.cobase = cblk * COT;
    return true;
}

// channel c of x0 ++ x1 in sample n: its plane in the source that holds it (hw: elements per plane of the sources).  All
// channels of a chunk come from one source (c0 is a multiple of every chunk size that meets a concat).
__device__ __forceinline__ const float *concat_chunk(const ConvArgs &a, int c, int n, int hw)
{
    const float *src;
    int cs, C;
    if (c < a.c0) { src = a.x0; cs = c; C = a.c0; }
    else { src = a.x1; cs = c - a.c0; C = a.c1; }
    return src + ((size_t)n * C + cs) * hw;
}

// ---------------------------------------------------------------- staging plan of the split-operand kernels
// What a thread of k_conv_s3 / k_conv_s3p moves every chunk, computed once (WP waves of PT pixel tiles, KS x KS taps, COT output
// channels, WU 16-byte weight units resident at a time; LDS layouts: slomo_s3.h):
//   pinfo  patch item tid + j * NT (8 channels of one patch pixel) -> offset of its first channel inside one sample's chunk, in
//          floats (PRES, pre-split input: in 16-byte units), or -1: zero padding / unused
//   woff   weight unit tid + j * NT -> offset inside one group's weight block (surplus threads load a valid unit and do not store it)
template <int KS, int WP, int PT, int TW, int COT, int WU, bool PRES, int NPI, int NWU>
__device__ __forceinline__ void s3_plan(const ConvArgs &a, const ConvTile &t, int (&pinfo)[NPI], int (&woff)[NWU])
{
    constexpr int NT = WP * 64, PAD = KS / 2;
    constexpr int PH = WP * PT * 32 / TW + KS - 1, PW = TW + KS - 1, PP = PH * PW;
    const int tid = threadIdx.x, hw = a.h * a.w_;
#pragma unroll
    for (int j = 0; j < NPI; ++j) {
        const int i = tid + j * NT;
        int v = -1;
        if (i < 2 * PP) {
            const int cig = i / PP, r = i - cig * PP;
            const int py = r / PW, px = r - py * PW;
            const int gy = t.oy0 + py - PAD, gx = t.ox0 + px - PAD;
            if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w_) v = cig * (PRES ? 1 : 8) * hw + gy * a.w_ + gx;
        }
        pinfo[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NWU; ++j) {
        const int u = tid + j * NT;
        const int uu = u < WU ? u : WU - 1;
        const int r = uu / COT, c = uu - r * COT;
        woff[j] = r * a.cout + t.cobase + c;
    }
}

// ---------------------------------------------------------------- accumulators and epilogue
template <int CT, int PT>
__device__ __forceinline__ void acc_zero(f32x16 (&acc)[CT][PT])
{
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ct][pt][r] = 0.f;
}

// C/D layout of the 32 x 32 multiplies: register r of a lane in channel tile ct is this channel of the tile's block, at pixel lane & 31
__device__ __forceinline__ int acc_channel(int ct, int r)
{
    const int hsel = (threadIdx.x & 63) >> 5;
    return ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
}

// the value a convolution stores: bias, leaky_relu(0.1).  s: the sum, times os1 already where the operands were staged scaled.
__device__ __forceinline__ float lrelu_bias(float s, float bias)
{
    const float v = s + bias;
    return v > 0.f ? v : v * 0.1f;
}

// the epilogue: every accumulator through lrelu_bias into y (NCHW: a register is 32 consecutive x of one channel), the largest
// |value| into the layer's range slot.  os1: the power of two a two-piece kernel divides out of its sums, 1 elsewhere (folded
// away).  cout is a multiple of 32.  (k_conv, with its stacked tiles and its masked channels, has a loop of its own: slomo_conv.h.)
template <int TW, int CT, int PT>
__device__ __forceinline__ void conv_store(const ConvArgs &a, const ConvTile &t, const f32x16 (&acc)[CT][PT], float os1)
{
    const int wave = threadIdx.x >> 6, l31 = threadIdx.x & 31;
    uint32_t omax = 0u;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int m = (wave * PT + pt) * 32 + l31;
        const int oy = t.oy0 + m / TW, ox = t.ox0 + (m % TW);
        const bool pok = oy < a.h && ox < a.w_;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = t.cobase + acc_channel(ct, r);
                if (pok) {
                    const float v = lrelu_bias(acc[ct][pt][r] * os1, a.bias[ch]);
                    amax_fold(omax, v);
                    a.y[(((size_t)t.n * a.cout + ch) * a.h + oy) * a.w_ + ox] = v;
                }
            }
        }
    }
    if (a.am_out) amax_commit(a.am_out, omax);
}

// ---------------------------------------------------------------- host: grid and launch
// Launches K on the th x tw pixel tiles of `a` times ncb channel blocks, with `lds` bytes of dynamic LDS (the attribute that
// allows them is set once per kernel function): a 1-D grid in XCD order (conv_tile) where the launcher asks for it, else 2-D.
template <void (*K)(ConvArgs)>
static int launch_tiles(ConvArgs &a, int th, int tw, int ncb, bool xcd_order, int threads, size_t lds, hipStream_t s)
{
    static bool attr_set = false; // one per K
    if (lds && !attr_set) {
        V2E_HIP(hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set = true;
    }
    a.tiles_x = (a.w_ + tw - 1) / tw;
    a.tiles_y = (a.h + th - 1) / th;
    const int ntiles = a.n * a.tiles_x * a.tiles_y;
    a.ncb = xcd_order ? ncb : 0;
    const dim3 grid = a.ncb ? dim3((unsigned)((ntiles + 7) / 8 * 8 * ncb)) : dim3((unsigned)ntiles, (unsigned)ncb);
    K<<<grid, threads, lds, s>>>(a);
    return 0;
}
