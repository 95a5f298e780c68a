// patches.hip -- per-event time-surface patches: for every row of a device-resident run the (2r+1) x (2r+1) patch of ages and
// polarities around it, as the maps were just before the row (host side: v2e_amd/patches.py, EventPatches).
//
// Rows are float4 (t, x = column, y = row, p), taken in row order.  A row is bad under exactly DenoiseSweep's rule: t not finite, or
// x / y not an integer value inside [0,W) / [0,H); p is not examined for validity.  A bad row reads and writes no map and gets
// valid = 0; its features are the "none" values below.  last_t (float32 [H][W], starts at -inf) and last_p (int8 [H][W], starts at
// 0) are carried from call to call.  For a valid row i at (x, y) and every offset (dy, dx) in [-r, r]^2, r = 1, 2 or 3, the centre
// included, the patch entry [dy + r][dx + r] looks at q = (x + dx, y + dy): outside the sensor the entry is none; otherwise T_q and
// P_q are the t and the sign of p (+1 if p > 0, else -1) of the latest valid row j < i at q in this call, else the carried maps'
// (a carried T_q of -inf: none).  age = (double)t_i - (double)T_q; a T_q later than t_i gives a negative age, which is kept.  The
// centre entry is the previous event at the same pixel: the row is never in its own patch.  After reading, the row stamps
// last_t[y][x] = t_i and last_p[y][x] = sign(p_i).  out is float32 [n][2][P][P], P = 2r + 1:
//   mode 0 ("age"):    channel 0 = (float)age, rounded to nearest even, +inf where none; channel 1 = P_q as +-1.0, 0 where none.
//   mode 1 ("linear"): channel 0 = 0 where none or age >= tau, 1 where age <= 0, otherwise (float)(1 - age / tau), the division and
//                      the subtraction each rounded in float64; channel 1 = P_q where not none and age < tau, otherwise 0.
//
// The lookup "the latest earlier row at q" is denoise.hip's: v2e_denoise_keys gives row i the key pixel << 32 | i, the host sorts
// the keys, v2e_denoise_segments finds each pixel's stretch, and rowkeys.h's latest_before searches q's stretch for that row;
// one 16-byte gather of it supplies both t and p.  Every entry is then independent of every other, so the result depends on
// the row order alone, not on scheduling or on how a clip is cut into calls or passes.  The rule of one entry is patch_entry.h's
// patch_entry, which mlpf.hip's fused kernel calls as well.
//
// Mapping: one thread per (row, offset), the rows taken in sorted-key (pixel) order as in k_denoise_ages: the P * P lanes of a row
// read adjacent seg entries, neighbouring rows search neighbouring stretches, and a row's lanes write two contiguous stretches of
// P * P floats.  Bad rows have no row index in the sorted keys; k_patches_bad_rows walks the rows in row order, writes valid[] for
// all of them and the none values of the bad ones.  (Threads in row order -- coalesced row reads, scattered searches -- measured
// slower at r = 3: 59 against 51 us on 137 k rows, 11.3 against 4.2 ms on 4.4 M rows, profiles/r17_event_patches.txt; only the
// sorted order was kept.)
#include "common.h"
#include "patch_entry.h"

namespace {

constexpr int FEATURES_MAX_BLOCKS = 1 << 16;

struct PatchArgs {
    PatchSource src;             // rows, row index and carried maps
    int n;                       // rows of this pass
    int mode;                    // 0 age, 1 linear
    double tau;
    float *out;                  // [n][2][P][P]
    unsigned char *valid;        // [n]
};

template <int R>
__global__ __launch_bounds__(256) void k_patches_features(PatchArgs a)
{
    constexpr int P = 2 * R + 1, PP = P * P;
    const int W = a.src.W, H = a.src.H;
    const long long total = (long long)valid_keys(a.src.seg, H, W, a.n) * PP;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const int j = (int)(g / PP), o = (int)(g - (long long)j * PP);
        const RowKey key = decode_key(a.src.sorted[j], W);
        const unsigned int i = key.i;
        if (i >= (unsigned int)a.n || key.p >= (long long)H * W) continue; // (not a key of this pass: nothing is written for it)
        float f0, f1;
        patch_entry<R>(a.src, key, a.src.ev[i].x, o, a.mode, a.tau, &f0, &f1);
        float *o_row = a.out + (long long)i * (2 * PP); // (64-bit: n * 2 * PP passes 2^31)
        o_row[o] = f0;
        o_row[PP + o] = f1;
    }
}

// valid[i] for every row, in row order, and the none values of the bad rows: the lanes of a wave share the work of its bad rows
__global__ __launch_bounds__(256) void k_patches_bad_rows(const float4 *__restrict__ ev, long long n, int H, int W, int PP, float none0,
                                                          float *__restrict__ out, unsigned char *__restrict__ valid)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool bad = false;
    if (i < n) {
        bad = row_pixel(ev[i], H, W) < 0;
        valid[i] = bad ? 0 : 1;
    }
    unsigned long long m = __ballot(bad);
    const long long i0 = i - lane;
    while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        float *o_row = out + (i0 + l) * (2 * PP);
        for (int e = lane; e < 2 * PP; e += 64) o_row[e] = e < PP ? none0 : 0.0f;
    }
}

// the maps of pixel p from its last row of the pass (behind k_patches_features on the stream: it read the maps as they were)
__global__ __launch_bounds__(256) void k_patches_map_update(const float4 *__restrict__ ev, const long long *__restrict__ sorted,
                                                            const int *__restrict__ seg, long long npx, float *__restrict__ last_t,
                                                            signed char *__restrict__ last_p)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < npx) map_update(ev, sorted, seg, p, last_t, last_p);
}

} // namespace

extern "C" {

int v2e_patches_features(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                         const int8_t *last_p, int radius, int mode, double tau, float *out, uint8_t *valid, void *stream)
{
    V2E_REQUIRE(n >= 0 && n <= 0x7fffffff && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && seg && last_t && last_p &&
                ((events && sorted_keys && out && valid) || n == 0), "bad args");
    V2E_REQUIRE(radius >= 1 && radius <= 3, "radius 1, 2 or 3");
    V2E_REQUIRE(mode == 0 || mode == 1, "mode 0 (age) or 1 (linear)");
    V2E_REQUIRE(mode == 0 || (tau > 0.0 && tau <= 1.7976931348623157e308), "linear mode: tau > 0 and finite");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0 && ((uintptr_t)out & 3u) == 0, "rows must be 16-byte aligned, out 4-byte aligned");
    if (n == 0) return 0;
    const int P = 2 * radius + 1, PP = P * P;
    PatchArgs a;
    a.src.ev = (const float4 *)events; a.src.sorted = (const long long *)sorted_keys; a.src.seg = seg; a.src.last_t = last_t;
    a.src.last_p = (const signed char *)last_p; a.src.H = H; a.src.W = W;
    a.n = (int)n; a.mode = mode; a.tau = tau; a.out = out; a.valid = valid;
    const int64_t want = (n * PP + 255) / 256;
    const int blocks = (int)(want < FEATURES_MAX_BLOCKS ? want : FEATURES_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    if (radius == 1) k_patches_features<1><<<blocks, 256, 0, s>>>(a);
    else if (radius == 2) k_patches_features<2><<<blocks, 256, 0, s>>>(a);
    else k_patches_features<3><<<blocks, 256, 0, s>>>(a);
    V2E_HIP(hipGetLastError());
    k_patches_bad_rows<<<v2e_cdiv(n, 256), 256, 0, s>>>((const float4 *)events, n, H, W, PP, mode ? 0.0f : __builtin_inff(), out, valid);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_patches_map_update(const float *events, const int64_t *sorted_keys, const int32_t *seg, int H, int W, float *last_t, int8_t *last_p,
                           void *stream)
{
    V2E_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && events && sorted_keys && seg && last_t && last_p, "bad args");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0, "rows must be 16-byte aligned");
    const int64_t npx = (int64_t)H * W;
    k_patches_map_update<<<v2e_cdiv(npx, 256), 256, 0, (hipStream_t)stream>>>((const float4 *)events, (const long long *)sorted_keys, seg, npx,
                                                                              last_t, (signed char *)last_p);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
