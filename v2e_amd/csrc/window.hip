// window.hip -- the fixed-window filter (FWF of the DND21 denoising benchmark) scored for every (L, sigma, k) in one pass over the
// rows of a device-resident run (host side: v2e_amd/window.py, WindowSweep).
//
// Rows are float4 (t, x = column, y = row, p), taken in row order; neither p nor the value of t is used.  A row is bad under
// rowkeys.h's row_pixel (t not finite, x / y not an integer value inside the sensor): it is only counted.  The valid rows of all
// passes form one stream v_0, v_1, ...; the window of v_m is v_{m-1} (depth 1) ... v_{m-D}, D = min(m, Lmax).  For a sigma and
// k = 1 .. 4, d = the smallest depth j at which k of the rows at depth 1 .. j lie within L1 distance sigma of the row (the same
// pixel counts), Lmax + 1 if the window holds fewer.  The row passes FWF(L, sigma, k) iff d <= L, so with bin(d) = the number of
// table lengths strictly below d (searchsorted 'left'; bin NL: passes none) hist[k-1][s][label][bin(d)] += 1 holds the ROC of
// every length of the table.  After its depths are read the row enters the window, whatever any filter says.
//
// The filter is serial only through "the last Lmax valid rows".  k_window_count / k_window_bases / k_window_compact write the
// packed words x | y << 16 of a pass's valid rows, in order, behind the Lmax words carried from the pass before (XY_NONE: no
// row yet), and beside them each valid row's index in the pass.  In k_window_depths a workgroup stages 256 consecutive words and
// the Lmax before them in LDS and every thread walks back from its own; every sum is an integer atomic (LDS int32 per workgroup,
// flushed with 64-bit global atomics), so the result depends on the row order only.  k_window_tail then carries the last Lmax
// words on.  The host never learns the number of valid rows: every kernel reads it from device memory.
#include "common.h"
#include "rowkeys.h"
#include "block_ops.h"

namespace {

constexpr int MAX_LENGTHS = 64, MAX_LENGTH = 1024, MAX_SIGMAS = 8, MAX_SUPPORT = 4;
constexpr int MAX_SLOTS = MAX_SIGMAS + 1;                   // the table's sigmas and the keep mask's own
constexpr unsigned int XY_NONE = 0xffffffffu;               // (x, y) = (65535, 65535): no sensor has that pixel (H, W <= 65535)
constexpr int SIGMA_MAX = 0x7ffffffe;                       // a sigma is clamped to this: XY_NONE's distance, 2^31 - 1, stays above it
constexpr int DEPTHS_MAX_BLOCKS = 2048;
constexpr int STOP_CHECK_EVERY = 16;                        // steps of the walk between two "has every lane all its depths" ballots
constexpr int WALK_UNROLL = 4;                              // steps whose words are read together; divides STOP_CHECK_EVERY
constexpr int WALK_PAD = STOP_CHECK_EVERY;                  // words in front of the staged stretch that the last steps may read

// the packed word of a valid row, XY_NONE for a bad one
__device__ __forceinline__ unsigned int row_word(const float4 e, int H, int W)
{
    if (row_pixel(e, H, W) < 0) return XY_NONE;
    return (unsigned int)(int)e.y | ((unsigned int)(int)e.z << 16);
}

// blk[b] = the valid rows among rows 256 b .. 256 b + 255; keep (or null) gets 0 at bad rows
__global__ __launch_bounds__(256) void k_window_count(const float4 *__restrict__ ev, long long n, int H, int W, int *__restrict__ blk,
                                                      unsigned char *__restrict__ keep)
{
    __shared__ int s[4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n && row_pixel(ev[i], H, W) >= 0;
    if (keep && i < n && !valid) keep[i] = 0;
    const int c = block_count(valid, s, 4);
    if (threadIdx.x == 0) blk[blockIdx.x] = c;
}

// One workgroup of 1024 threads: blk becomes its exclusive scan, n_valid[0] the pass's valid rows, which the counters take
// ([0] += valid, [1] += bad: the call's and the sweep's), and the carried tail becomes the first lmax words of xy.
__global__ __launch_bounds__(1024) void k_window_bases(int *__restrict__ blk, int nblk, long long n, const unsigned int *__restrict__ tail,
                                                       int lmax, unsigned int *__restrict__ xy, int *__restrict__ n_valid,
                                                       unsigned long long *__restrict__ call_cnt, unsigned long long *__restrict__ seen_cnt)
{
    __shared__ int s_part[1024];
    const int total = block_bases<int>(blk, nblk, s_part);
    if (threadIdx.x == 1023) {
        n_valid[0] = total;
        call_cnt[0] += (unsigned long long)total;
        call_cnt[1] += (unsigned long long)(n - total);
        seen_cnt[0] += (unsigned long long)total;
        seen_cnt[1] += (unsigned long long)(n - total);
    }
    if ((int)threadIdx.x < lmax) xy[threadIdx.x] = tail[threadIdx.x];
}

// valid row i, the r-th of the pass: xy[lmax + r] = its word, idx[r] = i
__global__ __launch_bounds__(256) void k_window_compact(const float4 *__restrict__ ev, long long n, int H, int W, const int *__restrict__ blk,
                                                        int lmax, unsigned int *__restrict__ xy, int *__restrict__ idx)
{
    __shared__ int s[4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned int w = i < n ? row_word(ev[i], H, W) : XY_NONE;
    const bool valid = w != XY_NONE;
    const int r = blk[blockIdx.x] + block_rank(valid, s);
    if (valid) {
        xy[lmax + r] = w;
        idx[r] = (int)i;
    }
}

struct DepthArgs {
    const unsigned int *xy;      // [lmax + n]: the carried tail, then the pass's valid rows
    const int *idx;              // [n]: the row of the pass behind each compacted word
    int n;                       // rows of this pass
    const int *n_valid;          // [1]
    const int *lengths;          // [NL] ascending, lengths[NL-1] = lmax
    int NL, lmax;
    int sigma[MAX_SLOTS];        // the table's sigmas; with a keep mask its own sigma behind them
    const unsigned char *labels; // [n]: 1 signal, 0 noise; or null
    const long long *lbounds;    // v2e_denoise_ages' table of bounds; or null
    int n_lbounds;
    long long row0;              // index in the whole call of this pass's row 0 (for lbounds)
    unsigned long long *hist;    // [4][S][2][NL+1]
    unsigned char *keep;         // [n] or null
    int keep_length, keep_k;
};

// NS: the sigmas walked, the keep mask's included.  Counters and depths live in registers: every index below is a constant once
// the loops over s and k are unrolled.  At step j lane t reads word lmax + t - j of the staged stretch: consecutive lanes,
// consecutive words.  Most steps of a sparse stream support no row of the wave: a ballot per sigma, largest first, skips them.
template <int NS> __global__ __launch_bounds__(256) void k_window_depths(DepthArgs r)
{
    extern __shared__ int s_mem[];
    const int lmax = r.lmax, NL = r.NL, nb = NL + 1;
    const int S = r.keep ? NS - 1 : NS;                        // the sigmas of the histogram
    const int nh = MAX_SUPPORT * S * 2 * nb;
    unsigned int *s_xy = (unsigned int *)s_mem + WALK_PAD;     // [lmax + 256], WALK_PAD words in front: read, never used
    int *s_len = s_mem + WALK_PAD + lmax + 256;                // [NL]
    int *s_hist = s_len + NL;                                  // [4][S][2][NL+1]
    const int tid = threadIdx.x;
    for (int j = tid; j < NL; j += 256) s_len[j] = r.lengths[j];
    for (int j = tid; j < nh; j += 256) s_hist[j] = 0;
    const int nv_dev = r.n_valid[0];
    const int nv = nv_dev < r.n ? nv_dev : r.n;                // no read past the pass's words, whatever n_valid holds
    const int tiles = (nv + 255) >> 8;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int base = tile << 8;
        __syncthreads(); // the walk before is over, the tables above are written
        for (int j = tid; j < lmax + 256; j += 256) s_xy[j] = base + j < lmax + nv ? r.xy[base + j] : XY_NONE;
        __syncthreads();
        const int row = base + tid;
        const bool active = row < nv;
        const unsigned int me = s_xy[lmax + tid];
        const int x = (int)(me & 0xffffu), y = (int)(me >> 16);
        int cnt[NS], d[NS][MAX_SUPPORT];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            cnt[s] = 0;
#pragma unroll
            for (int k = 0; k < MAX_SUPPORT; ++k) d[s][k] = lmax + 1;
        }
        for (int j0 = 1; j0 <= lmax; j0 += STOP_CHECK_EVERY) {
            for (int j = j0; j < j0 + STOP_CHECK_EVERY; j += WALK_UNROLL) {
                // the words of WALK_UNROLL steps are read before the first is used: a wave waits for the LDS once, not once per
                // step.  A step beyond lmax counts as "no row" whatever it reads: in the first lanes a word in front of s_xy
                unsigned int w[WALK_UNROLL];
#pragma unroll
                for (int u = 0; u < WALK_UNROLL; ++u) w[u] = s_xy[lmax + tid - j - u];
#pragma unroll
                for (int u = 0; u < WALK_UNROLL; ++u) {
                    const int dx = x - (int)(w[u] & 0xffffu), dy = y - (int)(w[u] >> 16);
                    const bool none = w[u] == XY_NONE || j + u > lmax;
                    const int dist = none ? 0x7fffffff : (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
                    // A step that supports no row of the wave for a sigma updates nothing for it, nor for the smaller ones: the
                    // table's sigmas ascend (the keep mask's own stands outside that order)
#pragma unroll
                    for (int s = NS - 1; s >= 0; --s) {
                        const bool hit = dist <= r.sigma[s];
                        if (__ballot(hit) == 0ull) {
                            if (s == NS - 1 && r.keep) continue;
                            break;
                        }
                        cnt[s] += hit ? 1 : 0;
#pragma unroll
                        for (int k = 0; k < MAX_SUPPORT; ++k) d[s][k] = (hit && cnt[s] == k + 1) ? j + u : d[s][k];
                    }
                }
            }
            bool more = false;
#pragma unroll
            for (int s = 0; s < NS; ++s) more = more || cnt[s] < MAX_SUPPORT;
            if (__ballot(active && more) == 0ull) break; // the wave's rows have all their depths
        }
        if (!active) continue;
        const int i = r.idx[row];
        const int label = row_label(r.labels, r.lbounds, r.n_lbounds, r.row0, i);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s >= S) continue;
            int b = 0; // the depths ascend with k: each search starts at the bin before
#pragma unroll
            for (int k = 0; k < MAX_SUPPORT; ++k) {
                b = count_lt<int>(s_len, NL, d[s][k], b);
                atomicAdd(&s_hist[((k * S + s) * 2 + label) * nb + b], 1);
            }
        }
        if (r.keep) {
            int dk = d[NS - 1][0];
#pragma unroll
            for (int k = 1; k < MAX_SUPPORT; ++k) dk = (k == r.keep_k - 1) ? d[NS - 1][k] : dk;
            r.keep[i] = dk <= r.keep_length ? 1 : 0;
        }
    }
    __syncthreads();
    for (int j = tid; j < nh; j += 256) {
        const int v = s_hist[j];
        if (v) atomicAdd(&r.hist[j], (unsigned long long)v);
    }
}

// tail = the last lmax words of xy (its own buffer: k_window_depths of the same pass read xy, the next pass reads tail)
__global__ __launch_bounds__(256) void k_window_tail(const unsigned int *__restrict__ xy, const int *__restrict__ n_valid, int n, int lmax,
                                                     unsigned int *__restrict__ tail)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int nv = n_valid[0] < n ? n_valid[0] : n;
    if (j < lmax) tail[j] = xy[nv + j];
}

template <int NS> void launch_depths(const DepthArgs &r, int blocks, size_t lds, hipStream_t stream)
{
    k_window_depths<NS><<<blocks, 256, lds, stream>>>(r);
}

} // namespace

extern "C" {

int v2e_window_compact(const float *events, int64_t n, int H, int W, const uint32_t *tail, int lmax, uint32_t *xy, int32_t *idx,
                       int32_t *blk, int32_t *n_valid, uint64_t *call_counters, uint64_t *seen_counters, uint8_t *keep, void *stream)
{
    V2E_REQUIRE(n >= 1 && n <= (1 << 30) && H > 0 && W > 0 && H <= 65535 && W <= 65535, "1 to 2^30 rows, a sensor of at most 65535 x 65535");
    V2E_REQUIRE(lmax >= 1 && lmax <= MAX_LENGTH, "the longest window is 1 to 1024 rows");
    V2E_REQUIRE(events && tail && xy && idx && blk && n_valid && call_counters && seen_counters, "bad args");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0, "rows must be 16-byte aligned");
    const int nblk = v2e_cdiv(n, 256);
    hipStream_t s = (hipStream_t)stream;
    k_window_count<<<nblk, 256, 0, s>>>((const float4 *)events, n, H, W, blk, keep);
    k_window_bases<<<1, 1024, 0, s>>>(blk, nblk, n, tail, lmax, xy, n_valid, (unsigned long long *)call_counters,
                                      (unsigned long long *)seen_counters);
    k_window_compact<<<nblk, 256, 0, s>>>((const float4 *)events, n, H, W, blk, lmax, xy, idx);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_window_depths(const uint32_t *xy, const int32_t *idx, int64_t n, const int32_t *n_valid, const int32_t *lengths, int n_lengths,
                      int lmax, const int32_t *sigmas, int n_sigmas, const uint8_t *labels, const int64_t *label_bounds,
                      int n_label_bounds, int64_t row0, uint64_t *hist, uint8_t *keep, int keep_length, int64_t keep_sigma, int keep_k,
                      void *stream)
{
    V2E_REQUIRE(n >= 1 && n <= (1 << 30) && xy && idx && n_valid && lengths && sigmas && hist && row0 >= 0, "bad args");
    V2E_REQUIRE(n_lengths >= 1 && n_lengths <= MAX_LENGTHS && lmax >= 1 && lmax <= MAX_LENGTH, "1 to 64 lengths, the longest 1 to 1024");
    V2E_REQUIRE(n_sigmas >= 1 && n_sigmas <= MAX_SIGMAS, "1 to 8 sigmas");
    V2E_REQUIRE_LABELS(labels, label_bounds, n_label_bounds);
    V2E_REQUIRE(!keep || (keep_length >= 1 && keep_length <= lmax && keep_sigma >= 0 && keep_k >= 1 && keep_k <= MAX_SUPPORT),
                "keep: L in 1 .. the longest length, sigma >= 0, k in 1 .. 4");
    DepthArgs r;
    r.xy = xy; r.idx = idx; r.n = (int)n; r.n_valid = n_valid; r.lengths = lengths; r.NL = n_lengths; r.lmax = lmax;
    for (int s = 0; s < MAX_SLOTS; ++s) r.sigma[s] = -1;
    for (int s = 0; s < n_sigmas; ++s) {
        V2E_REQUIRE(sigmas[s] >= 0 && sigmas[s] <= 65535 && (s == 0 || sigmas[s] > sigmas[s - 1]), "sigmas: 0 .. 65535, strictly ascending");
        r.sigma[s] = sigmas[s];
    }
    if (keep) r.sigma[n_sigmas] = keep_sigma < SIGMA_MAX ? (int)keep_sigma : SIGMA_MAX;
    r.labels = labels; r.lbounds = (const long long *)label_bounds; r.n_lbounds = label_bounds ? n_label_bounds : 0; r.row0 = row0;
    r.hist = (unsigned long long *)hist; r.keep = keep; r.keep_length = keep_length; r.keep_k = keep_k;
    const size_t lds = ((size_t)WALK_PAD + lmax + 256 + n_lengths + (size_t)MAX_SUPPORT * n_sigmas * 2 * (n_lengths + 1)) * 4;
    const int64_t tiles = (n + 255) / 256;
    const int blocks = (int)(tiles < DEPTHS_MAX_BLOCKS ? tiles : DEPTHS_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    switch (n_sigmas + (keep ? 1 : 0)) {
    case 1: launch_depths<1>(r, blocks, lds, s); break;
    case 2: launch_depths<2>(r, blocks, lds, s); break;
    case 3: launch_depths<3>(r, blocks, lds, s); break;
    case 4: launch_depths<4>(r, blocks, lds, s); break;
    case 5: launch_depths<5>(r, blocks, lds, s); break;
    case 6: launch_depths<6>(r, blocks, lds, s); break;
    case 7: launch_depths<7>(r, blocks, lds, s); break;
    case 8: launch_depths<8>(r, blocks, lds, s); break;
    default: launch_depths<9>(r, blocks, lds, s); break;
    }
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_window_tail(const uint32_t *xy, const int32_t *n_valid, int64_t n, int lmax, uint32_t *tail, void *stream)
{
    V2E_REQUIRE(n >= 1 && n <= (1 << 30) && lmax >= 1 && lmax <= MAX_LENGTH && xy && n_valid && tail, "bad args");
    k_window_tail<<<v2e_cdiv(lmax, 256), 256, 0, (hipStream_t)stream>>>(xy, n_valid, (int)n, lmax, tail);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
