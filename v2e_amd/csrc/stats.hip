// stats.hip -- a stream's own statistics: per-pixel counts, same-pixel inter-event intervals and time-bin counts of the rows of
// device-resident runs (host side: v2e_amd/stats.py, EventStats).
//
// Rows are float4 (t, x = column, y = row, p), taken in row order.  A row is bad under exactly rowkeys.h's rule: t not finite, or
// x / y not an integer value inside [0,W) / [0,H); it is only counted (v2e_denoise_segments) and touches nothing.  A valid row is ON
// iff p > 0 (EventPatches' rule).  Its label is 1 (signal) or 0 (noise): labels[i] != 0, or an odd number of label_bounds entries
// <= row0 + i (k_denoise_ages' two forms), or 1 with neither.  With c = 2 * label + ON:
//   count[c][y][x] += 1 for every valid row, whatever the ROI and the time bounds are.
// Everything below counts the valid rows with x0 <= x <= x1 and y0 <= y <= y1 only (the carried maps are stamped by every valid row):
//   Intervals.  The previous event of row i is the latest valid row j < i at the same pixel in this pass, else the carried
//   last_t[y][x] (float32, starts at -inf: none) / last_p[y][x] (int8 +-1, starts at 0) -- EventPatches' centre entry.  None:
//   n_first[c] += 1.  Otherwise d = (double)t_i - (double)T_prev, kept when negative, tr = 2 * (previous ON) + ON, and
//   isi_hist[label][tr][the number of edges <= d] += 1 (searchsorted 'right'; E edges, E + 1 bins); d < 0 also counts in
//   n_backwards[label]; min_isi[label][tr] is the smallest d >= 0, a 64-bit unsigned minimum of the bit pattern (which orders the
//   non-negative doubles).
//   Time bins.  With a table of K + 1 ascending bounds, k = (the number of bounds <= (double)t) - 1; time_hist[c][k] += 1 for
//   0 <= k < K, else n_before += 1 (k < 0) or n_after += 1.
//   t_first / t_last: the smallest and largest t of ALL valid rows, as 32-bit unsigned minimum / maximum of float_key(t), an
//   order-preserving transform of the float's bits.
//
// Thread j takes sorted key j (rowkeys.h: pixel << 32 | row, sorted), so the previous event at its pixel is sorted key j - 1 when
// that has the same pixel and the carried map otherwise: no search.  Every sum is an integer atomic, so the result depends on the
// row order alone, not on scheduling or on how a clip is cut.  Per workgroup in LDS, flushed with 64-bit global atomics: the interval
// histogram, n_first, n_backwards, n_before, n_after (each summed per wave with a ballot first), the minima and the extremes.
// Straight to memory: the count map and the time histogram.  Workgroup b adds to copy b % R of the time histogram and flushes to
// copy b % R' of the interval histogram, and the caller sums the copies: rows in pixel order scatter over all time bins, and with
// one copy every row was a contended atomic on one of a few hundred words -- 120 us of kernel time against 28 on 137 k rows.
// A pixel's rows are adjacent in thread order: the first lane of each run of equal pixels in a wave adds the run's four counts
// (ballots and popcounts) instead of every lane adding 1 -- 0.82 against 1.09 ms on 4.4 M rows, 1.2 against 26.8 ms with all of them
// on one pixel.  (All four measured, profiles/r22_event_stats.txt; only the faster forms were kept.)
#include "common.h"
#include "rowkeys.h"

namespace {

constexpr int MAX_EDGES = 256;
constexpr int ROWS_MAX_BLOCKS = 2048;
constexpr unsigned long long INF_BITS = 0x7ff0000000000000ULL;

// the layout of sums[]: uint64 words
enum { S_FIRST = 0, S_BACK = 4, S_BEFORE = 6, S_AFTER = 7, S_MIN = 8, S_TFIRST = 16, S_TLAST = 17, S_WORDS = 18 };

struct StatsArgs {
    const float4 *ev;
    int n;                        // rows of this pass
    int H, W;
    const long long *sorted;      // the sorted keys
    const int *seg;               // [H*W + 1]
    const float *last_t;          // [H*W], the carried maps (read only here)
    const signed char *last_p;    // [H*W]
    int x0, x1, y0, y1;           // the ROI, inclusive
    const double *edges;          // [E]
    int E;
    const double *bounds;         // [K + 1] or null
    int K;
    const unsigned char *labels;  // [n] or null
    const long long *lbounds;     // k_denoise_ages' table or null
    int n_lbounds;
    long long row0;
    unsigned long long *count;    // [4][H*W]
    unsigned long long *isi_hist; // [isi_replicas][2][4][E+1]
    unsigned long long *time_hist;// [time_replicas][4][K]
    int isi_replicas, time_replicas;
    unsigned long long *sums;     // [S_WORDS]
};

// unsigned keys that order like the floats they come from (no NaN reaches here)
__device__ __forceinline__ unsigned int float_key(float v)
{
    const unsigned int u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_stats_rows(StatsArgs a)
{
    __shared__ double s_edges[MAX_EDGES];
    __shared__ int s_hist[8 * (MAX_EDGES + 1)];
    __shared__ unsigned long long s_min[8];
    __shared__ int s_cnt[8];                                  // n_first[4], n_backwards[2], n_before, n_after
    __shared__ unsigned int s_text[2];                        // keys of t_first, t_last
    const int E = a.E, nb = E + 1, nh = 8 * nb;
    for (int j = threadIdx.x; j < E; j += 256) s_edges[j] = a.edges[j];
    for (int j = threadIdx.x; j < nh; j += 256) s_hist[j] = 0;
    if (threadIdx.x < 8) { s_min[threadIdx.x] = INF_BITS; s_cnt[threadIdx.x] = 0; }
    if (threadIdx.x == 0) { s_text[0] = 0xffffffffu; s_text[1] = 0u; }
    __syncthreads();
    const int W = a.W, H = a.H, lane = threadIdx.x & 63;
    const long long npx = (long long)H * W;
    const int n_valid = valid_keys(a.seg, H, W, a.n);
    unsigned int t_lo = 0xffffffffu, t_hi = 0u;               // this thread's extremes (keys)
    unsigned long long *time_hist = a.time_hist + (long long)(blockIdx.x % a.time_replicas) * 4 * a.K;

    // (whole workgroups go round the loop together: the ballots below need every lane of a wave)
    for (long long base = (long long)blockIdx.x * 256; base < n_valid; base += (long long)gridDim.x * 256) {
        const long long j = base + threadIdx.x;
        bool active = j < n_valid;
        RowKey key = {0u, 0, 0, 0};
        if (active) {
            key = decode_key(a.sorted[j], W);
            active = key.i < (unsigned int)a.n && key.p < npx; // (not a key of this pass: nothing is read or written for it)
        }
        float4 e = {0.0f, 0.0f, 0.0f, 0.0f};
        int label = 1;
        if (active) {
            e = a.ev[key.i];
            label = row_label(a.labels, a.lbounds, a.n_lbounds, a.row0, key.i);
        }
        const int on = e.w > 0.0f ? 1 : 0, c = 2 * label + on;

        // the count map: the first lane of a run of equal pixels adds the run's rows, lanes [lane, end), cell by cell
        const int pi = active ? (int)key.p : -1;
        const int before = __shfl_up(pi, 1);
        const bool head = active && (lane == 0 || before != pi);
        const unsigned long long cuts = __ballot(head || !active);
        const unsigned long long above = lane == 63 ? 0ull : cuts & ~((2ull << lane) - 1ull);
        const int end = above ? __ffsll((long long)above) - 1 : 64;
        const unsigned long long run = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const unsigned long long m = __ballot(active && c == cc);
            const int v = __popcll(m & run);
            if (head && v) atomicAdd(&a.count[cc * npx + key.p], (unsigned long long)v);
        }
        if (active) {
            const unsigned int tk = float_key(e.x);
            t_lo = tk < t_lo ? tk : t_lo;
            t_hi = tk > t_hi ? tk : t_hi;
        }
        int cnt_time = -1, cnt_isi = -1;                      // the cells of s_cnt this row counts in: 6 / 7 and 0 .. 5
        if (active && key.x >= a.x0 && key.x <= a.x1 && key.y >= a.y0 && key.y <= a.y1) {
            const double t = (double)e.x;
            if (a.bounds) {
                const int k = count_le<double>(a.bounds, a.K + 1, t) - 1;
                if (k < 0) cnt_time = 6;
                else if (k >= a.K) cnt_time = 7;
                else atomicAdd(&time_hist[(long long)c * a.K + k], 1ull);
            }
            float tp;
            int pon;
            if (j > 0 && (a.sorted[j - 1] >> 32) == key.p) {
                const float4 q = a.ev[(unsigned int)a.sorted[j - 1]];
                tp = q.x;
                pon = q.w > 0.0f ? 1 : 0;
            } else {
                tp = a.last_t[key.p];
                pon = a.last_p[key.p] > 0 ? 1 : 0;
            }
            if (tp == -__builtin_inff()) {
                cnt_isi = c;
            } else {
                const double d = t - (double)tp;
                const int tr = 2 * pon + on;
                atomicAdd(&s_hist[(label * 4 + tr) * nb + count_le<double>(s_edges, E, d)], 1);
                if (d < 0.0) {
                    cnt_isi = 4 + label;
                } else {
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
                    volatile unsigned long long *seen = &s_min[label * 4 + tr]; // (it only falls: a stale value costs one atomic)
                    if (bits < *seen) atomicMin(&s_min[label * 4 + tr], bits);
                }
            }
        }
        // n_first, n_backwards, n_before, n_after: one LDS atomic per wave and cell instead of one per row
#pragma unroll
        for (int cell = 0; cell < 8; ++cell) {
            const int v = __popcll(__ballot(cnt_time == cell || cnt_isi == cell));
            if (lane == 0 && v) atomicAdd(&s_cnt[cell], v);
        }
    }
    if (t_hi != 0u) {
        atomicMin(&s_text[0], t_lo);
        atomicMax(&s_text[1], t_hi);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nh; j += 256) {
        const int v = s_hist[j];
        if (v) atomicAdd(&a.isi_hist[(long long)(blockIdx.x % a.isi_replicas) * nh + j], (unsigned long long)v);
    }
    if (threadIdx.x < 8) {
        const int v = s_cnt[threadIdx.x];
        if (v) atomicAdd(&a.sums[S_FIRST + threadIdx.x], (unsigned long long)v);
        if (s_min[threadIdx.x] != INF_BITS) atomicMin(&a.sums[S_MIN + threadIdx.x], s_min[threadIdx.x]);
    }
    if (threadIdx.x == 0 && s_text[1] != 0u) {
        atomicMin(&a.sums[S_TFIRST], (unsigned long long)s_text[0]);
        atomicMax(&a.sums[S_TLAST], (unsigned long long)s_text[1]);
    }
}

// the maps of pixel p from its last row of the pass (behind k_stats_rows on the stream: it read the maps as they were)
__global__ __launch_bounds__(256) void k_stats_map_update(const float4 *__restrict__ ev, const long long *__restrict__ sorted,
                                                          const int *__restrict__ seg, long long npx, float *__restrict__ last_t,
                                                          signed char *__restrict__ last_p)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < npx) map_update(ev, sorted, seg, p, last_t, last_p);
}

} // namespace

extern "C" {

int v2e_stats_rows(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                   const int8_t *last_p, int x0, int x1, int y0, int y1, const double *isi_edges, int n_edges, const double *time_bounds,
                   int n_bins, const uint8_t *labels, const int64_t *label_bounds, int n_label_bounds, int64_t row0, uint64_t *count,
                   uint64_t *isi_hist, int isi_replicas, uint64_t *time_hist, int time_replicas, uint64_t *sums, void *stream)
{
    V2E_REQUIRE(n >= 0 && n <= 0x7fffffff && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && ((events && sorted_keys) || n == 0) && seg &&
                last_t && last_p && isi_edges && count && isi_hist && sums && row0 >= 0, "bad args");
    V2E_REQUIRE(0 <= x0 && x0 <= x1 && x1 < W && 0 <= y0 && y0 <= y1 && y1 < H, "the ROI must lie inside the sensor");
    V2E_REQUIRE(n_edges >= 1 && n_edges <= MAX_EDGES, "1 to 256 interval edges");
    V2E_REQUIRE(time_bounds ? (n_bins >= 1 && n_bins <= (1 << 20) && time_hist) : n_bins == 0, "time bounds: 1 to 2^20 bins, or none");
    V2E_REQUIRE(isi_replicas >= 1 && time_replicas >= 1 && isi_replicas <= ROWS_MAX_BLOCKS && time_replicas <= ROWS_MAX_BLOCKS,
                "1 to 2048 replicas of each histogram");
    V2E_REQUIRE_LABELS(labels, label_bounds, n_label_bounds);
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0, "rows must be 16-byte aligned");
    if (n == 0) return 0;
    StatsArgs a;
    a.ev = (const float4 *)events; a.n = (int)n; a.H = H; a.W = W; a.sorted = (const long long *)sorted_keys; a.seg = seg;
    a.last_t = last_t; a.last_p = (const signed char *)last_p; a.x0 = x0; a.x1 = x1; a.y0 = y0; a.y1 = y1; a.edges = isi_edges;
    a.E = n_edges; a.bounds = time_bounds; a.K = n_bins; a.labels = labels; a.lbounds = (const long long *)label_bounds;
    a.n_lbounds = label_bounds ? n_label_bounds : 0; a.row0 = row0; a.count = (unsigned long long *)count;
    a.isi_hist = (unsigned long long *)isi_hist; a.time_hist = (unsigned long long *)time_hist; a.sums = (unsigned long long *)sums;
    a.isi_replicas = isi_replicas; a.time_replicas = time_replicas;
    const int64_t blocks = (n + 255) / 256;
    k_stats_rows<<<(int)(blocks < ROWS_MAX_BLOCKS ? blocks : ROWS_MAX_BLOCKS), 256, 0, (hipStream_t)stream>>>(a);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_stats_map_update(const float *events, const int64_t *sorted_keys, const int32_t *seg, int H, int W, float *last_t, int8_t *last_p,
                         void *stream)
{
    V2E_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && events && sorted_keys && seg && last_t && last_p, "bad args");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0, "rows must be 16-byte aligned");
    const int64_t npx = (int64_t)H * W;
    k_stats_map_update<<<v2e_cdiv(npx, 256), 256, 0, (hipStream_t)stream>>>((const float4 *)events, (const long long *)sorted_keys, seg, npx,
                                                                            last_t, (signed char *)last_p);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
