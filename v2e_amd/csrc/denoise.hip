// denoise.hip -- the spatio-temporal correlation filter (STCF; with one supporting neighbour jAER's background-activity filter)
// scored for every (k, tau) in one pass over the rows of a device-resident run (host side: v2e_amd/denoise.py, DenoiseSweep).
//
// Rows are float4 (t, x = column, y = row, p), processed in row order; p is not read.  A row is bad if t is not finite or x / y
// is not an integer value inside the sensor: it reads and writes nothing and is only counted.  For a valid row i at pixel (x, y)
// each of the 8 neighbours q (centre excluded) inside the sensor gives age_q = (double)t_i - (double)T_q, T_q the t of the latest
// row j < i at q in this call, else the carried last_t[q] (-inf: none yet, age +inf; a neighbour outside the sensor: +inf; a T_q
// later than t_i: a negative age, kept).  a_1 <= ... <= a_8 are the ages sorted; the row passes STCF(k, tau) iff a_k <= tau, so
// hist[k-1][label][bin(a_k)] += 1 with bin(a) = the number of taus strictly below a (searchsorted 'left'; bin T: passes none)
// holds the ROC of all 8 * T filters.  Then last_t[x,y] = t_i, whatever the filters say.
//
// The filter is serial only through "the latest earlier row at pixel q".  k_denoise_keys gives row i the key pixel << 32 | i
// (a bad row KEY_BAD, above every other); the host sorts the keys; k_denoise_segments finds each pixel's stretch of the sorted
// keys; in k_denoise_ages that lookup is rowkeys.h's latest_before, a binary search of q's stretch.  Every row is then
// independent of the others, every sum is an integer atomic (LDS int32 per workgroup, flushed with 64-bit global atomics), and
// the result does not depend on how threads are scheduled or how a clip is cut into calls.
#include "common.h"
#include "rowkeys.h"

namespace {

constexpr int MAX_TAUS = 256;
constexpr int LDS_LABEL_BOUNDS_MAX = 2048;                  // label bounds staged in LDS up to this many entries (16 KB)
constexpr int AGES_MAX_BLOCKS = 2048;                       // (keys, stretches and the lookup in them: rowkeys.h)

__global__ __launch_bounds__(256) void k_denoise_keys(const float4 *__restrict__ ev, long long n, int H, int W, long long *__restrict__ keys,
                                                      unsigned char *__restrict__ keep)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long p = row_pixel(ev[i], H, W);
    keys[i] = p < 0 ? KEY_BAD : ((p << 32) | i);
    if (keep && p < 0) keep[i] = 0;
}

// seg[p] = the number of sorted keys below p << 32, p = 0 .. npx: pixel p's rows are sorted[seg[p] .. seg[p+1]), in row order, and
// seg[npx] is the number of valid rows.  counters (or null): [0] += valid rows, [1] += bad rows.
__global__ __launch_bounds__(256) void k_denoise_segments(const long long *__restrict__ sorted, int n, long long npx, int *__restrict__ seg,
                                                          unsigned long long *__restrict__ counters)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p > npx) return;
    const int a = count_lt<long long>(sorted, n, p << 32);
    seg[p] = a;
    if (p == npx && counters) {
        if (a) atomicAdd(&counters[0], (unsigned long long)a);
        if (n - a) atomicAdd(&counters[1], (unsigned long long)(n - a));
    }
}

struct AgesArgs {
    const float4 *ev;
    int n;                       // rows of this pass
    int H, W;
    const long long *sorted;     // the sorted keys
    const int *seg;              // [H*W + 1]
    const float *last_t;         // [H*W], the carried map (read only here)
    const double *taus;
    int T;
    const unsigned char *labels; // [n]: 1 signal, 0 noise; or null
    const long long *lbounds;    // ascending row indices (of the whole call): frame f's signal rows start at lbounds[2f], its noise
    int n_lbounds;               //   rows at lbounds[2f+1]; a row is signal iff an odd number of entries is <= its index; or null
    long long row0;              // index in the whole call of this pass's row 0 (for lbounds)
    unsigned long long *hist;    // [8][2][T+1]
    unsigned char *keep;         // [n] or null
    int keep_k;                  // 1 .. 8
    double keep_tau;
};

__device__ __forceinline__ void cswap(double &a, double &b)
{
    const double lo = a < b ? a : b, hi = a < b ? b : a; // (no NaN can occur: t_i is finite, T_q finite or -inf)
    a = lo; b = hi;
}

// Thread j takes the row of sorted key j, so that neighbouring threads search neighbouring stretches and long stretches stay in
// cache; the row itself is gathered.  (Threads in row order -- coalesced row reads, scattered searches -- measured slower: 34
// against 29 us on 137 k rows, 2.9 against 0.98 ms per pass on 4.4 M rows, profiles/r15_denoise_sweep.txt.)
__global__ __launch_bounds__(256) void k_denoise_ages(AgesArgs r)
{
    extern __shared__ double s_mem[];
    double *s_taus = s_mem;                                   // [T]
    long long *s_lb = (long long *)(s_mem + r.T);             // [n_lbounds] when staged
    const bool lb_lds = r.lbounds && r.n_lbounds <= LDS_LABEL_BOUNDS_MAX;
    int *s_hist = (int *)(s_lb + (lb_lds ? r.n_lbounds : 0)); // [8][2][T+1]
    const int T = r.T, nb = T + 1, nh = 16 * nb;
    for (int j = threadIdx.x; j < T; j += 256) s_taus[j] = r.taus[j];
    if (lb_lds) for (int j = threadIdx.x; j < r.n_lbounds; j += 256) s_lb[j] = r.lbounds[j];
    for (int j = threadIdx.x; j < nh; j += 256) s_hist[j] = 0;
    __syncthreads();
    const long long *lb = lb_lds ? s_lb : r.lbounds;
    const int W = r.W, H = r.H;
    const int n_valid = valid_keys(r.seg, H, W, r.n);

    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n_valid; j += (long long)gridDim.x * 256) {
        const RowKey key = decode_key(r.sorted[j], W);
        const unsigned int i = key.i;
        const double t = (double)r.ev[i].x;
        double a[8];
        int m = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dx == 0 && dy == 0) continue;
                double age = __longlong_as_double(0x7ff0000000000000LL); // +inf
                const int qx = key.x + dx, qy = key.y + dy;
                if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                    const long long q = key.p + (long long)dy * W + dx;
                    unsigned int j_q;
                    const float tq = latest_before(r.sorted, r.seg, q, i, &j_q) ? r.ev[j_q].x : r.last_t[q];
                    age = t - (double)tq; // (tq = -inf: +inf)
                }
                a[m++] = age;
            }
        }
        // 19 exchanges in 6 layers (the smallest network for 8 keys)
        cswap(a[0], a[2]); cswap(a[1], a[3]); cswap(a[4], a[6]); cswap(a[5], a[7]);
        cswap(a[0], a[4]); cswap(a[1], a[5]); cswap(a[2], a[6]); cswap(a[3], a[7]);
        cswap(a[0], a[1]); cswap(a[2], a[3]); cswap(a[4], a[5]); cswap(a[6], a[7]);
        cswap(a[2], a[4]); cswap(a[3], a[5]);
        cswap(a[1], a[4]); cswap(a[3], a[6]);
        cswap(a[1], a[2]); cswap(a[3], a[4]); cswap(a[5], a[6]);

        const int label = row_label(r.labels, lb, r.n_lbounds, r.row0, i);
        int b = 0; // the bins ascend with k: each search starts at the bin before
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            b = count_lt<double>(s_taus, T, a[k], b);
            atomicAdd(&s_hist[(k * 2 + label) * nb + b], 1);
        }
        if (r.keep) {
            double ak = a[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) ak = (k == r.keep_k - 1) ? a[k] : ak;
            r.keep[i] = ak <= r.keep_tau ? 1 : 0;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nh; j += 256) {
        const int v = s_hist[j];
        if (v) atomicAdd(&r.hist[j], (unsigned long long)v);
    }
}

// last_t[p] = the t of pixel p's last row of the pass (behind k_denoise_ages on the stream: it read the map as it was)
__global__ __launch_bounds__(256) void k_denoise_map_update(const float4 *__restrict__ ev, const long long *__restrict__ sorted,
                                                            const int *__restrict__ seg, long long npx, float *__restrict__ last_t)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < npx) map_update(ev, sorted, seg, p, last_t, nullptr);
}

} // namespace

extern "C" {

int v2e_denoise_keys(const float *events, int64_t n, int H, int W, int64_t *keys, uint8_t *keep, void *stream)
{
    V2E_REQUIRE(n >= 0 && n <= 0x7fffffff && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && ((events && keys) || n == 0), "bad args");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0 && ((uintptr_t)keys & 7u) == 0, "rows must be 16-byte aligned, keys 8-byte aligned");
    if (n == 0) return 0;
    k_denoise_keys<<<v2e_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>((const float4 *)events, n, H, W, (long long *)keys, keep);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_denoise_segments(const int64_t *sorted_keys, int64_t n, int H, int W, int32_t *seg, uint64_t *counters, void *stream)
{
    V2E_REQUIRE(n >= 0 && n <= 0x7fffffff && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && seg && (sorted_keys || n == 0), "bad args");
    const int64_t npx = (int64_t)H * W;
    k_denoise_segments<<<v2e_cdiv(npx + 1, 256), 256, 0, (hipStream_t)stream>>>((const long long *)sorted_keys, (int)n, npx, seg,
                                                                                (unsigned long long *)counters);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_denoise_ages(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                     const double *taus, int n_taus, const uint8_t *labels, const int64_t *label_bounds, int n_label_bounds,
                     int64_t row0, uint64_t *hist, uint8_t *keep, int keep_k, double keep_tau, void *stream)
{
    V2E_REQUIRE(n >= 0 && n <= 0x7fffffff && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && ((events && sorted_keys) || n == 0) && seg &&
                last_t && taus && hist && row0 >= 0, "bad args");
    V2E_REQUIRE(n_taus >= 1 && n_taus <= MAX_TAUS, "1 to 256 taus");
    V2E_REQUIRE_LABELS(labels, label_bounds, n_label_bounds);
    V2E_REQUIRE(!keep || (keep_k >= 1 && keep_k <= 8 && keep_tau >= 0.0), "keep: k in 1 .. 8 and tau >= 0");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0, "rows must be 16-byte aligned");
    if (n == 0) return 0;
    AgesArgs r;
    r.ev = (const float4 *)events; r.n = (int)n; r.H = H; r.W = W; r.sorted = (const long long *)sorted_keys; r.seg = seg;
    r.last_t = last_t; r.taus = taus; r.T = n_taus; r.labels = labels; r.lbounds = (const long long *)label_bounds;
    r.n_lbounds = label_bounds ? n_label_bounds : 0; r.row0 = row0; r.hist = (unsigned long long *)hist; r.keep = keep;
    r.keep_k = keep_k; r.keep_tau = keep_tau;
    const bool lb_lds = label_bounds && n_label_bounds <= LDS_LABEL_BOUNDS_MAX;
    const size_t lds = (size_t)n_taus * 8 + (lb_lds ? (size_t)n_label_bounds * 8 : 0) + (size_t)16 * (n_taus + 1) * 4;
    const int64_t blocks = (n + 255) / 256;
    k_denoise_ages<<<(int)(blocks < AGES_MAX_BLOCKS ? blocks : AGES_MAX_BLOCKS), 256, lds, (hipStream_t)stream>>>(r);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_denoise_map_update(const float *events, const int64_t *sorted_keys, const int32_t *seg, int H, int W, float *last_t, void *stream)
{
    V2E_REQUIRE(H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && events && sorted_keys && seg && last_t, "bad args");
    const int64_t npx = (int64_t)H * W;
    k_denoise_map_update<<<v2e_cdiv(npx, 256), 256, 0, (hipStream_t)stream>>>((const float4 *)events, (const long long *)sorted_keys, seg, npx,
                                                                              last_t);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
