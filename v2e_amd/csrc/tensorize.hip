// tensorize.hip -- dense event tensors from the rows of a device-resident run: per-polarity count images, voxel grids with
// bilinear time weights, time surfaces (host side: v2e_amd/tensors.py, EventTensorizer).
//
// Rows are float4 (t, x = column, y = row, p = +-1), in any order.  A launch covers `nk` consecutive windows of the clip, the
// last of which may be the clip's open window (the one the run ends in): its accumulators are the carried planes of the
// tensorizer, every other window's plane lies in the launch's output.  Window k = [B_k, B_k+1), float64 throughout:
//   uniform   B_k = t_start + (double)k * window_s (one product, one sum; the library is built with -ffp-contract=off), k from
//             floor((t - t_start) / window_s), corrected by +-1 against B_k and B_k+1
//   explicit  an ascending float64 table, table_search.h's count_le (staged in LDS when it fits)
// so that k == searchsorted(B, t, 'right') - 1 in both.  A row takes part if x / y is a coordinate of the sensor (rowkeys.h:
// pixel_coord), p is +-1 and t is not NaN.
//
// All scattered updates are no-return INTEGER atomics, so the result does not depend on the order the rows arrive in: count adds 1
// to an int32, voxel adds +-q (the bilinear weight in units of 2^-24) to an int64, the time surface takes the maximum of an
// order-preserving uint32 key of the float32 time stamp.  The finish kernels turn the voxel sums into float32 and the keys,
// by a running maximum over the windows, into time stamps.  Everything is enqueued on the caller's stream.
#include "common.h"
#include "block_ops.h"
#include "rowkeys.h"

namespace {

constexpr int LDS_BOUNDS_MAX = 4096;                       // explicit bounds staged in LDS up to this many entries (32 KB)
constexpr int SCATTER_MAX_BLOCKS = 4096;                   // k_tensorize_scatter's grid: more rows than this holds take further trips
constexpr unsigned int KEY_NEG_INF = 0x007fffffu;          // surf_key(-inf): what a pixel without an event holds
constexpr double Q_ONE = 16777216.0;                       // 2^24: voxel weights are integers in units of 2^-24

// order-preserving key of a float: a < b  <=>  surf_key(a) < surf_key(b), negative values included; 0 lies below every key
__device__ __forceinline__ unsigned int surf_key(float t)
{
    const unsigned int u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float surf_time(unsigned int key)
{
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

struct ScatterArgs {
    const float4 *ev;
    long long n;
    int H, W;
    int uniform;
    double t_start, window_s;
    const double *bounds;      // explicit: B of the launch's first window at bounds[0], nk + 1 entries
    long long k0;              // uniform: clip index of the launch's first window
    int nk;                    // windows of this launch, the open one included
    int open_k;                // launch-local index of the open window (nk - 1), or -1
    int *count, *count_open;   // [.,2,H,W] planes of the complete windows / the carried plane of the open one
    long long *vox, *vox_open; // [v_b - v_a,B,H,W] / [B,H,W]
    int v_a, v_b;              // launch-local complete windows this launch's voxel scratch holds
    int B;
    unsigned int *surf, *surf_open;
    unsigned long long *counters; // n_bad, n_before, n_after; or null
};

__global__ __launch_bounds__(256) void k_tensorize_scatter(ScatterArgs r)
{
    extern __shared__ double s_bounds[];
    const double *b = r.bounds;
    if (!r.uniform && r.nk + 1 <= LDS_BOUNDS_MAX) {
        for (int j = threadIdx.x; j <= r.nk; j += 256) s_bounds[j] = r.bounds[j];
        __syncthreads();
        b = s_bounds;
    }
    const double lo = r.uniform ? r.t_start + (double)r.k0 * r.window_s : b[0];
    const double hi = r.uniform ? r.t_start + (double)(r.k0 + r.nk) * r.window_s : b[r.nk];
    const size_t npx = (size_t)r.H * r.W;
    unsigned long long n_bad = 0, n_before = 0, n_after = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < r.n; i += (long long)gridDim.x * 256) {
        const float4 e = r.ev[i];
        const int x = pixel_coord(e.y, r.W), y = pixel_coord(e.z, r.H);
        if (x < 0 || y < 0 || !(e.w == 1.0f || e.w == -1.0f) || e.x != e.x) { ++n_bad; continue; }
        const double t = (double)e.x;
        if (t < lo) { ++n_before; continue; }
        if (!(t < hi)) { ++n_after; continue; }
        int k;
        double bk, bk1;
        if (r.uniform) {
            long long kk = (long long)floor((t - r.t_start) / r.window_s); // finite: lo <= t < hi
            bk = r.t_start + (double)kk * r.window_s;
            bk1 = r.t_start + (double)(kk + 1) * r.window_s;
            if (t < bk) { --kk; bk1 = bk; bk = r.t_start + (double)kk * r.window_s; }
            else if (t >= bk1) { ++kk; bk = bk1; bk1 = r.t_start + (double)(kk + 1) * r.window_s; }
            k = (int)(kk - r.k0);
        } else {
            k = count_le<double>(b, r.nk + 1, t) - 1; // entries <= t: at least one (t >= lo), at most nk (t < hi)
            bk = b[k];
            bk1 = b[k + 1];
        }
        if (k < 0 || k >= r.nk) { ++n_after; continue; } // (cannot happen for lo <= t < hi; no store without this check)
        const bool open = k == r.open_k;
        const int on = e.w == 1.0f ? 1 : 0;
        const size_t px = (size_t)y * r.W + x;
        if (r.count_open) {
            int *plane = open ? r.count_open : r.count + (size_t)k * 2 * npx;
            atomicAdd(plane + on * npx + px, 1);
        }
        if (r.surf_open) {
            unsigned int *plane = open ? r.surf_open : r.surf + (size_t)k * 2 * npx;
            atomicMax(plane + on * npx + px, surf_key(e.x));
        }
        if (r.vox_open && (open || (k >= r.v_a && k < r.v_b))) {
            long long *plane = open ? r.vox_open : r.vox + (size_t)(k - r.v_a) * r.B * npx;
            const double tau = (double)(r.B - 1) * ((t - bk) / (bk1 - bk));
            int b0 = (int)floor(tau);
            b0 = b0 < 0 ? 0 : (b0 > r.B - 1 ? r.B - 1 : b0);
            const double frac = tau - (double)b0;
            const long long q1 = llrint(frac * Q_ONE), q0 = (long long)Q_ONE - q1;
            const long long s = on ? 1 : -1;
            atomicAdd((unsigned long long *)(plane + (size_t)b0 * npx + px), (unsigned long long)(s * q0));
            if (q1 != 0 && b0 + 1 < r.B) atomicAdd((unsigned long long *)(plane + (size_t)(b0 + 1) * npx + px), (unsigned long long)(s * q1));
        }
    }
    if (r.counters) { // one add per wave and counter, and only where there is something to add
        n_bad = wave_sum(n_bad);
        n_before = wave_sum(n_before);
        n_after = wave_sum(n_after);
        if ((threadIdx.x & 63) == 0) {
            if (n_bad) atomicAdd(&r.counters[0], n_bad);
            if (n_before) atomicAdd(&r.counters[1], n_before);
            if (n_after) atomicAdd(&r.counters[2], n_after);
        }
    }
}

// V consecutive 32-bit words per lane: V = 4 is one 16-byte access (the pointers are 16-byte aligned and the counts multiples of 4)
template <int V> struct Words;
template <> struct Words<1> { typedef unsigned int T; };
template <> struct Words<4> { typedef uint4 T; };
__device__ __forceinline__ unsigned int word_zero(unsigned int) { return 0u; }
__device__ __forceinline__ uint4 word_zero(uint4) { return make_uint4(0u, 0u, 0u, 0u); }

// dst[0 .. n) = carry[0 .. n_carry) followed by zeros; carry = 0 (the open window's plane moves into the output as its first plane)
template <int V> __global__ __launch_bounds__(256) void k_move_zero(unsigned int *__restrict__ dst, long long n,
                                                                    unsigned int *__restrict__ carry, long long n_carry)
{
    typedef typename Words<V>::T T;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n) return;
    T v = word_zero(T());
    if (i < n_carry) {
        v = *(const T *)(carry + i);
        *(T *)(carry + i) = word_zero(T());
    }
    *(T *)(dst + i) = v;
}

// out[i] = (float)((double)acc[i] * 2^-24); clear: acc = 0 afterwards (the carried plane, once it has been handed out)
template <int V> __global__ __launch_bounds__(256) void k_voxel_finish(long long *__restrict__ acc, long long n, float *__restrict__ out,
                                                                       int clear)
{
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n) return;
    if constexpr (V == 1) {
        out[i] = (float)((double)acc[i] * (1.0 / Q_ONE));
        if (clear) acc[i] = 0;
    } else {
        const longlong2 a = *(const longlong2 *)(acc + i), b = *(const longlong2 *)(acc + i + 2);
        *(float4 *)(out + i) = make_float4((float)((double)a.x * (1.0 / Q_ONE)), (float)((double)a.y * (1.0 / Q_ONE)),
                                           (float)((double)b.x * (1.0 / Q_ONE)), (float)((double)b.y * (1.0 / Q_ONE)));
        if (clear) {
            *(longlong2 *)(acc + i) = make_longlong2(0, 0);
            *(longlong2 *)(acc + i + 2) = make_longlong2(0, 0);
        }
    }
}

// In place: planes[k][i] holds window k's maximum key (0: none); running maximum from state[i] on, decoded to the time stamp;
// state[i] = the maximum after the last plane.
template <int V> __global__ __launch_bounds__(256) void k_surface_finish(unsigned int *__restrict__ planes, int n_planes, long long plane_words,
                                                                         unsigned int *__restrict__ state)
{
    typedef typename Words<V>::T T;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= plane_words) return;
    union { T t; unsigned int w[V]; } m, c;
    m.t = *(const T *)(state + i);
    for (int k = 0; k < n_planes; ++k) {
        T *p = (T *)(planes + (size_t)k * plane_words + i);
        c.t = *p;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            m.w[j] = m.w[j] > c.w[j] ? m.w[j] : c.w[j];
            c.w[j] = __float_as_uint(surf_time(m.w[j]));
        }
        *p = c.t;
    }
    *(T *)(state + i) = m.t;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

} // namespace

extern "C" {

int v2e_tensorize_scatter(const float *events, int64_t n, int H, int W, double t_start, double window_s, const double *bounds,
                          int64_t k0, int nk, int has_open, int32_t *count, int32_t *count_open, int64_t *voxel_acc,
                          int64_t *voxel_open, int v_a, int v_b, int voxel_bins, uint32_t *surf_keys, uint32_t *surf_open,
                          uint64_t *counters, void *stream)
{
    V2E_REQUIRE(n >= 0 && (events || n == 0) && H > 0 && W > 0 && nk >= 0 && nk <= (1 << 22) + 1 && k0 >= 0 && (has_open == 0 || nk >= 1),
                "bad args");
    // (explicit bounds, nk == 0: the clip's last window is complete; every row is counted before or after bounds[0])
    V2E_REQUIRE(bounds || (window_s > 0 && nk >= 1), "a window length or a bounds table");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0, "rows must be 16-byte aligned");
    const int nc = nk - (has_open ? 1 : 0); // complete windows
    V2E_REQUIRE(!count_open || count || nc == 0, "null count planes");
    V2E_REQUIRE(!surf_open || surf_keys || nc == 0, "null surface planes");
    V2E_REQUIRE(!voxel_open || (voxel_bins >= 1 && v_a >= 0 && v_a <= v_b && v_b <= nc && (voxel_acc || v_a == v_b)), "bad voxel block");
    if (n == 0) return 0;
    ScatterArgs r;
    r.ev = (const float4 *)events; r.n = n; r.H = H; r.W = W; r.uniform = bounds ? 0 : 1; r.t_start = t_start; r.window_s = window_s;
    r.bounds = bounds; r.k0 = k0; r.nk = nk; r.open_k = has_open ? nk - 1 : -1;
    r.count = count; r.count_open = count_open; r.vox = (long long *)voxel_acc; r.vox_open = (long long *)voxel_open;
    r.v_a = v_a; r.v_b = v_b; r.B = voxel_bins; r.surf = surf_keys; r.surf_open = surf_open;
    r.counters = (unsigned long long *)counters;
    const int64_t blocks = (n + 255) / 256;
    const size_t lds = (bounds && nk + 1 <= LDS_BOUNDS_MAX) ? (size_t)(nk + 1) * sizeof(double) : 0;
    k_tensorize_scatter<<<(int)(blocks < SCATTER_MAX_BLOCKS ? blocks : SCATTER_MAX_BLOCKS), 256, lds, (hipStream_t)stream>>>(r);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_tensorize_move_zero(void *dst, int64_t n_words, void *carry, int64_t n_carry_words, void *stream)
{
    V2E_REQUIRE(n_words >= 0 && (dst || n_words == 0) && n_carry_words >= 0 && n_carry_words <= n_words && (carry || n_carry_words == 0) &&
                (((uintptr_t)dst | (uintptr_t)carry) & 3u) == 0, "bad args");
    if (n_words == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(dst) && aligned16(carry) && n_words % 4 == 0 && n_carry_words % 4 == 0)
        k_move_zero<4><<<v2e_cdiv(n_words / 4, 256), 256, 0, s>>>((unsigned int *)dst, n_words, (unsigned int *)carry, n_carry_words);
    else
        k_move_zero<1><<<v2e_cdiv(n_words, 256), 256, 0, s>>>((unsigned int *)dst, n_words, (unsigned int *)carry, n_carry_words);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_tensorize_voxel_finish(int64_t *acc, int64_t n, float *out, int clear, void *stream)
{
    V2E_REQUIRE(n >= 0 && ((acc && out) || n == 0) && ((uintptr_t)acc & 7u) == 0 && ((uintptr_t)out & 3u) == 0, "bad args");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(acc) && aligned16(out) && n % 4 == 0)
        k_voxel_finish<4><<<v2e_cdiv(n / 4, 256), 256, 0, s>>>((long long *)acc, n, out, clear);
    else
        k_voxel_finish<1><<<v2e_cdiv(n, 256), 256, 0, s>>>((long long *)acc, n, out, clear);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_tensorize_surface_finish(void *planes, int n_planes, int64_t plane_words, uint32_t *state, void *stream)
{
    V2E_REQUIRE(n_planes >= 0 && plane_words > 0 && state && (planes || n_planes == 0) && (((uintptr_t)planes | (uintptr_t)state) & 3u) == 0,
                "bad args");
    if (n_planes == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(planes) && aligned16(state) && plane_words % 4 == 0)
        k_surface_finish<4><<<v2e_cdiv(plane_words / 4, 256), 256, 0, s>>>((unsigned int *)planes, n_planes, plane_words, state);
    else
        k_surface_finish<1><<<v2e_cdiv(plane_words, 256), 256, 0, s>>>((unsigned int *)planes, n_planes, plane_words, state);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
