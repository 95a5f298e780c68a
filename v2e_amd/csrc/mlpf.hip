// mlpf.hip -- a learned patch filter in one pass: for every row of a device-resident run the (2r+1) x (2r+1) time-surface patch of
// patches.hip in mode "linear" is gathered into LDS, a one-hidden-layer MLP is evaluated on it and one float32 score per row is
// written; no feature ever exists in global memory (host side: v2e_amd/mlpf.py, MLPFilter).
//
// Rows, validity, carried maps and the per-row patch are exactly patches.hip's with mode 1 and the same tau (patch_entry.h).  The
// input of row i is its patch flattened as [2][P][P]: x[c * P * P + (dy + r) * P + (dx + r)], K = 2 * P * P entries, all finite.
// Network: w1 float32 [hidden][K], b1 [hidden], w2 [hidden], b2 [1], 1 <= hidden <= 64.  Arithmetic, so that a plain loop
// reproduces it bit for bit:
//   a_j = (double)b1[j];  for k = 0 .. K-1 ascending: a_j = a_j + (double)w1[j][k] * (double)x[k]
//   h_j = (float)a_j, rounded to nearest even;  h_j = h_j > 0 ? h_j : 0 (a NaN becomes 0)
//   s = (double)b2;  for j ascending: s = s + (double)w2[j] * (double)h_j;  score = (float)s
// The product of two float32 values is exact in float64, so every step is one float64 rounding, with an fma or without one: the
// kernel says fma() and the result does not depend on -ffp-contract.  mask (optional): (double)score >= threshold, 0 for a bad row;
// a bad row's score is the quiet NaN 0x7fc00000 and its valid flag 0.
//
// Mapping: a workgroup of 256 threads takes tiles of MLP_TILE_ROWS = 64 consecutive sorted keys (pixel order, as k_patches_features:
// neighbouring rows search neighbouring stretches), in a grid-stride loop under a capped grid.
//   phase 1: one thread per (row, offset) calls patch_entry and stores the two features into the LDS tile x[row][KS], KS = K | 1: an
//            odd row stride, so that the 64 lanes of a wave that walk k in phase 2, one row each, hit 64 banks.
//   phase 2: wave g of the workgroup owns the hidden units g * G .. g * G + G - 1, G = ceil(hidden / 4), lane = row: G float64
//            accumulators in registers, k ascending.  w1 is staged once per workgroup in LDS, transposed and zero-padded to
//            wt[k][4][GP], GP = G rounded up to 4: a wave's weights of one k are one address for all lanes (broadcast reads of 16 bytes).
//   phase 3: h goes to LDS as float32 (over the feature tile, which nobody reads any more; row stride hidden | 1), one thread per row
//            sums j ascending and writes score and mask at the row's own index.
// LDS at r = 3, hidden = 64: 25 344 bytes of features / h + 25 088 of weights + 768 of row keys and times: three workgroups per CU.
// Bad rows have no sorted key: k_mlp_bad_rows walks the rows in row order and writes valid[] for all, NaN and mask 0 for the bad.
#include "common.h"
#include "patch_entry.h"

namespace {

constexpr int MLP_TILE_ROWS = 64;          // rows per workgroup and tile (v2e_amd/mlpf.py: ROWS_PER_WORKGROUP)
constexpr int MLP_MAX_BLOCKS = 2048;       // x MLP_TILE_ROWS: a second grid-stride trip above 131 072 valid rows
constexpr int MLP_MAX_HIDDEN = 64;
constexpr int MLP_GROUPS = 4;              // waves of a workgroup: each owns a group of hidden units

struct MlpArgs {
    PatchSource src;             // rows, row index and carried maps
    int n;                       // rows of this pass
    double tau;
    const float *w1, *b1, *w2, *b2;
    int hidden;
    float *scores;               // [n]
    double threshold;
    unsigned char *mask;         // [n] or null
};

__host__ __device__ constexpr int mlp_tile_floats(int K, int hidden)
{
    const int ks = K | 1, hs = hidden | 1;
    return MLP_TILE_ROWS * (ks > hs ? ks : hs);
}

// the hidden units of wave g over the tile's features: lane = row, k ascending, G accumulators
template <int G, int K>
__device__ __forceinline__ void mlp_hidden(const float *x_row, const float *wt_g, const float *b1, int j0, int hidden, float *h)
{
    constexpr int GP = (G + 3) & ~3;
    double acc[G];
#pragma unroll
    for (int u = 0; u < G; ++u) acc[u] = j0 + u < hidden ? (double)b1[j0 + u] : 0.0;
    for (int k = 0; k < K; ++k) {
        const double x = (double)x_row[k];
        const float *w = wt_g + k * (MLP_GROUPS * GP);
#pragma unroll
        for (int u = 0; u < G; ++u) acc[u] = fma((double)w[u], x, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const float v = (float)acc[u];
        h[u] = v > 0.0f ? v : 0.0f;
    }
}

template <int R, int G>
__device__ __forceinline__ void mlp_hidden_g(const float *x_row, const float *wt_g, const float *b1, int j0, int hidden, float *h)
{
    mlp_hidden<G, 2 * (2 * R + 1) * (2 * R + 1)>(x_row, wt_g, b1, j0, hidden, h);
}

template <int R>
__global__ __launch_bounds__(256) void k_mlp_scores(MlpArgs a)
{
    constexpr int P = 2 * R + 1, PP = P * P, K = 2 * PP, KS = K | 1, T = MLP_TILE_ROWS;
    extern __shared__ float lds[];
    __shared__ long long s_key[T];
    __shared__ float s_t[T];
    const int W = a.src.W, H = a.src.H, hidden = a.hidden;
    const int G = (hidden + MLP_GROUPS - 1) / MLP_GROUPS, GP = (G + 3) & ~3, HS = hidden | 1;
    float *x = lds;                                      // [T][KS] features, then [T][HS] hidden values
    float *wt = lds + mlp_tile_floats(K, hidden);        // [K][MLP_GROUPS][GP]
    const int tid = threadIdx.x;
    for (int e = tid; e < K * MLP_GROUPS * GP; e += 256) {
        const int k = e / (MLP_GROUPS * GP), c = e - k * (MLP_GROUPS * GP), g = c / GP, u = c - g * GP;
        const int j = g * G + u;
        wt[e] = (u < G && j < hidden) ? a.w1[j * K + k] : 0.0f;
    }
    const int total = valid_keys(a.src.seg, H, W, a.n);
    const int tiles = (total + T - 1) / T;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int j0 = tile * T;
        __syncthreads();                                 // the previous tile's phase 3 has read h; the weights are staged
        if (tid < T) {
            long long key = KEY_BAD;
            float t = 0.0f;
            if (j0 + tid < total) {
                key = a.src.sorted[j0 + tid];
                const RowKey rk = decode_key(key, W);
                if (rk.i >= (unsigned int)a.n || rk.p >= (long long)H * W) key = KEY_BAD; // (not a key of this pass)
                else t = a.src.ev[rk.i].x;
            }
            s_key[tid] = key;
            s_t[tid] = t;
        }
        __syncthreads();
        // phase 1: the features of the tile's rows
        for (int e = tid; e < T * PP; e += 256) {
            const int row = e / PP, o = e - row * PP;
            const long long key = s_key[row];
            float f0 = 0.0f, f1 = 0.0f;
            if (key != KEY_BAD) patch_entry<R>(a.src, decode_key(key, W), s_t[row], o, 1, a.tau, &f0, &f1);
            x[row * KS + o] = f0;
            x[row * KS + PP + o] = f1;
        }
        __syncthreads();
        // phase 2: wave g, lane = row
        const int g = tid >> 6, row = tid & 63;
        float h[16];
        {
            const float *x_row = x + row * KS, *wt_g = wt + g * GP;
            const int u0 = g * G;
            switch (G) {
            case 1: mlp_hidden_g<R, 1>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 2: mlp_hidden_g<R, 2>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 3: mlp_hidden_g<R, 3>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 4: mlp_hidden_g<R, 4>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 5: mlp_hidden_g<R, 5>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 6: mlp_hidden_g<R, 6>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 7: mlp_hidden_g<R, 7>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 8: mlp_hidden_g<R, 8>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 9: mlp_hidden_g<R, 9>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 10: mlp_hidden_g<R, 10>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 11: mlp_hidden_g<R, 11>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 12: mlp_hidden_g<R, 12>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 13: mlp_hidden_g<R, 13>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 14: mlp_hidden_g<R, 14>(x_row, wt_g, a.b1, u0, hidden, h); break;
            case 15: mlp_hidden_g<R, 15>(x_row, wt_g, a.b1, u0, hidden, h); break;
            default: mlp_hidden_g<R, 16>(x_row, wt_g, a.b1, u0, hidden, h); break;
            }
        }
        __syncthreads();                                 // every wave has read its features: h takes their place
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (u < G && g * G + u < hidden) x[row * HS + g * G + u] = h[u];
        __syncthreads();
        // phase 3: one thread per row, j ascending
        if (tid < T && s_key[tid] != KEY_BAD) {
            double s = (double)a.b2[0];
            for (int j = 0; j < hidden; ++j) s = fma((double)a.w2[j], (double)x[tid * HS + j], s);
            const float score = (float)s;
            const unsigned int i = (unsigned int)s_key[tid];
            a.scores[i] = score;
            if (a.mask) a.mask[i] = (double)score >= a.threshold ? 1 : 0;
        }
    }
}

// valid[i] for every row, in row order; the quiet NaN and mask 0 of the bad ones
__global__ __launch_bounds__(256) void k_mlp_bad_rows(const float4 *__restrict__ ev, long long n, int H, int W, float *__restrict__ scores,
                                                      unsigned char *__restrict__ valid, unsigned char *__restrict__ mask)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool bad = row_pixel(ev[i], H, W) < 0;
    valid[i] = bad ? 0 : 1;
    if (bad) {
        scores[i] = __int_as_float(0x7fc00000);
        if (mask) mask[i] = 0;
    }
}

} // namespace

extern "C" {

int v2e_patches_mlp_scores(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                           const int8_t *last_p, int radius, double tau, const float *w1, const float *b1, int hidden, const float *w2,
                           const float *b2, float *scores, uint8_t *valid, double threshold, uint8_t *mask_or_null, void *stream)
{
    V2E_REQUIRE(n >= 0 && n <= 0x7fffffff && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff && seg && last_t && last_p &&
                ((events && sorted_keys && scores && valid) || n == 0), "bad args");
    V2E_REQUIRE(radius >= 1 && radius <= 3, "radius 1, 2 or 3");
    V2E_REQUIRE(hidden >= 1 && hidden <= MLP_MAX_HIDDEN, "hidden 1 .. 64");
    V2E_REQUIRE(tau > 0.0 && tau <= 1.7976931348623157e308, "tau > 0 and finite");
    V2E_REQUIRE(w1 && b1 && w2 && b2, "null weights");
    V2E_REQUIRE(((uintptr_t)events & 15u) == 0 && ((uintptr_t)scores & 3u) == 0 && ((uintptr_t)w1 & 3u) == 0 && ((uintptr_t)b1 & 3u) == 0 &&
                ((uintptr_t)w2 & 3u) == 0 && ((uintptr_t)b2 & 3u) == 0, "rows must be 16-byte aligned, scores and weights 4-byte aligned");
    V2E_REQUIRE(threshold == threshold || !mask_or_null, "threshold NaN");
    if (n == 0) return 0;
    const int P = 2 * radius + 1, K = 2 * P * P;
    const int G = (hidden + MLP_GROUPS - 1) / MLP_GROUPS, GP = (G + 3) & ~3;
    MlpArgs a;
    a.src.ev = (const float4 *)events; a.src.sorted = (const long long *)sorted_keys; a.src.seg = seg; a.src.last_t = last_t;
    a.src.last_p = (const signed char *)last_p; a.src.H = H; a.src.W = W;
    a.n = (int)n; a.tau = tau; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.hidden = hidden; a.scores = scores; a.threshold = threshold;
    a.mask = mask_or_null;
    const size_t lds_bytes = ((size_t)mlp_tile_floats(K, hidden) + (size_t)K * MLP_GROUPS * GP) * sizeof(float); // <= 50 432
    const int64_t want = (n + MLP_TILE_ROWS - 1) / MLP_TILE_ROWS;
    const int blocks = (int)(want < MLP_MAX_BLOCKS ? want : MLP_MAX_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    if (radius == 1) k_mlp_scores<1><<<blocks, 256, lds_bytes, s>>>(a);
    else if (radius == 2) k_mlp_scores<2><<<blocks, 256, lds_bytes, s>>>(a);
    else k_mlp_scores<3><<<blocks, 256, lds_bytes, s>>>(a);
    V2E_HIP(hipGetLastError());
    k_mlp_bad_rows<<<v2e_cdiv(n, 256), 256, 0, s>>>((const float4 *)events, n, H, W, scores, valid, mask_or_null);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
