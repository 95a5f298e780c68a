// rowkeys.h -- the row index of denoise.hip and patches.hip: which rows are valid, the sort key pixel << 32 | row of a valid row,
// and "the latest earlier row at pixel q" in the sorted keys.  seg[p] (k_denoise_segments) is the number of sorted keys below
// p << 32: pixel p's rows are sorted[seg[p] .. seg[p+1]), in row order, and seg[H*W] is the number of valid rows.  It also holds
// the label rule of every kernel that takes the rows' signal / noise labels (row_label), window.hip's and dwindow.hip's included.
#pragma once
#include <hip/hip_runtime.h>

#include "table_search.h"

constexpr long long KEY_BAD = 0x7fffffffffffffffLL;         // sorts behind every valid key as a signed 64-bit value

// v as a coordinate: its value if that is an integer in [0, size), else -1 (the float comparisons come first: they refuse NaN and
// everything the int conversion cannot hold)
__device__ __forceinline__ int pixel_coord(float v, int size)
{
    if (!(v >= 0.0f && v < (float)size)) return -1;
    const int c = (int)v;
    return (float)c == v ? c : -1;
}

// the pixel of a valid row, -1 for a bad one: x / y not a coordinate of the sensor, or t not finite
__device__ __forceinline__ long long row_pixel(const float4 e, int H, int W)
{
    const int x = pixel_coord(e.y, W), y = pixel_coord(e.z, H);
    if (x < 0 || y < 0 || !(fabsf(e.x) <= 3.402823466e+38f)) return -1;
    return (long long)y * W + x;
}

// The label of row i of a pass, 1 = signal, 0 = noise: labels[i] != 0 (a byte per row of the pass), else whether an odd number of
// lbounds entries (ascending row indices of the whole call, in which the pass's row 0 is row0) is <= row0 + i, else signal.
__device__ __forceinline__ int row_label(const unsigned char *labels, const long long *lbounds, int n_lbounds, long long row0,
                                         long long i)
{
    int label = 1;
    if (labels) label = labels[i] ? 1 : 0;
    else if (lbounds) label = count_le<long long>(lbounds, n_lbounds, row0 + i) & 1;
    return label;
}

struct RowKey { unsigned int i; long long p; int x, y; }; // row index, pixel = y * W + x (p < H * W <= 2^31 - 1)

__device__ __forceinline__ RowKey decode_key(long long key, int W)
{
    RowKey k;
    k.i = (unsigned int)key;
    k.p = key >> 32;
    k.y = (int)k.p / W;
    k.x = (int)k.p - k.y * W;
    return k;
}

// the valid keys of a pass of n rows: no read past the pass's keys, whatever seg holds
__device__ __forceinline__ int valid_keys(const int *seg, int H, int W, int n)
{
    const int n_seg = seg[(long long)H * W];
    return n_seg < n ? n_seg : n;
}

// The latest row of the pass before row i at pixel q: the largest row index below i in q's stretch, which the search meets as its
// last probe below i.  true: *row is that row; false: the pass has none and the carried map holds what was there.
__device__ __forceinline__ bool latest_before(const long long *sorted, const int *seg, long long q, unsigned int i, unsigned int *row)
{
    const int lo = seg[q];
    unsigned int before = 0;
    const int s = first_not(lo, seg[q + 1], [&](int m) {
        const unsigned int v = (unsigned int)sorted[m];
        if (v < i) before = v;
        return v < i;
    });
    *row = before;
    return s > lo;
}

// the carried maps of pixel p from its last row of the pass, if it has one (last_p: null where no polarity map is carried)
__device__ __forceinline__ void map_update(const float4 *ev, const long long *sorted, const int *seg, long long p, float *last_t,
                                           signed char *last_p)
{
    const int lo = seg[p], hi = seg[p + 1];
    if (hi <= lo) return;
    const float4 e = ev[(unsigned int)sorted[hi - 1]];
    last_t[p] = e.x;
    if (last_p) last_p[p] = e.w > 0.0f ? 1 : -1;
}
