// block_ops.h -- sums, ranks and scans over the lanes of a workgroup, shared by the event-row kernels (sinks.hip, readers.hip,
// tensorize.hip).  Every function is called by all threads of the workgroup; `s` is LDS of the caller.
#pragma once
#include <hip/hip_runtime.h>

// sum of v over the wave, valid in lane 0
template <typename T> __device__ __forceinline__ T wave_sum(T v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sum over the workgroup's `waves` waves of the value lane 0 of each holds, valid in thread 0 (s: one slot per wave).  A caller
// that passes its wave count as a constant gets the slots read at once; a loop of unknown length reads them one after the other
__device__ __forceinline__ int sum_of_waves(int wave_value, int *s, int waves)
{
    __syncthreads(); // s may still be read from an earlier sum
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = wave_value;
    __syncthreads();
    int t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < waves; ++w) t += s[w];
    return t;
}

// sum of v over the workgroup, valid in thread 0; block_count: the number of its lanes with `flag`, by ballot instead of shuffles
__device__ __forceinline__ int block_sum(int v, int *s, int waves = blockDim.x >> 6) { return sum_of_waves(wave_sum(v), s, waves); }
__device__ __forceinline__ int block_count(bool flag, int *s, int waves = blockDim.x >> 6)
{
    return sum_of_waves((int)__popcll(__ballot(flag)), s, waves);
}

// the number of kept items before this lane in its workgroup (s: one slot per wave)
__device__ __forceinline__ int block_rank(bool keep, int *s)
{
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads(); // s may still be read from an earlier rank or sum
    if (lane == 0) s[wave] = (int)__popcll(b);
    __syncthreads();
    int before = (int)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += s[w];
    return before;
}

// Hillis-Steele inclusive scan in place over s[0 .. N), N the workgroup's size: thread t wrote s[t] before the call and may read
// every entry after it
template <int N, typename T> __device__ __forceinline__ void block_scan(T *s)
{
    const int tid = threadIdx.x;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const T v = tid >= off ? s[tid - off] : T(0);
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
}

// exclusive scan of the per-block counts blk[0 .. nblk) in place by ONE workgroup of 1024 threads (s_part: 1024 slots), thread t
// owning the (nblk + 1023) / 1024 entries from t times that on.  Returns the thread's inclusive partial: in thread 1023 the total.
template <typename T> __device__ __forceinline__ T block_bases(T *__restrict__ blk, int nblk, T *s_part)
{
    const int tid = threadIdx.x;
    const int per = (nblk + 1023) / 1024;
    T sum = 0;
    for (int k = 0; k < per; ++k) { const int j = tid * per + k; if (j < nblk) sum += blk[j]; }
    s_part[tid] = sum;
    block_scan<1024>(s_part);
    T run = s_part[tid] - sum;
    for (int k = 0; k < per; ++k) {
        const int j = tid * per + k;
        if (j < nblk) { const T c = blk[j]; blk[j] = run; run += c; }
    }
    return s_part[tid];
}
