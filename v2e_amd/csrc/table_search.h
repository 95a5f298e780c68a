// table_search.h -- the binary searches over ascending tables of the event-row kernels (sinks.hip, probe.hip, render.hip,
// denoise.hip, patches.hip, tensorize.hip): one loop, first_not, and the counts and frame lookups on top of it.
//
// Included by the device code, by host code of the library (v2e_events_format_text_host) and by the CPU test
// (tests/test_table_search.py), which checks it against numpy.searchsorted and direct loops.
#pragma once
#include <stdint.h>

#include "../../include/v2e_amd.h"

#if defined(__HIPCC__)
#define V2E_TS_HD __host__ __device__ __forceinline__
#else
#define V2E_TS_HD static inline
#endif

// the first index in [lo, hi) at which below(index) is false, hi if it is true throughout; below is true on a prefix of the range
// and false behind it (lo >= hi: lo).  It is called once per probe, so it may remember what it saw (rowkeys.h: latest_before).
template <typename F> V2E_TS_HD int first_not(int lo, int hi, F below)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (below(mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the number of entries of the ascending table a[0 .. n) that are <= v (numpy.searchsorted 'right') / < v ('left').  from: a known
// lower bound of the result -- the entries before it are not read
template <typename T> V2E_TS_HD int count_le(const T *a, int n, T v, int from = 0)
{
    return first_not(from, n, [=](int m) { return a[m] <= v; });
}
template <typename T> V2E_TS_HD int count_lt(const T *a, int n, T v, int from = 0)
{
    return first_not(from, n, [=](int m) { return a[m] < v; });
}

// the frame of row i of a run: the last record whose ev_offset is <= i (of frames without rows, which share an ev_offset, the
// last); record 0 for a row below every ev_offset
V2E_TS_HD int frame_of_row(const v2e_frame_rec *recs, int nrec, int64_t i)
{
    return first_not(1, nrec, [=](int m) { return (int64_t)recs[m].ev_offset <= i; }) - 1;
}

// 1: row i is a signal event, 0: noise -- the emulator puts a frame's n_signal signal rows first, then its noise.
// recs == nullptr: one frame of n_signal0 signal rows at row 0 (the per-frame path)
V2E_TS_HD int row_is_signal(int64_t i, const v2e_frame_rec *recs, int nrec, int64_t n_signal0)
{
    if (!recs) return i < n_signal0;
    const v2e_frame_rec *r = recs + frame_of_row(recs, nrec, i);
    return i - (int64_t)r->ev_offset < (int64_t)r->n_signal;
}
