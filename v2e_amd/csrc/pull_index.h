// pull_index.h -- k_cpull's group lookup (emu_chain.h): which emission group holds canonical index cp of a key.
//
// A key's prefix row pre[0 .. P2) is the exclusive prefix of its per-group event counts (k_cframe*); entries at and beyond the
// last group hold the key's total T or more.  The group of cp < T is the LAST g with pre[g] <= cp (an empty group shares its
// prefix with the next one).  A binary search over the whole row is log2(P2) dependent LDS reads per row (9 at 346x260).
//
// The bucketed index: canonical indices are cut into buckets of 2^s (s from pull_bucket_shift: at most nb - 1 index entries), and
// idx[b] is the group holding index b << s; idx[ceil(T / 2^s)] is the last non-empty group.  The group of cp then lies in
// [idx[cp >> s], idx[(cp >> s) + 1]], which is a couple of groups wide when there are about as many buckets as groups: one index
// read (two entries) and a binary search over that range, instead of a search over the whole row.  Each non-empty group writes
// the entries of the bucket starts it holds (pull_index_group), so the index is built from the row as it is staged, with no
// extra pass.
//
// Included by the device code and by the CPU test (tests/test_cpull_lookup.py), which checks it against the whole-row search.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define V2E_PI_HD __host__ __device__ __forceinline__
#else
#define V2E_PI_HD static inline
#endif

// the smallest s with ((T - 1) >> s) + 1 < nb: entries 0 .. ceil(T / 2^s) of the index fit in nb
V2E_PI_HD uint32_t pull_bucket_shift(uint32_t T, uint32_t nb)
{
    uint32_t s = 0;
    if (T > 0u)
        while (((T - 1u) >> s) + 2u > nb) ++s;
    return s;
}

// group g covers canonical indices [cur, next) (both clamped to T: rows beyond the last group and padding write nothing)
V2E_PI_HD void pull_index_group(uint16_t *idx, uint32_t g, uint32_t cur, uint32_t next, uint32_t T, uint32_t s)
{
    cur = cur < T ? cur : T;
    next = next < T ? next : T;
    if (cur >= next) return; // empty
    const uint32_t b0 = cur == 0u ? 0u : ((cur - 1u) >> s) + 1u; // ceil(cur / 2^s): the first bucket starting in the group
    uint32_t b1 = ((next - 1u) >> s) + 1u;                        // ceil(next / 2^s)
    if (next == T) ++b1;                                          // the last group also writes the closing entry
    for (uint32_t b = b0; b < b1; ++b) idx[b] = (uint16_t)g;
}

// the last g with tab[g] <= cp (cp < T); *gbase = tab[g]
V2E_PI_HD uint32_t pull_index_find(const uint32_t *tab, const uint16_t *idx, uint32_t s, uint32_t cp, uint32_t *gbase)
{
    const uint32_t b = cp >> s;
    uint32_t lo = idx[b], hi = idx[b + 1u]; // tab[lo] <= b << s <= cp; every group after hi starts beyond cp
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (tab[mid] <= cp) lo = mid;
        else hi = mid - 1u;
    }
    *gbase = tab[lo];
    return lo;
}
