// patch_entry.h -- one entry of a row's time-surface patch, the rule of patches.hip's header comment written once: the inside-sensor
// test, the search for the latest earlier row at the entry's pixel, the fall-back to the carried maps, -inf -> none, the age and the
// two features of either mode.  Called per (row, offset) by k_patches_features (patches.hip), which writes the features out, and by
// k_mlp_scores (mlpf.hip), which keeps them in LDS.
#pragma once
#include "rowkeys.h"

struct PatchSource {
    const float4 *ev;            // the rows of the pass
    const long long *sorted;     // the sorted keys
    const int *seg;              // [H*W + 1]
    const float *last_t;         // [H*W], the carried maps (read only here)
    const signed char *last_p;   // [H*W]
    int H, W;
};

__device__ __forceinline__ float pos_inf() { return __int_as_float(0x7f800000); }

// entry o = (dy + R) * P + (dx + R) of the patch of row key.i, whose time is t: *f0, *f1 are its channel 0 and channel 1 features
// (mode 0 age, 1 linear with tau)
template <int R>
__device__ __forceinline__ void patch_entry(const PatchSource &s, const RowKey &key, float t, int o, int mode, double tau, float *f0,
                                            float *f1)
{
    constexpr int P = 2 * R + 1;
    const int dy = o / P - R, dx = o - (o / P) * P - R;
    const int qx = key.x + dx, qy = key.y + dy;
    *f0 = mode ? 0.0f : pos_inf(); // none
    *f1 = 0.0f;
    if (qx >= 0 && qx < s.W && qy >= 0 && qy < s.H) {
        const long long q = key.p + (long long)dy * s.W + dx;
        unsigned int before;
        float tq, pq;
        if (latest_before(s.sorted, s.seg, q, key.i, &before)) {
            const float4 e = s.ev[before];
            tq = e.x;
            pq = e.w > 0.0f ? 1.0f : -1.0f;
        } else {
            tq = s.last_t[q];
            pq = (float)s.last_p[q];
        }
        if (tq != -pos_inf()) {
            const double age = (double)t - (double)tq;
            if (mode == 0) {
                *f0 = (float)age;
                *f1 = pq;
            } else if (age < tau) {
                *f0 = age <= 0.0 ? 1.0f : (float)(1.0 - age / tau);
                *f1 = pq;
            }
        }
    }
}
