// emu_shared.h -- what more than one translation unit of the emulator model needs (emu.hip through emu_kernels.h, sweep.hip): the
// per-frame scalars (FrameCtl / make_ctl), the lin-log mapping, the reference's floor division and the wave64 sums.  One text,
// included by both, so that both compute the same values; every unit gets its own copy in its anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;

struct FrameCtl {
    double t_prev, t_frame;
    // per-frame scalars the reference evaluates once in Python doubles; filled by the host with the
    // same IEEE operations (emulator_utils.py:80-84, 326-327) so kernels need not redo them per lane
    double dt_over_tau; // delta_time / (1/(math.pi*2*cutoff_hz)), 0 when cutoff_hz <= 0
    double shot_base;   // (shot_noise_rate_hz/2) * delta_time
    // timestamp generator (emulator.py:791-796) and refractory switch (:830) for every iteration
    // count n = 1..32, so the kernel needs no float64 division once the frame's max is known
    float ts_start[32], ts_stepf[32];
    uint32_t refr_mask; // bit n-1: refractory_period_s > delta_time / n
    float ts_end;       // (float)t_frame
    uint32_t refr_on_n; // smallest iteration count n >= 1 for which the rule is on (0xFFFFFFFF: never); the predicate is monotone in n
    uint32_t pad_;
};

__host__ __device__ inline FrameCtl make_ctl(double t_prev, double t_frame, double cutoff_hz, double shot_rate_hz, double refr_s)
{
    FrameCtl c;
    c.t_prev = t_prev; c.t_frame = t_frame;
    const double dt = t_frame - t_prev;
    c.dt_over_tau = 0.0;
    if (cutoff_hz > 0) { const double tau = 1.0 / (M_PI * 2 * cutoff_hz); c.dt_over_tau = dt / tau; }
    c.shot_base = (shot_rate_hz / 2) * dt;
    c.refr_mask = 0;
    const float end = (float)t_frame;
    c.ts_end = end;
    for (int n = 1; n <= 32; ++n) { // same IEEE operations as TsGen (emu_kernels.h)
        const double ts_step = dt / (double)n;
        const float start = (float)(t_prev + ts_step);
        c.ts_start[n - 1] = start;
        c.ts_stepf[n - 1] = n > 1 ? (end - start) / (float)(n - 1) : 0.0f;
        if (refr_s > ts_step) c.refr_mask |= 1u << (n - 1);
    }
    c.refr_on_n = 0xFFFFFFFFu;
    c.pad_ = 0u;
    if (refr_s > 0) { // emulator.py:830 `refractory_period_s > ts_step`, ts_step = delta_time / n: first n that satisfies it
        const double g = dt / refr_s;
        if (!(g > 4.0e9)) {
            long long n0 = (long long)floor(g) - 2;
            if (n0 < 1) n0 = 1;
            while (!(refr_s > dt / (double)n0) && n0 < 0xFFFFFFFEll) ++n0;
            while (n0 > 1 && refr_s > dt / (double)(n0 - 1)) --n0;
            c.refr_on_n = (uint32_t)n0;
        }
    }
    return c;
}

// (1./20)*math.log(20) as evaluated by CPython (emulator_utils.py:34)
__device__ constexpr double LINLOG_F = 0x1.32c352f8fe941p-3;

__device__ __forceinline__ float lin_log(double x)
{
    double y = (x <= 20.0) ? x * LINLOG_F : log(x);
    y = rint(y * 1e8) / 1e8;
    return (float)y;
}

// c10::div_floor_floating
template <typename R> __device__ __forceinline__ R div_floor(R a, R b)
{
    if (b == (R)0) return a / b;
    R mod = fmod(a, b);
    R div = (a - mod) / b;
    if (mod != (R)0 && ((b < (R)0) != (mod < (R)0))) div -= (R)1;
    R fd;
    if (div != (R)0) {
        fd = floor(div);
        if (div - fd > (R)0.5) fd += (R)1;
    } else {
        fd = copysign((R)0, a / b);
    }
    return fd;
}

// ---- wave64 reductions on the VALU data-parallel-primitive path (DPP), not through the LDS
// crossbar (__shfl_* lowers to ds_bpermute, an LDS-latency operation per step; with one wave per
// SIMD nothing hides it).  Within a 16-lane row: butterfly with quad_perm / row_half_mirror /
// row_mirror; across the four rows: v_readlane + scalar ops, so results are wave-uniform SGPRs.
#define V2E_DPP(v, ctrl) __builtin_amdgcn_update_dpp(0, (v), (ctrl), 0xf, 0xf, true)

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t u)
{
    int v = (int)u;
    v += V2E_DPP(v, 0xB1);
    v += V2E_DPP(v, 0x4E);
    v += V2E_DPP(v, 0x141);
    v += V2E_DPP(v, 0x140);
    return (uint32_t)(__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
                      __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

__device__ __forceinline__ uint32_t wave_or_u32(uint32_t u)
{
    int v = (int)u;
    v |= V2E_DPP(v, 0xB1);
    v |= V2E_DPP(v, 0x4E);
    v |= V2E_DPP(v, 0x141);
    v |= V2E_DPP(v, 0x140);
    return (uint32_t)(__builtin_amdgcn_readlane(v, 0) | __builtin_amdgcn_readlane(v, 16) |
                      __builtin_amdgcn_readlane(v, 32) | __builtin_amdgcn_readlane(v, 48));
}

} // namespace
