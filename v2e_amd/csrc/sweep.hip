// sweep.hip -- ON / OFF event counts of one clip for many thresholds in one pass (host side: v2e_amd/sweep.py, ThresholdSweep).
//
// Column j of the sweep is a Philox-mode emulator with pos_thres = pos[j], neg_thres = neg[j] and no shot noise, fed the clip's
// frames one by one.  Only the thresholds, base_log_frame and the counts depend on j: every Philox draw is keyed by (pixel, frame,
// stream, clip), lp_log_frame is a function of the frames alone.  So one thread (one pixel) reads each frame's byte once, advances
// lp_log_frame once, draws the frame's leak jitter once, and carries TB columns of (base_log_frame, ON count, OFF count) in
// registers; blockIdx.y is the chunk of TB columns.  Nothing is written per event, per frame or per pixel: the counts of the
// pixels inside the ROI are summed per wave and workgroup and added to counts[T][2] with integer atomics (two runs are bit-equal).
// A pixel's own ON (OFF) total of a column is a 32-bit register; every sum of pixels is 64-bit.
//
// Per frame and column the arithmetic is k_count's and k_emit's (emu_kernels.h), value for value: the leak step
// ((float)dt * rate) * thp, base - leak, diff = lp - base, the floor division (k_chain's guarded reciprocal form, emu_chain.h: the
// quotient estimate |diff| * (1 / theta), the exactly rounded remainder by one fma, a one-step fix-up; anything unusual takes
// div_floor), base +- (R)((float)count * theta).  The file is built with -ffp-contract=off like the rest of the library.
//
// The refractory rule (emulator.py:830) is the only coupling between pixels: it is on for a frame when refractory_period_s >
// dt / max(1, M), M the frame's largest per-pixel count.  While it has never been on, timestamp_mem is neither read nor written,
// so every column runs as if the rule were off and raises a sticky flag as soon as a pixel's count reaches the frame's
// FrameCtl::refr_on_n (the smallest M for which the rule is on).  A column whose flag stays 0 is exact; the others are the
// caller's to recompute with the emulator itself.
//
// A clip may arrive in chunks (v2e_thres_sweep_chunk): the same kernel template with CARRY = true takes lp and every column's base
// from planes of the caller's, [npx] and [T][npx] of R (a wave's 64 pixels of a column are 64 consecutive values: one coalesced
// load and store per column and thread, no LDS), and leaves the state behind the chunk's last frame in a second set of planes.  It
// never writes what it reads: when a flag rises in a chunk, the state at the START of that chunk -- exact by the invariant above --
// is still there for the emulator that takes the column over.  Counts are added to, flags OR-ed into, Philox is keyed by the
// clip's frame index.  Registers, occupancy and time of the CARRY = false instantiations are those the kernel had before it had
// the parameter (profiles/r18_sweep_stream.txt).
#include "common.h"
#include "../../include/v2e_detmath.h"
#include "emu_shared.h"

#include <cmath>
#include <mutex>
#include <vector>

namespace {

// a frame's scalars, from make_ctl's arithmetic on the host.  Entry 0 is the first frame (it initialises the state: k_init), whose
// low-pass step runs from time 0.
struct SweepFrame {
    double dt_over_tau; // FrameCtl::dt_over_tau
    float dtime_f;      // (float)(t_frame - t_prev)
    uint32_t refr_on_n; // FrameCtl::refr_on_n
};

struct SweepArgs {
    const uint8_t *frames; // [F][npx]
    int F, npx, W, T;
    int x0, x1, y0, y1;    // ROI, inclusive
    const SweepFrame *tab; // [F]
    const double *pos, *neg; // [T]
    int do_leak, need_r, has_cutoff;
    float sigma_f, leak_hz_f, jit_f, ln10cov_f;
    unsigned long long seed;
    unsigned long long *counts; // [T][2]: ON, OFF
    int *rule_on;               // [T]
};

// What a chunk of a streamed clip adds (v2e_thres_sweep_chunk): the clip's index of the chunk's first frame and the per-column state
// carried from call to call.  The kernel never writes what it reads: the state at the start of the chunk outlives the chunk.
struct SweepCarry {
    uint32_t frame0 = 0u;     // the clip's index of frames[0]; 0: that frame initialises the state and the in-planes are not read
    const void *lp_in = nullptr;   // [npx] of R
    const void *base_in = nullptr; // [T][npx] of R: column j's plane is 64 consecutive values to a wave
    void *lp_out = nullptr, *base_out = nullptr;
};

// One pixel through the F frames for TB columns.  CARRY = false is the whole clip (v2e_thres_sweep; cy is not read); CARRY = true
// is one chunk of it (v2e_thres_sweep_chunk): the state comes from and goes to SweepCarry's planes, the Philox keys use the clip's
// frame index frame0 + f, and a pixel's 32-bit ON / OFF registers hold the chunk's events only.  (One kernel template, not a body
// shared by two kernels: inlined from a function, the 16-column instantiations of the whole-clip kernel took 14 to 22 more
// registers; as a template parameter they keep the registers and occupancy they had without it, profiles/r18_sweep_stream.txt.)
template <typename R, int TB, bool SCALAR, bool CARRY>
__global__ __launch_bounds__(BLOCK) void k_sweep(SweepArgs a, SweepCarry cy)
{
    static_assert(TB >= 1 && TB <= 32, "one flag bit per column of the chunk");
    __shared__ float s_lutL[256];
    __shared__ double s_lutI[256];
    __shared__ unsigned long long s_sum[BLOCK / WAVE][TB][2];
    __shared__ uint32_t s_flag[BLOCK / WAVE];
    const int tid = threadIdx.x;
    // lin_log(x) and (x + 20) / 275 of the 256 grey levels, by the functions k_lut and the per-pixel path use
    s_lutL[tid] = lin_log((double)tid);
    s_lutI[tid] = ((double)tid + 20.0) / 275.0;
    __syncthreads();
    const int p = blockIdx.x * BLOCK + tid;
    const bool valid = p < a.npx;
    const int j0 = blockIdx.y * TB;
    const int px_x = p % a.W, px_y = p / a.W;
    const bool in_roi = valid && px_x >= a.x0 && px_x <= a.x1 && px_y >= a.y0 && px_y <= a.y1;
    const uint8_t *fp = a.frames + (valid ? p : 0);

    // ---- per pixel, the same for every column: the draws behind the thresholds and the noise rate (k_init)
    float n_pos = 0.f, n_neg = 0.f, n_rate = 0.f;
    v2e_draw_init(a.seed, 0u, (uint32_t)p, &n_pos, &n_neg, &n_rate);
    const float nr = a.do_leak ? v2e_det_expf(a.ln10cov_f * n_rate) : 0.f;
    const float lk = a.leak_hz_f * nr; // emulator_utils.py:126

    // ---- per column: thresholds, divisors and their reciprocals (a column beyond T repeats the last one; nothing of it is added)
    float thp[TB], thn[TB];
    R tpd_s[TB], tnd_s[TB]; // SCALAR: the divisors (wave-uniform); otherwise they are (R)thp, (R)thn
    R rtp[TB], rtn[TB];
    bool thr_bad = false; // guard of the reciprocal floor division: a threshold that is not positive takes the generic path
#pragma unroll
    for (int c = 0; c < TB; ++c) {
        const int j = min(j0 + c, a.T - 1);
        const double pj = a.pos[j], nj = a.neg[j];
        float tp, tn;
        if (!SCALAR) { // k_init
            tp = n_pos * a.sigma_f + (float)pj;
            tn = n_neg * a.sigma_f + (float)nj;
            tp = tp < 0.01f ? 0.01f : tp;
            tn = tn < 0.01f ? 0.01f : tn;
        } else {
            tp = (float)pj;
            tn = (float)nj;
        }
        thp[c] = tp;
        thn[c] = tn;
        const R tpd = SCALAR ? (R)pj : (R)tp; // emulator_utils.py:154-157 divisors (scalar thresholds: the Python doubles)
        const R tnd = SCALAR ? (R)nj : (R)tn;
        tpd_s[c] = tpd;
        tnd_s[c] = tnd;
        thr_bad = thr_bad || !(tpd > (R)0) || !(tnd > (R)0);
        rtp[c] = (R)1 / tpd;
        rtn[c] = (R)1 / tnd;
    }
    constexpr double QMAX = sizeof(R) == 8 ? 1.0e9 : 1.0e6; // quotients beyond it (and NaN) take the generic path

    // ---- the clip's first frame initialises the state and emits nothing (k_init); a later chunk takes up the carried state
    const bool first = !CARRY || cy.frame0 == 0u;
    const uint32_t g0 = CARRY ? cy.frame0 : 0u; // the emulator's frame index of frames[0]: the clip's first frame is 0, clip 0
    const int fs = first ? 1 : 0;               // the first frame that is an ordinary one
    R lp;
    if (first) {
        const int px = valid ? (int)fp[0] : 0;
        const double L = (double)s_lutL[px];
        if (a.has_cutoff) {
            double eps = s_lutI[px] * a.tab[0].dt_over_tau;
            if (eps > 1.0) eps = 1.0;
            lp = (R)((1.0 - eps) * L + eps * L);
        } else {
            lp = (R)L;
        }
    } else {
        lp = ((const R *)cy.lp_in)[valid ? p : 0];
    }
    R b[TB];
    uint32_t n_on[TB], n_off[TB];
#pragma unroll
    for (int c = 0; c < TB; ++c) { b[c] = lp; n_on[c] = 0u; n_off[c] = 0u; }
    if (CARRY && !first) {
#pragma unroll
        for (int c = 0; c < TB; ++c) b[c] = ((const R *)cy.base_in)[(size_t)min(j0 + c, a.T - 1) * a.npx + (valid ? p : 0)];
    }
    uint32_t flags = 0u; // bit c: the refractory rule would have switched on in column j0 + c

    // the draws of the current frame pair: made at the pair's first half, and at the first frame whichever half it is (a chunk may
    // begin on the second)
    float r_odd = 0.f, u_odd = 0.f, r_even = 0.f, u_even = 0.f;
    bool have_pair = false;
    int px_next = (valid && a.F > fs) ? (int)fp[(size_t)fs * a.npx] : 0;
    for (int f = fs; f < a.F; ++f) {
        const int px = px_next;
        if (valid && f + 1 < a.F) px_next = (int)fp[(size_t)(f + 1) * a.npx]; // (in flight while this frame is computed)
        const SweepFrame sf = a.tab[f];
        const uint32_t gf = g0 + (uint32_t)f;
        if (a.need_r) {                  // one Philox call per pair of frames (v2e_detmath.h)
            if (!have_pair || v2e_frame_half(gf) == 0u)
                v2e_draw_pair(a.seed, 0u, v2e_frame_pair(gf), (uint32_t)p, 1, &r_odd, &u_odd, &r_even, &u_even);
            have_pair = true;
        }
        const float rr = v2e_frame_half(gf) != 0u ? r_even : r_odd;
        // low_pass_filter (emulator_utils.py:69-104)
        const double L = (double)s_lutL[px];
        if (a.has_cutoff) {
            double eps = s_lutI[px] * sf.dt_over_tau;
            if (eps > 1.0) eps = 1.0;
            lp = (R)((1.0 - eps) * (double)lp + eps * L);
        } else {
            lp = (R)L;
        }
        const R photo = lp + (R)0.0f; // photoreceptor + photoreceptor_noise_arr (emulator.py:747-751)
        // emulator_utils.py:126-129, float32 left to right: all but the last factor
        const float rate = lk * (1.0f - a.jit_f * rr);
        const float dtr = sf.dtime_f * rate;
#pragma unroll
        for (int c = 0; c < TB; ++c) {
            R bc = b[c];
            if (a.do_leak) bc = bc - (R)(dtr * thp[c]); // emulator_utils.py:131
            const R diff = photo - bc;
            const bool is_pos = diff > (R)0;
            const R bt = is_pos ? (SCALAR ? tpd_s[c] : (R)thp[c]) : (SCALAR ? tnd_s[c] : (R)thn[c]);
            const R rbt = is_pos ? rtp[c] : rtn[c];
            const R am = sizeof(R) == 8 ? (R)__builtin_fabs((double)diff) : (R)__builtin_fabsf((float)diff);
            const R q0 = floor(am * rbt);
            const R r0 = fma(-q0, bt, am);
            int mag = (int)q0;
            mag -= (r0 < (R)0) ? 1 : 0;
            mag += (r0 >= bt) ? 1 : 0;
            if (__builtin_expect(!(q0 <= (R)QMAX) || thr_bad, 0)) {
                const R mg = is_pos ? diff : ((-diff) > (R)0 ? -diff : (R)0);
                const int q = (int)div_floor<R>(mg, bt);
                mag = q > 0 ? q : 0;
            }
            // emulator.py:936-942 with every candidate event surviving (the rule is off): base +- count * theta
            float d = (float)mag * (is_pos ? thp[c] : thn[c]);
            d = is_pos ? d : -d;
            b[c] = mag > 0 ? bc + (R)d : bc;
            if (in_roi) {
                n_on[c] += is_pos ? (uint32_t)mag : 0u;
                n_off[c] += is_pos ? 0u : (uint32_t)mag;
            }
            // emulator.py:830: on for this frame when max(1, M) >= refr_on_n
            if ((uint32_t)(mag > 1 ? mag : 1) >= sf.refr_on_n) flags |= 1u << c;
        }
    }
    if (!valid) flags = 0u;
    if (CARRY && valid) { // the state for the next chunk (lp is the same in every chunk of columns: the first one writes it)
        if (blockIdx.y == 0) ((R *)cy.lp_out)[p] = lp;
#pragma unroll
        for (int c = 0; c < TB; ++c)
            if (j0 + c < a.T) ((R *)cy.base_out)[(size_t)(j0 + c) * a.npx + p] = b[c];
    }

    // ---- wave sums, workgroup sums, one integer atomic per column and polarity.  64 lanes of 32-bit counts sum to up to 38 bits:
    // the 16-bit halves are summed apart (each sum stays below 2^22) and put together in 64 bits.
    const int lane = tid & (WAVE - 1), wid = tid / WAVE;
#pragma unroll
    for (int c = 0; c < TB; ++c) {
        const unsigned long long so = (unsigned long long)wave_sum_u32(n_on[c] & 0xFFFFu) + ((unsigned long long)wave_sum_u32(n_on[c] >> 16) << 16);
        const unsigned long long sf = (unsigned long long)wave_sum_u32(n_off[c] & 0xFFFFu) + ((unsigned long long)wave_sum_u32(n_off[c] >> 16) << 16);
        if (lane == 0) { s_sum[wid][c][0] = so; s_sum[wid][c][1] = sf; }
    }
    const uint32_t wf = wave_or_u32(flags);
    if (lane == 0) s_flag[wid] = wf;
    __syncthreads();
    if (tid < TB * 2) {
        const int c = tid >> 1, pol = tid & 1, j = j0 + c;
        unsigned long long s = 0ull;
#pragma unroll
        for (int w = 0; w < BLOCK / WAVE; ++w) s += s_sum[w][c][pol];
        if (j < a.T && s != 0ull) atomicAdd(&a.counts[(size_t)j * 2 + pol], s);
    } else if (tid >= WAVE && tid < WAVE + TB) {
        const int c = tid - WAVE, j = j0 + c;
        uint32_t fl = 0u;
#pragma unroll
        for (int w = 0; w < BLOCK / WAVE; ++w) fl |= s_flag[w];
        if (j < a.T && ((fl >> c) & 1u)) atomicOr(&a.rule_on[j], 1);
    }
}

typedef void (*SweepKernel)(SweepArgs, SweepCarry);

template <typename R, bool SCALAR, bool CARRY> SweepKernel pick_tb(int tb)
{
    switch (tb) {
    case 4: return k_sweep<R, 4, SCALAR, CARRY>;
    case 8: return k_sweep<R, 8, SCALAR, CARRY>;
    case 16: return k_sweep<R, 16, SCALAR, CARRY>;
    default: return nullptr;
    }
}

template <bool CARRY> SweepKernel pick_carry(bool f64, bool scalar, int tb)
{
    if (f64) return scalar ? pick_tb<double, true, CARRY>(tb) : pick_tb<double, false, CARRY>(tb);
    return scalar ? pick_tb<float, true, CARRY>(tb) : pick_tb<float, false, CARRY>(tb);
}

SweepKernel pick_kernel(bool f64, bool scalar, int tb, bool carry = false)
{
    return carry ? pick_carry<true>(f64, scalar, tb) : pick_carry<false>(f64, scalar, tb);
}

constexpr int SWEEP_TB_DEFAULT = 8; // columns per thread where the caller names none (profiles/r14_threshold_sweep.txt)

// The library's only private scratch of a sweep: the frame scalars and the thresholds of the call in flight, per device.  Calls on
// one stream reuse it in stream order; a call on another stream first waits for the stream that used it last.
struct SweepScratch {
    void *dev = nullptr;
    size_t cap = 0;
    hipStream_t last = nullptr;
    bool used = false;
};
std::mutex g_mu;
SweepScratch g_scratch[64];

// Both entry points.  cy == nullptr: the whole clip (CARRY = false; counts and flags start from zero); otherwise the chunk whose first frame
// is the clip's frame cy->frame0 (CARRY = true; counts are added to, flags OR-ed into).  t_previous: the emulator's t_previous when
// it is given frames[0] -- 0 for the clip's first two frames (the first frame does not advance it, emulator.py:717).
int sweep_enqueue(const void *frames, int frame_dtype, int F, int H, int W, const double *t_frames, const SweepCarry *cy, double t_previous,
                  const v2e_sweep_params *p, const double *pos, const double *neg, int T, const int roi[4], uint64_t *counts_dev,
                  int32_t *rule_on_dev, void *stream)
{
    const bool first = !cy || cy->frame0 == 0u; // frames[0] is the clip's first frame
    V2E_REQUIRE(frames && t_frames && p && pos && neg && roi && counts_dev && rule_on_dev, "null argument");
    V2E_REQUIRE(frame_dtype == V2E_DT_U8, "the sweep reads uint8 frames only");
    V2E_REQUIRE(F >= (cy ? 1 : 2), cy ? "a chunk needs at least one frame" : "a sweep needs at least two frames (the first one initialises the state)");
    V2E_REQUIRE(T >= 1, "no thresholds");
    V2E_REQUIRE(H > 0 && W > 0 && (long long)H * W <= 0x7FFFFF00ll, "bad sensor size");
    V2E_REQUIRE(roi[0] >= 0 && roi[0] <= roi[1] && roi[1] < W && roi[2] >= 0 && roi[2] <= roi[3] && roi[3] < H,
                "ROI (x0, x1, y0, y1; inclusive) is empty or outside the sensor");
    for (int j = 0; j < T; ++j)
        V2E_REQUIRE(pos[j] > 0 && neg[j] > 0 && std::isfinite(pos[j]) && std::isfinite(neg[j]), "thresholds must be positive and finite");
    V2E_REQUIRE(std::isfinite(p->sigma_thres) && p->sigma_thres >= 0 && std::isfinite(p->cutoff_hz) && p->cutoff_hz >= 0 &&
                std::isfinite(p->leak_rate_hz) && p->leak_rate_hz >= 0 && std::isfinite(p->refractory_period_s) &&
                p->refractory_period_s >= 0 && std::isfinite(p->leak_jitter_fraction) && std::isfinite(p->noise_rate_cov_decades),
                "bad model parameters");
    const int tb = p->cols_per_thread ? p->cols_per_thread : SWEEP_TB_DEFAULT;
    const bool f64 = p->cutoff_hz > 0, scalar = !(p->sigma_thres > 0);
    const SweepKernel kern = pick_kernel(f64, scalar, tb, cy != nullptr);
    V2E_REQUIRE(kern, "cols_per_thread must be 0 (default), 4, 8 or 16");
    V2E_REQUIRE((T + tb - 1) / tb <= 65535, "too many thresholds");
    if (cy) {
        V2E_REQUIRE(cy->lp_out && cy->base_out && (first || (cy->lp_in && cy->base_in)), "null state plane");
        V2E_REQUIRE(cy->lp_out != cy->lp_in && cy->base_out != cy->base_in, "the state is written to other planes than it is read from");
        V2E_REQUIRE((unsigned long long)cy->frame0 + (unsigned long long)F <= 0x7FFFFFFFull, "frame index out of range");
    }
    // a fresh emulator's frames: the first one at t[0] >= 0 = t_previous, which it does not advance (emulator.py:717); every
    // later one strictly after the one before
    V2E_REQUIRE(std::isfinite(t_frames[0]) && t_frames[0] >= 0, "the first frame time must be finite and not negative");
    V2E_REQUIRE(first ? t_previous == 0.0 : (std::isfinite(t_previous) && t_previous >= 0), "bad t_previous");
    std::vector<unsigned char> host(sizeof(SweepFrame) * (size_t)F + 2 * sizeof(double) * (size_t)T);
    SweepFrame *tab = (SweepFrame *)host.data();
    double *thr = (double *)(host.data() + sizeof(SweepFrame) * (size_t)F);
    double t_prev = t_previous;
    for (int f = 0; f < F; ++f) {
        V2E_REQUIRE(std::isfinite(t_frames[f]) && ((first && f == 0) || t_frames[f] > t_prev) && (f == 0 || t_frames[f] > t_frames[f - 1]),
                    "frame times must increase");
        const FrameCtl c = make_ctl(t_prev, t_frames[f], p->cutoff_hz, 0.0, p->refractory_period_s);
        tab[f].dt_over_tau = c.dt_over_tau;
        tab[f].dtime_f = (float)(c.t_frame - c.t_prev);
        tab[f].refr_on_n = c.refr_on_n;
        if (!(first && f == 0)) t_prev = t_frames[f];
    }
    for (int j = 0; j < T; ++j) { thr[j] = pos[j]; thr[T + j] = neg[j]; }

    hipStream_t s = (hipStream_t)stream;
    int dev = 0;
    V2E_HIP(hipGetDevice(&dev));
    V2E_REQUIRE(dev >= 0 && dev < 64, "device index out of range");
    std::lock_guard<std::mutex> lock(g_mu);
    SweepScratch &sc = g_scratch[dev];
    if (sc.used && sc.last != s) V2E_HIP(hipStreamSynchronize(sc.last));
    if (host.size() > sc.cap) {
        if (sc.used) V2E_HIP(hipStreamSynchronize(sc.last));
        if (sc.dev) V2E_HIP(hipFree(sc.dev));
        sc.dev = nullptr; sc.cap = 0;
        const size_t want = (host.size() + 4095) / 4096 * 4096;
        V2E_HIP(hipMalloc(&sc.dev, want));
        sc.cap = want;
    }
    sc.last = s; sc.used = true;
    // (pageable source: the copy has left `host` when the call returns)
    V2E_HIP(hipMemcpyAsync(sc.dev, host.data(), host.size(), hipMemcpyHostToDevice, s));
    if (!cy) {
        V2E_HIP(hipMemsetAsync(counts_dev, 0, sizeof(uint64_t) * 2 * (size_t)T, s));
        V2E_HIP(hipMemsetAsync(rule_on_dev, 0, sizeof(int32_t) * (size_t)T, s));
    }

    SweepArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = (const uint8_t *)frames; a.F = F; a.npx = H * W; a.W = W; a.T = T;
    a.x0 = roi[0]; a.x1 = roi[1]; a.y0 = roi[2]; a.y1 = roi[3];
    a.tab = (const SweepFrame *)sc.dev;
    a.pos = (const double *)((const unsigned char *)sc.dev + sizeof(SweepFrame) * (size_t)F);
    a.neg = a.pos + T;
    a.do_leak = p->leak_rate_hz > 0; a.has_cutoff = p->cutoff_hz > 0;
    a.sigma_f = (float)p->sigma_thres; a.leak_hz_f = (float)p->leak_rate_hz; a.jit_f = (float)p->leak_jitter_fraction;
    a.ln10cov_f = (float)(log(10.0) * p->noise_rate_cov_decades);
    a.need_r = a.do_leak && a.jit_f != 0.f;
    a.seed = p->seed;
    a.counts = (unsigned long long *)counts_dev; a.rule_on = (int *)rule_on_dev;
    const dim3 grid((unsigned)v2e_cdiv(a.npx, BLOCK), (unsigned)((T + tb - 1) / tb));
    kern<<<grid, BLOCK, 0, s>>>(a, cy ? *cy : SweepCarry());
    V2E_HIP(hipGetLastError());
    return 0;
}

int sweep_info(bool carry, int f64_state, int scalar_thres, int cols_per_thread, int *cols_out, int *vgprs, int *workgroups_per_cu)
{
    const int tb = cols_per_thread ? cols_per_thread : SWEEP_TB_DEFAULT;
    const SweepKernel kern = pick_kernel(f64_state != 0, scalar_thres != 0, tb, carry);
    V2E_REQUIRE(kern, "cols_per_thread must be 0 (default), 4, 8 or 16");
    if (cols_out) *cols_out = tb;
    if (vgprs) {
        hipFuncAttributes fa;
        V2E_HIP(hipFuncGetAttributes(&fa, (const void *)kern));
        *vgprs = fa.numRegs;
    }
    if (workgroups_per_cu) V2E_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(workgroups_per_cu, (const void *)kern, BLOCK, 0));
    return 0;
}

} // namespace

extern "C" {

int v2e_thres_sweep(const void *frames, int frame_dtype, int F, int H, int W, const double *t_frames, const v2e_sweep_params *p,
                    const double *pos, const double *neg, int T, const int roi[4], uint64_t *counts_dev, int32_t *rule_on_dev,
                    void *stream)
{
    return sweep_enqueue(frames, frame_dtype, F, H, W, t_frames, nullptr, 0.0, p, pos, neg, T, roi, counts_dev, rule_on_dev, stream);
}

int v2e_thres_sweep_chunk(const void *frames, int frame_dtype, int F, int H, int W, const double *t_frames, int64_t frame0,
                          double t_previous, const v2e_sweep_params *p, const double *pos, const double *neg, int T, const int roi[4],
                          const void *lp_in, const void *base_in, void *lp_out, void *base_out, uint64_t *counts_dev,
                          int32_t *rule_on_dev, void *stream)
{
    V2E_REQUIRE(frame0 >= 0 && frame0 <= 0x7FFFFFFFll, "frame0 out of range");
    SweepCarry cy;
    cy.frame0 = (uint32_t)frame0;
    cy.lp_in = lp_in; cy.base_in = base_in; cy.lp_out = lp_out; cy.base_out = base_out;
    return sweep_enqueue(frames, frame_dtype, F, H, W, t_frames, &cy, t_previous, p, pos, neg, T, roi, counts_dev, rule_on_dev, stream);
}

int v2e_thres_sweep_info(int f64_state, int scalar_thres, int cols_per_thread, int *cols_out, int *vgprs, int *workgroups_per_cu)
{
    return sweep_info(false, f64_state, scalar_thres, cols_per_thread, cols_out, vgprs, workgroups_per_cu);
}

int v2e_thres_sweep_chunk_info(int f64_state, int scalar_thres, int cols_per_thread, int *cols_out, int *vgprs, int *workgroups_per_cu)
{
    return sweep_info(true, f64_state, scalar_thres, cols_per_thread, cols_out, vgprs, workgroups_per_cu);
}

} // extern "C"
