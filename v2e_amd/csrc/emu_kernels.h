// emu_kernels.h -- the per-frame kernels of emu.hip (k_init .. k_frame_rows_to_host), their argument structs (FrameCtl, KArgs) and device
// helpers.  Not a translation unit: it opens emu.hip's anonymous namespace, which emu.hip closes behind emu_chain.h.
#include "emu_shared.h" // BLOCK, WAVE, FrameCtl / make_ctl, LINLOG_F, lin_log, div_floor, wave_sum_u32, wave_or_u32 (shared with sweep.hip)

namespace {

constexpr int RING = 64;        // record / control ring for the frame-at-a-time API
constexpr int SCAN_BLOCKS = 64; // workgroups of k_scan per clip
constexpr int STAMP_LAUNCHES = 128; // chain launches of one run that v2e_emu_launch_stamps keeps

// packed per-pixel scratch word written by k_count
constexpr uint32_t CNT_MASK = 0x00FFFFFFu;
constexpr uint32_t CNT_NEG = 1u << 24;
constexpr uint32_t CNT_SHOT_ON = 1u << 25;
constexpr uint32_t CNT_SHOT_OFF = 1u << 26;
// The chain's ring (RunScratch::ch_cnt) keeps a 16-bit word per (frame, pixel) instead: its count saturates at CCNT_MASK.  A frame
// with a pixel beyond max_iters <= CHAIN_MAX_ITERS (emu_chain.h) is refused, a saturated one with it; the chain advances the pixel
// state from the count in its registers, never from the word.
typedef uint16_t ccnt_t;
constexpr uint32_t CCNT_MASK = 0x1FFFu;
constexpr uint32_t CCNT_NEG = 1u << 13;
constexpr uint32_t CCNT_SHOT_ON = 1u << 14;
constexpr uint32_t CCNT_SHOT_OFF = 1u << 15;

struct KArgs {
    int W, npx, nwaves, nkeys_cap, max_iters;
    long long npx_pad;
    int scalar_thres, rng_mode, shuffle;
    int do_leak, do_shot, use_inten, has_cutoff, has_refr, log_input;
    double cutoff_two_pi; // math.pi*2*cutoff_hz
    double pos_div, neg_div;
    float pos_nom_f, neg_nom_f, pos_pre_scalar, neg_pre_scalar;
    float leak_hz_f, jit_f;
    float sigma_f, pos_mean_f, neg_mean_f, ln10cov_f;
    double shot_half_rate, inten_slope;
    double refr;
    float refr_f;
    unsigned long long seed;
    // state planes
    void *lp, *base;
    float *ts_mem, *pos_thres, *neg_thres, *noise_rate;
    // scratch
    uint32_t *cnt;
    uint32_t *hist; // [n_clips][nkeys_cap][nwaves]
    uint32_t *tot;  // [n_clips][nkeys_cap]
    // lin_log / inten01 of the 256 uint8 grey levels, built on device by k_lut with the same code
    const float *lut_L;
    const double *lut_I;
    // photoreceptor noise (frame-at-a-time API): state plane, tape draws (or nullptr), vrms as float32
    void *pn_arr;
    const float *pn_tape;
    float pn_vrms_f;
    // SCIDVS (emulator.py:56-80, 719-725; float64 state only): high-pass state, previous photoreceptor value, time constants
    void *sc_hp, *sc_prev;
    float *sc_tau;
    uint32_t sc_first_frame; // frame index at which scidvs_previous_photo is taken from the frame itself
    const void *cs_sur; // CSDVS: the surround plane the frame's photoreceptor output is compared against (emulator.py:753-754)
    int emit_guard; // k_emit: leave everything untouched (flag the record) when the frame's rows do not fit the buffer
    // model-state planes the reference keeps as attributes but the kernels otherwise never store (emulator.py:666, 749-754;
    // show_dvs_model_state, record_single_pixel_states): float64 [n_clips][npx_pad] each, written by k_count, nullptr = off
    double *dbg_lognew, *dbg_cms, *dbg_diff;
};

__device__ constexpr double SCIDVS_EFOLD = 1 / 0.7; // efold of the sinh conductance (emulator.py:78)

// ------------------------------------------------------------------ helpers
// (the DPP reductions shared with sweep.hip -- wave_sum_u32, wave_or_u32 -- and V2E_DPP: emu_shared.h)
__device__ __forceinline__ int wave_max_i32(int v)
{
    v = max(v, V2E_DPP(v, 0xB1));  // quad_perm [1,0,3,2]
    v = max(v, V2E_DPP(v, 0x4E));  // quad_perm [2,3,0,1]
    v = max(v, V2E_DPP(v, 0x141)); // row_half_mirror
    v = max(v, V2E_DPP(v, 0x140)); // row_mirror
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// exclusive prefix sum across the 64 lanes: Hillis-Steele inside each 16-lane row with
// row_shr DPP (zero fill), row carries through v_readlane + scalar adds
__device__ __forceinline__ uint32_t wave_excl_scan_u32(uint32_t u, int lane)
{
    int inc = (int)u;
    inc += V2E_DPP(inc, 0x111); // row_shr:1
    inc += V2E_DPP(inc, 0x112); // row_shr:2
    inc += V2E_DPP(inc, 0x114); // row_shr:4
    inc += V2E_DPP(inc, 0x118); // row_shr:8
    const int t0 = __builtin_amdgcn_readlane(inc, 15), t1 = __builtin_amdgcn_readlane(inc, 31),
              t2 = __builtin_amdgcn_readlane(inc, 47);
    const int row = lane >> 4;
    const int off = row == 0 ? 0 : (row == 1 ? t0 : (row == 2 ? t0 + t1 : t0 + t1 + t2));
    return (uint32_t)(inc + off) - u;
}

// value of lane `idx` (idx wave-uniform) as a scalar
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int idx)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(idx));
}

// shot-noise decision, emulator_utils.py:326-349 (float64 compare of a float32 draw)
__device__ __forceinline__ uint32_t shot_bits(const KArgs &a, double inten01, double shot_base,
                                              float thp, float thn, float u)
{
    double F = shot_base * (a.inten_slope * inten01 + 1);
    float ppre = a.scalar_thres ? a.pos_pre_scalar : a.pos_nom_f / thp;
    float npre = a.scalar_thres ? a.neg_pre_scalar : a.neg_nom_f / thn;
    double on_thr = 1 - F * (double)ppre;
    double off_thr = F * (double)npre;
    uint32_t b = 0;
    if ((double)u > on_thr) b |= CNT_SHOT_ON;
    if ((double)u < off_thr) b |= CNT_SHOT_OFF;
    return b;
}

// timestamps of the n iterations of one frame (emulator.py:791-796)
struct TsGen {
    const float *tab;
    float start, end, step;
    uint32_t n;
    __device__ __forceinline__ TsGen(const FrameCtl &c, int n_, const float *tab_) : tab(tab_), n((uint32_t)n_)
    {
        double dt = c.t_frame - c.t_prev;
        double ts_step = dt / (double)n_;
        start = (float)(c.t_prev + ts_step);
        end = (float)c.t_frame;
        step = (n_ > 1) ? (end - start) / (float)(n_ - 1) : 0.0f;
    }
    __device__ __forceinline__ TsGen(float start_, float end_, float step_, int n_) : tab(nullptr), start(start_), end(end_), step(step_), n((uint32_t)n_) {}
    __device__ __forceinline__ float operator()(int i) const
    {
        return tab ? tab[i] : v2e_ts_formula((uint32_t)i, n, start, end, step);
    }
};

// lin_log(x) and (x+20)/275 for x = 0..255, evaluated by the very functions the per-pixel path
// uses, so a lookup returns bit-identical values (uint8 frames only)
__global__ void k_lut(float *lut_L, double *lut_I)
{
    const int i = threadIdx.x;
    const double x = (double)i;
    lut_L[i] = lin_log(x);
    lut_I[i] = (x + 20.0) / 275.0;
}

// ------------------------------------------------------------------ k_init
template <typename R, typename FT>
__global__ __launch_bounds__(BLOCK) void k_init(KArgs a, const FT *__restrict__ frame, double t_frame,
                                                const float *__restrict__ tp_tape,
                                                const float *__restrict__ tn_tape,
                                                const float *__restrict__ nr_tape)
{
    const int clip = blockIdx.y;
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.npx) return;
    const size_t sp = (size_t)clip * a.npx_pad + p;
    const size_t fp = (size_t)clip * a.npx + p;
    double x = (double)frame[fp];
    const double L = a.log_input ? x : (double)lin_log(x); // emulator.py:666
    R lp;
    if (a.has_cutoff) {
        double delta_time = t_frame - 0.0;
        double tau = 1.0 / a.cutoff_two_pi;
        double dt_over_tau = delta_time / tau;
        double inten01 = (x + 20.0) / 275.0;
        double eps = inten01 * dt_over_tau;
        if (eps > 1.0) eps = 1.0;
        lp = (R)((1.0 - eps) * (double)L + eps * (double)L);
    } else {
        lp = (R)L;
    }
    ((R *)a.lp)[sp] = lp;
    ((R *)a.base)[sp] = lp;
    float n_pos = 0.f, n_neg = 0.f, n_rate = 0.f;
    if (a.rng_mode == V2E_RNG_PHILOX)
        v2e_draw_init(a.seed, (uint32_t)clip, (uint32_t)p, &n_pos, &n_neg, &n_rate);
    float tp, tn;
    if (!a.scalar_thres) {
        if (a.rng_mode == V2E_RNG_PHILOX) {
            tp = n_pos * a.sigma_f + a.pos_mean_f;
            tn = n_neg * a.sigma_f + a.neg_mean_f;
        } else {
            tp = tp_tape[fp];
            tn = tn_tape[fp];
        }
        tp = tp < 0.01f ? 0.01f : tp;
        tn = tn < 0.01f ? 0.01f : tn;
    } else {
        tp = a.pos_mean_f;
        tn = a.neg_mean_f;
    }
    a.pos_thres[sp] = tp;
    a.neg_thres[sp] = tn;
    if (a.do_leak)
        a.noise_rate[sp] = (a.rng_mode == V2E_RNG_PHILOX) ? v2e_det_expf(a.ln10cov_f * n_rate) : nr_tape[fp];
    if (a.has_refr) a.ts_mem[sp] = 0.0f - a.refr_f;
    if (a.sc_hp) { // scidvs_highpass = zeros_like(lp); tau = SCIDVS_TAU_S * exp(normal(0, SCIDVS_TAU_COV)) (emulator.py:480-483, 719-722)
        ((R *)a.sc_hp)[sp] = (R)0;
        ((R *)a.sc_prev)[sp] = (R)0;
        if (a.rng_mode == V2E_RNG_PHILOX) a.sc_tau[sp] = 0.01f * v2e_det_expf(0.5f * v2e_draw_scidvs(a.seed, (uint32_t)clip, (uint32_t)p));
    }
}

// low_pass_filter (emulator_utils.py:69-104) of one pixel: the new lp_log_frame value
template <typename R>
__device__ __forceinline__ R lp_next(const KArgs &a, double L, double inten01, double delta_time, size_t sp)
{
    if (a.has_cutoff) { // R == double
        double tau = 1.0 / a.cutoff_two_pi;
        double dt_over_tau = delta_time / tau;
        double eps = inten01 * dt_over_tau;
        if (eps > 1.0) eps = 1.0;
        return (R)((1.0 - eps) * (double)((R *)a.lp)[sp] + eps * (double)L);
    }
    return (R)L;
}

// CSDVS: the frame's lp_log_frame BEFORE the frame is counted -- the surround's diffuser is stepped against it
// (emulator.py:707-708 sits between the low-pass and the event computation); k_count recomputes the same value
template <typename R, typename FT>
__global__ __launch_bounds__(BLOCK) void k_cs_lp(KArgs a, const FT *__restrict__ frame, const FrameCtl *__restrict__ ctl, R *__restrict__ out)
{
    const int clip = blockIdx.y;
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.npx) return;
    const FrameCtl c = ctl[clip];
    const size_t sp = (size_t)clip * a.npx_pad + p;
    const double x = (double)frame[(size_t)clip * a.npx + p];
    const double L = a.log_input ? x : (double)lin_log(x);
    const double inten01 = a.use_inten ? (x + 20.0) / 275.0 : 0.0;
    out[sp] = lp_next<R>(a, L, inten01, c.t_frame - c.t_prev, sp);
}

// ----------------------------------------------------------------- k_count
template <typename R, typename FT>
__global__ __launch_bounds__(BLOCK) void k_count(KArgs a, const FT *__restrict__ frame,
                                                 const FrameCtl *__restrict__ ctl,
                                                 const uint32_t *__restrict__ fidx_base, uint32_t fidx_off,
                                                 const float *__restrict__ leak_tape,
                                                 const float *__restrict__ shot_tape, v2e_frame_rec *rec,
                                                 const FrameCtl *__restrict__ ctl_host, FrameCtl *ctl_copy,
                                                 double t_prev_v, double t_frame_v)
{
    __shared__ int smax[BLOCK / WAVE];
    const int clip = blockIdx.y;
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    // ctl == nullptr (v2e_emu_frame): the frame's times arrive by value, and workgroup 0 copies the frame's scalars from pinned
    // host memory (ctl_host) to device memory (ctl_copy) for the kernels behind this one -- no launch of its own for that
    double delta_time_v = t_frame_v - t_prev_v;
    if (ctl) delta_time_v = ctl[clip].t_frame - ctl[clip].t_prev;
    else if (ctl_host && blockIdx.x == 0 && clip == 0 && threadIdx.x < sizeof(FrameCtl) / 4)
        ((uint32_t *)ctl_copy)[threadIdx.x] = ((const uint32_t *)ctl_host)[threadIdx.x];
    const uint32_t frame_idx = (fidx_base ? *fidx_base : 0u) + fidx_off;
    int m = 0;
    if (p < a.npx) {
        const size_t sp = (size_t)clip * a.npx_pad + p;
        const size_t fp = (size_t)clip * a.npx + p;
        const double delta_time = delta_time_v;
        double x = (double)frame[fp];
        const double L = a.log_input ? x : (double)lin_log(x); // emulator.py:666
        double inten01 = a.use_inten ? (x + 20.0) / 275.0 : 0.0;
        float r = 0.f, u = 0.f;
        const bool shot_here = a.do_shot && (a.rng_mode == V2E_RNG_PHILOX || shot_tape != nullptr);
        if (a.rng_mode == V2E_RNG_PHILOX) {
            if ((a.do_leak && a.jit_f != 0.f) || a.do_shot)
                v2e_draw_frame(a.seed, (uint32_t)clip, frame_idx, (uint32_t)p, &r, &u);
        } else {
            if (a.do_leak) r = leak_tape[fp];
            if (shot_here) u = shot_tape[fp];
        }
        const float thp = a.pos_thres[sp], thn = a.neg_thres[sp];
        float delta_leak = 0.f;
        if (a.do_leak) { // emulator_utils.py:126-129, float32 left to right
            float rate = (a.leak_hz_f * a.noise_rate[sp]) * (1.0f - a.jit_f * r);
            delta_leak = ((float)delta_time * rate) * thp;
        }
        const R lpn = lp_next<R>(a, L, inten01, delta_time, sp);
        ((R *)a.lp)[sp] = lpn;
        R b = ((R *)a.base)[sp];
        if (a.do_leak) {
            b = b - (R)delta_leak;
            ((R *)a.base)[sp] = b;
        }
        R pn = (R)0.0f;
        if (a.pn_arr) { // emulator.py:694-701: float32 white noise through low_pass_filter(noise, arr, None, dt, cutoff)
            const float rn = a.rng_mode == V2E_RNG_PHILOX ? v2e_draw_pnoise(a.seed, (uint32_t)clip, frame_idx, (uint32_t)p) : a.pn_tape[fp];
            const float noise = a.pn_vrms_f * rn;                // python float * float32 tensor
            const double eps_n = delta_time / (1.0 / a.cutoff_two_pi); // emulator_utils.py:97, not clamped
            const float term2 = (float)eps_n * noise;            // eps * float32 tensor
            const double pnn = (1.0 - eps_n) * (double)((R *)a.pn_arr)[sp] + (double)term2;
            ((R *)a.pn_arr)[sp] = (R)pnn;
            pn = (R)pnn;
        }
        R photo = lpn;
        if (a.sc_hp) { // SCIDVS: nonlinear CR high-pass of the photoreceptor, amplified (emulator.py:719-725, 747; R == double)
            const R prev = frame_idx == a.sc_first_frame ? lpn : ((R *)a.sc_prev)[sp]; // first frame: clone of lp_log_frame
            R hp = ((R *)a.sc_hp)[sp];
            const float inv_tau = 1.0f / a.sc_tau[sp];                  // torch.div(1, tau): float32
            if constexpr (sizeof(R) == 8) {
                const R sh = (R)sinh((double)hp / SCIDVS_EFOLD);         // torch.sinh(v / efold)
                const R dvdt = (R)inv_tau * sh;
                hp = hp + ((lpn - prev) - (R)(delta_time * (double)dvdt));
            } else { // float32 state: every operand is a float32 tensor, Python scalars take the tensor's type; torch's
                     // vectorised float32 sinh is Sleef's sinhf_u10, restated bit for bit in v2e_detmath.h
                const float sh = v2e_sleef_sinhf((float)hp / (float)SCIDVS_EFOLD);
                const float dvdt = inv_tau * sh;
                hp = (R)((float)hp + (((float)lpn - (float)prev) - ((float)delta_time * dvdt)));
            }
            ((R *)a.sc_hp)[sp] = hp;
            ((R *)a.sc_prev)[sp] = lpn;
            photo = (R)2 * hp;                                           // SCIDVS_GAIN * scidvs_highpass
        }
        R diff = (photo + pn) - b; // photoreceptor + photoreceptor_noise_arr - base_log_frame (emulator.py:747-751)
        if (a.cs_sur) diff = ((photo + pn) - ((const R *)a.cs_sur)[sp]) - b; // c_minus_s_frame - base_log_frame (:753-754)
        if (a.dbg_diff) {
            a.dbg_lognew[sp] = L;
            a.dbg_cms[sp] = a.cs_sur ? (double)((photo + pn) - ((const R *)a.cs_sur)[sp]) : 0.0;
            a.dbg_diff[sp] = (double)diff;
        }
        R pf = diff > (R)0 ? diff : (R)0;
        R nf = (-diff) > (R)0 ? -diff : (R)0;
        R tpd = a.scalar_thres ? (R)a.pos_div : (R)thp;
        R tnd = a.scalar_thres ? (R)a.neg_div : (R)thn;
        int pc = (int)div_floor<R>(pf, tpd);
        int nc = (int)div_floor<R>(nf, tnd);
        uint32_t w = 0;
        if (pc > 0) w = (uint32_t)pc & CNT_MASK;
        else if (nc > 0) w = ((uint32_t)nc & CNT_MASK) | CNT_NEG;
        if (shot_here) {
            double shot_base = a.shot_half_rate * delta_time;
            w |= shot_bits(a, inten01, shot_base, thp, thn, u);
        }
        a.cnt[sp] = w;
        m = pc > nc ? pc : nc;
    }
    m = wave_max_i32(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) smax[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        int bm = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
        if (bm > 0) atomicMax(&rec[clip].max_events, bm);
    }
}

// ------------------------------------------------------------------ k_shot
template <typename FT>
__global__ __launch_bounds__(BLOCK) void k_shot(KArgs a, const FT *__restrict__ frame,
                                                const FrameCtl *__restrict__ ctl,
                                                const float *__restrict__ shot_tape)
{
    const int clip = blockIdx.y;
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= a.npx) return;
    const FrameCtl c = ctl[clip];
    const size_t sp = (size_t)clip * a.npx_pad + p;
    const size_t fp = (size_t)clip * a.npx + p;
    double x = (double)frame[fp];
    double inten01 = (x + 20.0) / 275.0;
    double shot_base = a.shot_half_rate * (c.t_frame - c.t_prev);
    uint32_t w = a.cnt[sp] & ~(CNT_SHOT_ON | CNT_SHOT_OFF);
    w |= shot_bits(a, inten01, shot_base, a.pos_thres[sp], a.neg_thres[sp], shot_tape[fp]);
    a.cnt[sp] = w;
}

// ------------------------------------------------------------------ k_rank
// One wave = 64 consecutive pixels.  For every iteration i < M the wave counts its
// surviving ON and OFF events (keys 2i, 2i+1); keys 2M, 2M+1 are the shot pair.
__global__ __launch_bounds__(BLOCK) void k_rank(KArgs a, const FrameCtl *__restrict__ ctl,
                                                const v2e_frame_rec *__restrict__ rec,
                                                const float *__restrict__ ts_tab, int n_ts)
{
    const int clip = blockIdx.y;
    const int lane = threadIdx.x & (WAVE - 1);
    const int w = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    if (w >= a.nwaves) return;
    const int p = w * WAVE + lane;
    const int M = rec[clip].max_events;
    if (M > a.max_iters) return;
    const int n = M > 0 ? M : 1;
    const FrameCtl c = ctl[clip];
    const TsGen tg(c, n, ts_tab ? ts_tab + (size_t)clip * n_ts : nullptr);
    const bool use_refr = a.has_refr && (a.refr > (c.t_frame - c.t_prev) / (double)n);
    const size_t sp = (size_t)clip * a.npx_pad + p;
    const uint32_t cw = p < a.npx ? a.cnt[sp] : 0u;
    const int mag = (int)(cw & CNT_MASK);
    const bool neg = (cw & CNT_NEG) != 0;
    float tsm = (use_refr && p < a.npx) ? a.ts_mem[sp] : 0.f;
    uint32_t *hrow = a.hist + (size_t)clip * a.nkeys_cap * a.nwaves;
    bool alive = true; // some lane of the wave still has a candidate at this iteration
    for (int kb = 0; kb < 2 * M; kb += WAVE) {
        uint32_t mine = 0;
        const int i0 = kb >> 1;
        for (int ii = 0; ii < WAVE / 2 && i0 + ii < M && alive; ++ii) {
            const int i = i0 + ii;
            const bool cand = mag > i;
            if (__ballot(cand) == 0ull) { alive = false; break; }
            bool pass = cand;
            if (use_refr) {
                const float t = tg(i);
                const float pt = (cand ? 1.0f : 0.0f) * t - tsm;
                pass = pt > a.refr_f;
                if (pass) tsm = t;
            }
            const unsigned long long bo = __ballot(pass && !neg);
            const unsigned long long bf = __ballot(pass && neg);
            if (lane == 2 * ii) mine = (uint32_t)__popcll(bo);
            if (lane == 2 * ii + 1) mine = (uint32_t)__popcll(bf);
        }
        const int key = kb + lane;
        if (key < 2 * M) hrow[(size_t)key * a.nwaves + w] = mine;
    }
    const unsigned long long so = __ballot((cw & CNT_SHOT_ON) != 0);
    const unsigned long long sf = __ballot((cw & CNT_SHOT_OFF) != 0);
    if (lane == 0) hrow[(size_t)(2 * M) * a.nwaves + w] = (uint32_t)__popcll(so);
    if (lane == 1) hrow[(size_t)(2 * M + 1) * a.nwaves + w] = (uint32_t)__popcll(sf);
}

// ------------------------------------------------------------------ k_scan
// One workgroup per key: in-place exclusive scan over the per-wave counts, total to tot[].
__global__ __launch_bounds__(BLOCK) void k_scan(KArgs a, const v2e_frame_rec *__restrict__ rec)
{
    __shared__ uint32_t wsum[BLOCK / WAVE];
    const int clip = blockIdx.y;
    const int M = rec[clip].max_events;
    if (M > a.max_iters) return;
    const int nkeys = 2 * M + 2;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const int ipt = (a.nwaves + BLOCK - 1) / BLOCK;
    for (int key = blockIdx.x; key < nkeys; key += gridDim.x) {
        uint32_t *row = a.hist + ((size_t)clip * a.nkeys_cap + key) * a.nwaves;
        const int b = tid * ipt, e = min(b + ipt, a.nwaves);
        uint32_t s = 0;
        for (int j = b; j < e; ++j) s += row[j];
        const uint32_t ex = wave_excl_scan_u32(s, lane);
        if (lane == WAVE - 1) wsum[wid] = ex + s;
        __syncthreads();
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (int q = 0; q < BLOCK / WAVE; ++q) {
            if (q < wid) wbase += wsum[q];
            total += wsum[q];
        }
        uint32_t run = wbase + ex;
        for (int j = b; j < e; ++j) {
            const uint32_t v = row[j];
            row[j] = run;
            run += v;
        }
        if (tid == 0) a.tot[(size_t)clip * a.nkeys_cap + key] = total;
        __syncthreads();
    }
}

// ------------------------------------------------------------------ k_emit
template <typename R>
__global__ __launch_bounds__(BLOCK) void k_emit(KArgs a, const FrameCtl *__restrict__ ctl, v2e_frame_rec *rec,
                                                const v2e_frame_rec *__restrict__ rec_prev,
                                                const unsigned long long *__restrict__ ev_offset0,
                                                const uint32_t *__restrict__ fidx_base, uint32_t fidx_off,
                                                const float *__restrict__ ts_tab, int n_ts,
                                                float4 *__restrict__ events, unsigned long long cap)
{
    const int clip = blockIdx.y;
    const int lane = threadIdx.x & (WAVE - 1);
    const int w = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    if (w >= a.nwaves) return;
    const int p = w * WAVE + lane;
    const uint32_t frame_idx = (fidx_base ? *fidx_base : 0u) + fidx_off;
    const int M = rec[clip].max_events;
    unsigned long long ev0 = 0;
    if (ev_offset0) ev0 = ev_offset0[clip];
    else if (rec_prev) ev0 = rec_prev[clip].ev_offset + rec_prev[clip].n_events;
    if (M > a.max_iters) {
        if (w == 0 && lane == 0) {
            rec[clip].flags |= V2E_FLAG_ITERS_CLAMPED;
            rec[clip].ev_offset = ev0;
        }
        return;
    }
    const uint32_t *trow = a.tot + (size_t)clip * a.nkeys_cap;
    if (a.emit_guard) { // speculative launch (v2e_emu_frame): the host has not seen the totals yet
        uint32_t tsum = 0;
        for (int kb = 0; kb < 2 * M + 2; kb += WAVE) tsum += kb + lane < 2 * M + 2 ? trow[kb + lane] : 0u;
        if (ev0 + wave_sum_u32(tsum) > cap) {
            if (w == 0 && lane == 0) {
                rec[clip].flags |= V2E_FLAG_EVENTS_DROPPED;
                rec[clip].ev_offset = ev0;
            }
            return;
        }
    }
    const int n = M > 0 ? M : 1;
    const FrameCtl c = ctl[clip];
    const TsGen tg(c, n, ts_tab ? ts_tab + (size_t)clip * n_ts : nullptr);
    const bool use_refr = a.has_refr && (a.refr > (c.t_frame - c.t_prev) / (double)n);
    const size_t sp = (size_t)clip * a.npx_pad + p;
    const bool valid = p < a.npx;
    const uint32_t cw = valid ? a.cnt[sp] : 0u;
    const int mag = (int)(cw & CNT_MASK);
    const bool neg = (cw & CNT_NEG) != 0;
    float tsm = (use_refr && valid) ? a.ts_mem[sp] : 0.f;
    const uint32_t *hrow = a.hist + (size_t)clip * a.nkeys_cap * a.nwaves;
    float4 *ev = events + (size_t)clip * cap;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const float fx = (float)(p % a.W), fy = (float)(p / a.W);
    const bool shuf = (a.rng_mode == V2E_RNG_PHILOX) && a.shuffle;
    uint32_t carry = 0;          // events of all earlier iterations (whole frame)
    uint32_t sum_on = 0, sum_off = 0;
    int fcount = 0;              // this pixel's surviving events
    bool dropped = false;
    bool alive = true;
    for (int kb = 0; kb < 2 * M; kb += WAVE) {
        const int key = kb + lane;
        const uint32_t t_k = key < 2 * M ? trow[key] : 0u;
        const uint32_t o_k = key < 2 * M ? hrow[(size_t)key * a.nwaves + w] : 0u;
        const uint32_t kb_k = carry + wave_excl_scan_u32(t_k, lane);
        const uint32_t chunk_total = wave_sum_u32(t_k);
        sum_on += wave_sum_u32((lane & 1) ? 0u : t_k);
        sum_off += wave_sum_u32((lane & 1) ? t_k : 0u);
        const int i0 = kb >> 1;
        for (int ii = 0; ii < WAVE / 2 && i0 + ii < M && alive; ++ii) {
            const int i = i0 + ii;
            const bool cand = mag > i;
            if (__ballot(cand) == 0ull) { alive = false; break; }
            const float t = tg(i);
            bool pass = cand;
            if (use_refr) {
                const float pt = (cand ? 1.0f : 0.0f) * t - tsm;
                pass = pt > a.refr_f;
                if (pass) tsm = t;
            }
            const unsigned long long bo = __ballot(pass && !neg);
            const unsigned long long bf = __ballot(pass && neg);
            if ((bo | bf) == 0ull) continue;
            const uint32_t it_base = lane_value(kb_k, 2 * ii);
            const uint32_t tot_on = lane_value(t_k, 2 * ii);
            const uint32_t tot_off = lane_value(t_k, 2 * ii + 1);
            const uint32_t off_on = lane_value(o_k, 2 * ii);
            const uint32_t off_off = lane_value(o_k, 2 * ii + 1);
            if (pass) {
                uint32_t cidx = neg ? tot_on + off_off + (uint32_t)__popcll(bf & lt)
                                    : off_on + (uint32_t)__popcll(bo & lt);
                if (shuf) {
                    v2e_perm_t pm;
                    v2e_perm_init(&pm, a.seed, (uint32_t)clip, frame_idx, (uint32_t)i, tot_on + tot_off);
                    cidx = v2e_perm_apply(&pm, cidx);
                }
                const unsigned long long row = ev0 + it_base + cidx;
                if (row < cap) ev[row] = make_float4(t, fx, fy, neg ? -1.0f : 1.0f);
                else dropped = true;
                ++fcount;
            }
        }
        carry += chunk_total;
    }
    // shot-noise events: after all signal events, ON block then OFF block, ts[-1], unshuffled
    const uint32_t son_tot = trow[2 * M], soff_tot = trow[2 * M + 1];
    if (a.do_shot) {
        const bool s_on = (cw & CNT_SHOT_ON) != 0, s_off = (cw & CNT_SHOT_OFF) != 0;
        const unsigned long long so = __ballot(s_on), sf = __ballot(s_off);
        if (so | sf) {
            const float tl = tg(n - 1);
            if (s_on) {
                const unsigned long long row = ev0 + carry + hrow[(size_t)(2 * M) * a.nwaves + w] + (uint32_t)__popcll(so & lt);
                if (row < cap) ev[row] = make_float4(tl, fx, fy, 1.0f);
                else dropped = true;
            }
            if (s_off) {
                const unsigned long long row = ev0 + carry + son_tot + hrow[(size_t)(2 * M + 1) * a.nwaves + w] + (uint32_t)__popcll(sf & lt);
                if (row < cap) ev[row] = make_float4(tl, fx, fy, -1.0f);
                else dropped = true;
            }
        }
    }
    // emulator.py:936-942
    if (valid) {
        const bool shot = a.do_shot && (cw & (CNT_SHOT_ON | CNT_SHOT_OFF));
        if (fcount > 0 || shot) {
            R b = ((R *)a.base)[sp];
            const float dp = (float)(neg ? 0 : fcount) * a.pos_thres[sp];
            const float dn = (float)(neg ? fcount : 0) * a.neg_thres[sp];
            b = b + (R)dp;
            b = b - (R)dn;
            if (shot) b = ((R *)a.lp)[sp];
            ((R *)a.base)[sp] = b;
        }
        if (use_refr && fcount > 0) a.ts_mem[sp] = tsm;
    }
    if (__ballot(dropped) != 0ull && lane == 0) atomicOr(&rec[clip].flags, V2E_FLAG_EVENTS_DROPPED);
    if (w == 0 && lane == 0) {
        rec[clip].n_signal = carry;
        rec[clip].n_events = carry + (a.do_shot ? son_tot + soff_tot : 0u);
        rec[clip].n_on = sum_on + (a.do_shot ? son_tot : 0u);
        rec[clip].n_off = sum_off + (a.do_shot ? soff_tot : 0u);
        rec[clip].ev_offset = ev0;
    }
}

// out[row0 + j] = in[row0 + idx[j]]  (events_curr_iter[idx], emulator.py:869)
__global__ __launch_bounds__(BLOCK) void k_permute(const float4 *__restrict__ in, float4 *__restrict__ out,
                                                   const int32_t *__restrict__ idx, unsigned long long row0,
                                                   unsigned long long n)
{
    const unsigned long long j = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j < n) out[row0 + j] = in[row0 + (unsigned long long)idx[j]];
}

// ------------------------------------------------------------------ v2e_emu_frame's two ends
// Everything a frame needs goes through the compute queue: a copy engine between kernels costs a cross-queue dependency at
// either end (~20 us each on this runtime), more than the whole frame's kernels.  The frame's scalars arrive as a kernel
// argument, its pixels are read by k_count straight from the pinned staging buffer, and the rows go back by a kernel writing
// pinned host memory.
struct FrameScratch { // device
    v2e_frame_rec rec[2]; // alternating between calls: a frame's last kernel zeroes the one the next frame counts into
    FrameCtl ctl;         // the frame's scalars, copied from pinned host memory by k_count's workgroup 0
};

// rows [row0, min(n_events, row0 + max_rows)) of the frame to the pinned host buffer, and the frame record with them
__global__ __launch_bounds__(256) void k_frame_rows_to_host(const float4 *__restrict__ ev, const v2e_frame_rec *__restrict__ rec,
                                                            float4 *__restrict__ out_rows, v2e_frame_rec *__restrict__ out_rec,
                                                            unsigned long long row0, unsigned long long max_rows,
                                                            v2e_frame_rec *__restrict__ rec_next)
{
    const v2e_frame_rec r = *rec;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (out_rec) *out_rec = r;
        if (rec_next) { // the record the NEXT frame's k_count takes its maximum in (nobody in this launch reads it)
            v2e_frame_rec z;
            memset(&z, 0, sizeof(z));
            *rec_next = z;
        }
    }
    if (r.flags & (V2E_FLAG_EVENTS_DROPPED | V2E_FLAG_ITERS_CLAMPED)) return;
    const unsigned long long n = r.n_events < row0 + max_rows ? r.n_events : row0 + max_rows;
    for (unsigned long long i = row0 + (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256)
        out_rows[i] = ev[i];
}
