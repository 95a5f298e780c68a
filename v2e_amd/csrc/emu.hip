// emu.hip -- DVS pixel model (EventEmulator.generate_events) for gfx950 / MI355X.
//
// What is computed, and where it comes from in the reference (SensorsINI/v2e):
//   k_init   first-frame state           v2ecore/emulator.py:681-717, _init :439-511
//   k_count  lin-log photoreceptor, intensity-dependent IIR low-pass, leak, ON/OFF
//            event counts, shot-noise decisions, global max
//                                        emulator.py:656-775, emulator_utils.py:18-173,297-351
//   k_shot   shot-noise decisions as a separate pass (tape mode draw order)
//   k_rank   refractory filter + per-wave (iteration,polarity) histograms
//                                        emulator.py:810-850
//   k_scan   exclusive scan of the histograms over waves (one workgroup per key)
//   k_emit   dense (t,x,y,p) list in reference order, shuffle, base/ts_mem update
//                                        emulator.py:861-870, 906-942, 1024-1059
//
// Layout: one thread per pixel, row-major, so a wave64 touches 64 consecutive x
// (256/512-byte fully coalesced requests per plane).  Per-pixel state is SoA, one
// plane per field, [n_clips][npx_pad].  Compaction is deterministic: a wave ranks its
// events with __ballot/__popcll, k_scan turns per-wave counts into row offsets, so the
// output order is exactly the reference's nonzero() order -- no atomic cursors.
//
// Numerics: every floating-point step reproduces the reference's dtype and operation
// order; this file must be compiled with -ffp-contract=off.
//
// One translation unit, cut by concern: emu_kernels.h (the kernels above), emu_chain.h (the device-resident run's kernels),
// emu_handle.h (v2e_emu), emu_chain_host.h (the chain's launch schedule and the queue probe); here the C API, v2e_emu_run's
// modes and the dev tools.
#include "common.h"
#include "../../include/v2e_detmath.h"
#include <hip/hip_ext.h> // hipExtLaunchKernel: a kernel launch with a stop event (emu_chain_host.h)

#include <cstdarg>
#include <cstdlib>
#include <vector>

#include "emu_kernels.h" // (opens the anonymous namespace)

#include "emu_chain.h"
// k_cpull<false>: pixels' worth of a frame's rows per workgroup (wpf = npx / this; 346x260: 5 workgroups per frame).  Round 8
// (pixels per workgroup, rows per thread): (2048, 2) / (4096, 2) / (8192, 4) / (16384, 8) measured about 0.566 / 0.558 / 0.556 /
// 0.548 ms per headline step, the parent 0.575 (profiles/r08_emulator_experiments.txt).
#ifndef V2E_PULL_PX_PER_WG
#define V2E_PULL_PX_PER_WG 16384
#endif

} // namespace

// Zero-fill as a KERNEL node.  hipMemsetAsync captured into a hipGraph turned out unreliable for small buffers on
// this runtime (ROCm 7.0 / HIP 7.0.5): from the third launch of the same graph exec a 16..160-byte memset node wrote
// the high half of an address instead of zeros (frame-record flags, the emission offsets, the rendezvous counters).
namespace {
__global__ void k_zero_words(uint32_t *p, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}
// up to four ranges zeroed by ONE launch (the start of a run: four dependent 4-us launches were 17 us of every 300-frame step)
struct ZeroRanges { uint32_t *p[4]; unsigned long long n[4]; };
__global__ __launch_bounds__(256) void k_zero_ranges(ZeroRanges z)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long base = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (i >= base && i < base + z.n[r]) z.p[r][i - base] = 0u;
        base += z.n[r];
    }
}
} // namespace
static inline hipError_t zero_async(void *p, size_t bytes, hipStream_t s)
{
    const size_t n = (bytes + 3) / 4; // all callers pass multiples of 4
    if (n == 0) return hipSuccess;
    k_zero_words<<<(unsigned)((n + 255) / 256), 256, 0, s>>>((uint32_t *)p, n);
    return hipGetLastError();
}

#include "emu_handle.h"

static int alloc_iter_scratch(v2e_emu *h, int max_iters)
{
    if (h->hist) { V2E_HIP(hipFree(h->hist)); h->hist = nullptr; }
    if (h->tot) { V2E_HIP(hipFree(h->tot)); h->tot = nullptr; }
    h->max_iters = max_iters;
    h->nkeys_cap = 2 * max_iters + 2;
    V2E_HIP(hipMalloc(&h->hist, sizeof(uint32_t) * (size_t)h->n_clips * h->nkeys_cap * h->nwaves));
    V2E_HIP(hipMalloc(&h->tot, sizeof(uint32_t) * (size_t)h->n_clips * h->nkeys_cap));
    h->drop_graphs();
    return 0;
}

static V2E_INLINE int stage_ctl(v2e_emu *h, const v2e_emu_params *p, uint32_t frame_idx, const double *t_prev, const double *t_frame, hipStream_t s)
{
    FrameCtl *hc = h->ctl_host + (size_t)(frame_idx % RING) * h->n_clips;
    for (int c = 0; c < h->n_clips; ++c) hc[c] = make_ctl(t_prev[c], t_frame[c], p->cutoff_hz, p->shot_noise_rate_hz, p->refractory_period_s);
    V2E_HIP(hipMemcpyAsync(ctl_slot(h, frame_idx), hc, sizeof(FrameCtl) * h->n_clips, hipMemcpyHostToDevice, s));
    return 0;
}

// ---- one launcher per kernel of a frame: the step-wise API, v2e_emu_frame and the per-frame run loop launch them alike
// (k_init and k_shot have one caller each; their launchers stand here so that the kernel templates are instantiated in the order
// k_init, k_count, k_cs_lp, k_shot, k_emit, which is the order of the functions in the code object)
#define DISPATCH_FT(dtype, ...)                                          \
    switch (dtype) {                                                     \
    case V2E_DT_U8: { typedef uint8_t FT; __VA_ARGS__; } break;          \
    case V2E_DT_F32: { typedef float FT; __VA_ARGS__; } break;           \
    case V2E_DT_F64: { typedef double FT; __VA_ARGS__; } break;          \
    default: v2e_set_error("bad frame dtype %d", dtype); return V2E_EINVAL; \
    }

// a thread per pixel (k_init, k_count, k_cs_lp, k_shot) / a wave per 64 pixels (k_rank, k_emit)
static V2E_INLINE dim3 pixel_grid(const v2e_emu *h) { return dim3(v2e_cdiv(h->npx, BLOCK), h->n_clips); }
static V2E_INLINE dim3 wave_grid(const v2e_emu *h) { return dim3(v2e_cdiv((int64_t)h->nwaves * WAVE, BLOCK), h->n_clips); }

static V2E_INLINE int launch_init(v2e_emu *h, const KArgs &a, int f64_state, const void *frame, int dtype, double t_frame, const float *thres_pos,
                       const float *thres_neg, const float *noise_rate, hipStream_t s)
{
    DISPATCH_FT(dtype, {
        if (f64_state) k_init<double, FT><<<pixel_grid(h), BLOCK, 0, s>>>(a, (const FT *)frame, t_frame, thres_pos, thres_neg, noise_rate);
        else k_init<float, FT><<<pixel_grid(h), BLOCK, 0, s>>>(a, (const FT *)frame, t_frame, thres_pos, thres_neg, noise_rate);
    });
    return 0;
}

static V2E_INLINE int launch_count(v2e_emu *h, const KArgs &a, int f64_state, const void *frame, int dtype, const FrameCtl *ctl,
                        const uint32_t *fidx_base, uint32_t fidx_off, const float *leak, const float *shot,
                        v2e_frame_rec *rec, hipStream_t s, const FrameCtl *ctl_host = nullptr, FrameCtl *ctl_copy = nullptr,
                        double t_prev_v = 0.0, double t_frame_v = 0.0)
{
    DISPATCH_FT(dtype, {
        if (f64_state) k_count<double, FT><<<pixel_grid(h), BLOCK, 0, s>>>(a, (const FT *)frame, ctl, fidx_base, fidx_off, leak, shot, rec, ctl_host, ctl_copy, t_prev_v, t_frame_v);
        else k_count<float, FT><<<pixel_grid(h), BLOCK, 0, s>>>(a, (const FT *)frame, ctl, fidx_base, fidx_off, leak, shot, rec, ctl_host, ctl_copy, t_prev_v, t_frame_v);
    });
    return 0;
}

static V2E_INLINE int launch_cs_lp(v2e_emu *h, const KArgs &a, int f64_state, const void *frame, int dtype, const FrameCtl *ctl, void *lp_out, hipStream_t s)
{
    DISPATCH_FT(dtype, {
        if (f64_state) k_cs_lp<double, FT><<<pixel_grid(h), BLOCK, 0, s>>>(a, (const FT *)frame, ctl, (double *)lp_out);
        else k_cs_lp<float, FT><<<pixel_grid(h), BLOCK, 0, s>>>(a, (const FT *)frame, ctl, (float *)lp_out);
    });
    return 0;
}

static V2E_INLINE int launch_shot(v2e_emu *h, const KArgs &a, const void *frame, int dtype, const FrameCtl *ctl, const float *shot_rand, hipStream_t s)
{
    DISPATCH_FT(dtype, { k_shot<FT><<<pixel_grid(h), BLOCK, 0, s>>>(a, (const FT *)frame, ctl, shot_rand); });
    return 0;
}
#undef DISPATCH_FT

// k_rank, then k_scan (between them `mark`, a profiled run's event)
static V2E_INLINE int launch_rank_scan(v2e_emu *h, const KArgs &a, const FrameCtl *ctl, v2e_frame_rec *rec, const float *ts_table, int n_ts,
                            hipStream_t s, hipEvent_t mark = nullptr)
{
    k_rank<<<wave_grid(h), BLOCK, 0, s>>>(a, ctl, rec, ts_table, n_ts);
    if (mark) V2E_HIP(hipEventRecord(mark, s));
    k_scan<<<dim3(SCAN_BLOCKS, h->n_clips), BLOCK, 0, s>>>(a, rec);
    return 0;
}

static V2E_INLINE void launch_emit(v2e_emu *h, const KArgs &a, int f64_state, const FrameCtl *ctl, v2e_frame_rec *rec, const v2e_frame_rec *rec_prev,
                        const unsigned long long *d_off, const uint32_t *fidx_base, uint32_t fidx_off, const float *ts_table, int n_ts,
                        float *events, uint64_t cap, hipStream_t s)
{
    if (f64_state) k_emit<double><<<wave_grid(h), BLOCK, 0, s>>>(a, ctl, rec, rec_prev, d_off, fidx_base, fidx_off, ts_table, n_ts, (float4 *)events, cap);
    else k_emit<float><<<wave_grid(h), BLOCK, 0, s>>>(a, ctl, rec, rec_prev, d_off, fidx_base, fidx_off, ts_table, n_ts, (float4 *)events, cap);
}

// What a probed run needs beside the caller's buffer: the model-state planes (the caller's, else the library's own) and zeroed
// counters for the row pass.  Blocking only when something has to be (re)allocated.
static int probe_reserve(v2e_emu *h, int n_frames)
{
    if (!h->dbg_diff && !h->probe_planes) V2E_HIP(hipMalloc((void **)&h->probe_planes, sizeof(double) * 3 * (size_t)h->npx_pad));
    const size_t need = (size_t)n_frames * h->probe_run.n * 2 + 1;
    if (need > h->probe_cnt_cap) {
        V2E_HIP(hipDeviceSynchronize()); // (a run before may still count into the old one)
        h->drop_graphs();
        if (h->probe_cnt) V2E_HIP(hipFree(h->probe_cnt));
        h->probe_cnt = nullptr; h->probe_cnt_cap = 0;
        V2E_HIP(hipMalloc((void **)&h->probe_cnt, sizeof(unsigned int) * need));
        h->probe_cnt_cap = need;
    }
    return 0;
}

extern "C" {

const char *v2e_last_error(void) { return g_err; }
int v2e_version(void) { return 100; }

int64_t v2e_emu_npx_pad(int H, int W)
{
    int64_t npx = (int64_t)H * W;
    return (npx + 255) / 256 * 256;
}

int v2e_emu_create(int H, int W, int n_clips, int max_iters, int device, v2e_emu **out)
{
    V2E_REQUIRE(out && H > 0 && W > 0 && n_clips > 0 && max_iters > 0, "bad create args");
    V2E_REQUIRE((int64_t)H * W < (1ll << 31) - 256, "sensor too large");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        v2e_set_error("no HIP device visible");
        return V2E_ENODEV;
    }
    V2E_REQUIRE(device >= 0 && device < ndev, "bad device index");
    V2E_HIP(hipSetDevice(device));
    v2e_emu *h = new v2e_emu();
    h->H = H; h->W = W; h->n_clips = n_clips; h->device = device;
    h->npx = H * W;
    h->npx_pad = v2e_emu_npx_pad(H, W);
    h->nwaves = (h->npx + WAVE - 1) / WAVE;
    h->ngroups = (h->npx + BLOCK - 1) / BLOCK;
    for (int &v : h->occ_cache) v = -1;
    V2E_HIP(hipMalloc(&h->cnt, sizeof(uint32_t) * (size_t)n_clips * h->npx_pad));
    V2E_HIP(hipMalloc(&h->lut_L, sizeof(float) * 256));
    V2E_HIP(hipMalloc(&h->lut_I, sizeof(double) * 256));
    k_lut<<<1, 256>>>(h->lut_L, h->lut_I);
    V2E_HIP(hipDeviceSynchronize());
    {
        int ncu = 0;
        V2E_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
        h->n_cu = ncu;
    }
    V2E_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    int rc = alloc_iter_scratch(h, max_iters);
    if (rc) return rc;
    V2E_HIP(hipMalloc(&h->rec_ring, sizeof(v2e_frame_rec) * RING * n_clips));
    V2E_HIP(hipMemset(h->rec_ring, 0, sizeof(v2e_frame_rec) * RING * n_clips));
    V2E_HIP(hipMalloc(&h->ctl_ring, sizeof(FrameCtl) * RING * n_clips));
    V2E_HIP(hipHostMalloc(&h->ctl_host, sizeof(FrameCtl) * RING * n_clips));
    V2E_HIP(hipMalloc(&h->off_dev, sizeof(unsigned long long) * n_clips));
    V2E_HIP(hipMalloc(&h->off_zero, sizeof(unsigned long long) * n_clips));
    V2E_HIP(hipMemset(h->off_zero, 0, sizeof(unsigned long long) * n_clips));
    V2E_HIP(hipHostMalloc(&h->off_host, sizeof(unsigned long long) * n_clips));
    V2E_HIP(hipHostMalloc(&h->run_fidx_host, 2 * sizeof(uint32_t)));
    V2E_HIP(hipHostMalloc(&h->run_frames_host, 2 * sizeof(void *)));
    V2E_HIP(hipHostMalloc(&h->stamp_slot_host, 2 * sizeof(void *)));
    h->stamp_slot_host[0] = h->stamp_slot_host[1] = nullptr;
    for (RunScratch &r : h->sets) { // the run's device variables, in both scratch sets
        V2E_HIP(hipMalloc(&r.run_fidx, sizeof(uint32_t)));
        V2E_HIP(hipMalloc(&r.run_frames, sizeof(void *)));
        V2E_HIP(hipMalloc(&r.stamp_slot, sizeof(void *)));
        V2E_HIP(hipMemset(r.stamp_slot, 0, sizeof(void *)));
    }
    V2E_HIP(hipDeviceSynchronize()); // the fills above are ordered on the default stream only; the caller's stream may be any
    *out = h;
    return 0;
}

int v2e_emu_destroy(v2e_emu *h)
{
    if (!h) return 0;
    hipSetDevice(h->device);
    h->sync_runs();
    hipDeviceSynchronize();
    h->drop_graphs();
    // per-frame scratch, look-up tables and rings
    hipFree(h->cnt); hipFree(h->hist); hipFree(h->tot); hipFree(h->lut_L); hipFree(h->lut_I); hipFree(h->rec_ring); hipFree(h->ctl_ring);
    if (h->ctl_host) hipHostFree(h->ctl_host);
    hipFree(h->off_dev); hipFree(h->off_zero);
    if (h->off_host) hipHostFree(h->off_host);
    // v2e_emu_frame staging
    h->fr_stage.release(); h->fr_rec_host.release(); h->fr_ev_host.release();
    hipFree(h->fr_dev); if (h->fr_par) hipHostFree(h->fr_par);
    // model extensions
    hipFree(h->csr_slots); hipFree(h->probe_planes); hipFree(h->probe_cnt);
    // run staging
    for (int q = 0; q < 2; ++q) { if (h->run_ctl_host2[q]) hipHostFree(h->run_ctl_host2[q]); if (h->ev_stage[q]) hipEventDestroy(h->ev_stage[q]); }
    if (h->run_fidx_host) hipHostFree(h->run_fidx_host);
    if (h->run_frames_host) hipHostFree(h->run_frames_host);
    for (RunScratch &r : h->sets) r.free_all();
    // chain configuration
    hipFree(h->ch_ck); hipFree(h->ch_base2); hipFree(h->ch_lp2); hipFree(h->ch_ts2);
    // streams and events
    if (h->side) hipStreamDestroy(h->side);
    if (h->side2) hipStreamDestroy(h->side2);
    if (h->ahead) hipStreamDestroy(h->ahead);
    if (h->tabs) hipStreamDestroy(h->tabs);
    for (hipStream_t q : h->spare_streams) hipStreamDestroy(q);
    for (auto *evs : {&h->ev_fork, &h->ev_join, &h->ev_ahead, &h->ev_chain, &h->ev_tab})
        for (hipEvent_t e : *evs) hipEventDestroy(e);
    // pipelined-run bookkeeping
    for (int q = 0; q < 2; ++q) {
        if (h->ev_main_done2[q]) hipEventDestroy(h->ev_main_done2[q]);
        if (h->ev_tail_done2[q]) hipEventDestroy(h->ev_tail_done2[q]);
        if (h->recs_host[q]) hipHostFree(h->recs_host[q]);
    }
    if (h->ev_user) hipEventDestroy(h->ev_user);
    // profiling and dev tools
    hipFree(h->stamps);
    if (h->stamp_slot_host) hipHostFree(h->stamp_slot_host);
    delete h;
    return 0;
}

int v2e_emu_bind_state(v2e_emu *h, void *lp, void *base, float *ts_mem, float *pos_thres, float *neg_thres,
                       float *noise_rate)
{
    V2E_REQUIRE(h && lp && base && pos_thres && neg_thres, "bind_state: null plane");
    h->lp = lp; h->base = base; h->ts_mem = ts_mem;
    h->pos_thres = pos_thres; h->neg_thres = neg_thres; h->noise_rate = noise_rate;
    h->drop_graphs();
    return 0;
}

int v2e_emu_init_state(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype, double t_frame,
                       const float *thres_pos, const float *thres_neg, const float *noise_rate, void *stream)
{
    int rc = enter(h, p, stream);
    if (rc) return rc;
    V2E_REQUIRE(frame, "null frame");
    if (p->rng_mode == V2E_RNG_TAPE) {
        V2E_REQUIRE(p->scalar_thres || (thres_pos && thres_neg), "tape mode needs threshold draws");
        V2E_REQUIRE(!(p->leak_rate_hz > 0) || noise_rate, "tape mode needs noise_rate values");
    }
    V2E_HIP(hipSetDevice(h->device));
    KArgs a = make_kargs(h, p);
    if ((rc = launch_init(h, a, p->f64_state, frame, dtype, t_frame, thres_pos, thres_neg, noise_rate, (hipStream_t)stream))) return rc;
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_emu_set_scidvs(v2e_emu *h, void *highpass, void *previous_photo, float *tau, uint32_t first_frame_idx)
{
    V2E_REQUIRE(h && ((highpass && previous_photo && tau) || (!highpass && !previous_photo && !tau)), "set_scidvs: all three planes or none");
    h->sc_hp = highpass; h->sc_prev = previous_photo; h->sc_tau = tau; h->sc_first_frame = first_frame_idx;
    h->drop_graphs();
    return 0;
}

int v2e_emu_set_csdvs(v2e_emu *h, const void *surround)
{
    V2E_REQUIRE(h, "null");
    h->cs_sur = surround;
    h->drop_graphs();
    return 0;
}

int v2e_emu_lp_preview(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype, const double *t_prev, const double *t_frame,
                       uint32_t frame_idx, void *lp_out, void *stream)
{
    int rc = enter(h, p, stream);
    if (rc) return rc;
    V2E_REQUIRE(frame && t_prev && t_frame && lp_out, "null");
    V2E_REQUIRE(dtype == V2E_DT_U8 || dtype == V2E_DT_F32 || dtype == V2E_DT_F64, "bad frame dtype");
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if ((rc = stage_ctl(h, p, frame_idx, t_prev, t_frame, s))) return rc; // the frame's own slot: v2e_emu_count stages the same values again
    KArgs a = make_kargs(h, p);
    if ((rc = launch_cs_lp(h, a, p->f64_state, frame, dtype, ctl_slot(h, frame_idx), lp_out, s))) return rc;
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_emu_set_csdvs_run(v2e_emu *h, void *h_scratch, void *lp_scratch, const double *alpha_p, const double *alpha_h,
                          const int *num_steps, int n_frames, double max_change_to_stop, int *steps_taken_dev)
{
    V2E_REQUIRE(h, "null handle");
    h->csr_ap.clear(); h->csr_ah.clear(); h->csr_steps.clear();
    if (n_frames <= 0) return 0;
    V2E_REQUIRE(h_scratch && lp_scratch && alpha_p && alpha_h && num_steps && steps_taken_dev, "null");
    int mx = 0;
    for (int f = 0; f < n_frames; ++f) {
        V2E_REQUIRE(num_steps[f] >= 0 && num_steps[f] <= 65536, "CSDVS steps per frame out of range for a device-resident run");
        mx = num_steps[f] > mx ? num_steps[f] : mx;
    }
    V2E_HIP(hipSetDevice(h->device));
    if (mx + 1 > h->csr_slots_cap) {
        V2E_HIP(hipDeviceSynchronize());
        if (h->csr_slots) V2E_HIP(hipFree(h->csr_slots));
        h->csr_slots_cap = mx + 1;
        V2E_HIP(hipMalloc((void **)&h->csr_slots, sizeof(unsigned long long) * (size_t)h->csr_slots_cap));
    }
    h->csr_scratch = h_scratch; h->csr_lp = lp_scratch; h->csr_thr = max_change_to_stop; h->csr_steps_dev = steps_taken_dev;
    h->csr_ap.assign(alpha_p, alpha_p + n_frames); h->csr_ah.assign(alpha_h, alpha_h + n_frames);
    h->csr_steps.assign(num_steps, num_steps + n_frames);
    return 0;
}

int v2e_emu_set_model_state_planes(v2e_emu *h, double *log_new_frame, double *c_minus_s_frame, double *diff_frame)
{
    V2E_REQUIRE(h, "null handle");
    V2E_REQUIRE((log_new_frame && c_minus_s_frame && diff_frame) || (!log_new_frame && !c_minus_s_frame && !diff_frame),
                "model-state planes: all three or none");
    h->dbg_lognew = log_new_frame; h->dbg_cms = c_minus_s_frame; h->dbg_diff = diff_frame;
    return 0;
}

int v2e_emu_set_probes(v2e_emu *h, const int32_t *pixel_index, int n, double *out_dev)
{
    V2E_REQUIRE(h, "null handle");
    h->probe_next.n = 0; h->probe_next_out = nullptr;
    if (n == 0) return 0;
    V2E_REQUIRE(n > 0 && n <= V2E_PROBE_MAX, "set_probes: between 1 and V2E_PROBE_MAX (64) pixels");
    V2E_REQUIRE(pixel_index && out_dev, "set_probes: null pixel list or output buffer");
    V2E_REQUIRE(h->n_clips == 1, "set_probes: handles of one clip only");
    for (int j = 0; j < n; ++j) V2E_REQUIRE(pixel_index[j] >= 0 && pixel_index[j] < h->npx, "set_probes: pixel index outside [0, H * W)");
    for (int j = 0; j < V2E_PROBE_MAX; ++j) h->probe_next.pix[j] = j < n ? pixel_index[j] : 0; // (all of it is part of a graph's key)
    h->probe_next.n = n; h->probe_next_out = out_dev;
    return 0;
}

int v2e_emu_set_pnoise(v2e_emu *h, void *pn_arr, const float *randn_tape)
{
    V2E_REQUIRE(h, "null");
    h->pn_arr = pn_arr;
    h->pn_tape = randn_tape;
    return 0;
}

int v2e_emu_count(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype, const double *t_prev,
                  const double *t_frame, uint32_t frame_idx, const float *leak_randn, const float *shot_rand,
                  void *stream)
{
    int rc = enter(h, p, stream);
    if (rc) return rc;
    V2E_REQUIRE(frame && t_prev && t_frame, "null frame/time");
    if (p->rng_mode == V2E_RNG_TAPE) V2E_REQUIRE(!(p->leak_rate_hz > 0) || leak_randn, "tape mode needs leak_randn");
    if (p->photoreceptor_noise) {
        V2E_REQUIRE(h->pn_arr && p->f64_state && p->cutoff_hz > 0, "photoreceptor noise needs its plane (v2e_emu_set_pnoise) and a cutoff");
        V2E_REQUIRE(!(p->shot_noise_rate_hz > 0), "photoreceptor noise replaces shot events: pass shot_noise_rate_hz = 0");
        V2E_REQUIRE(p->rng_mode != V2E_RNG_TAPE || h->pn_tape, "tape mode needs the photoreceptor-noise draws");
    }
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if ((rc = stage_ctl(h, p, frame_idx, t_prev, t_frame, s))) return rc;
    v2e_frame_rec *rec = rec_slot(h, frame_idx);
    V2E_HIP(zero_async(rec, sizeof(v2e_frame_rec) * h->n_clips, s));
    KArgs a = make_kargs(h, p);
    if ((rc = launch_count(h, a, p->f64_state, frame, dtype, ctl_slot(h, frame_idx), nullptr, frame_idx, leak_randn, shot_rand, rec, s))) return rc;
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_emu_shot(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype, uint32_t frame_idx,
                 const float *shot_rand, void *stream)
{
    int rc = enter(h, p, stream);
    if (rc) return rc;
    V2E_REQUIRE(frame && shot_rand, "null frame/shot_rand");
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    KArgs a = make_kargs(h, p);
    if ((rc = launch_shot(h, a, frame, dtype, ctl_slot(h, frame_idx), shot_rand, s))) return rc;
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_emu_read_rec(v2e_emu *h, uint32_t frame_idx, v2e_frame_rec *recs_host, void *stream)
{
    int rc = join_pending(h, stream);
    if (rc) return rc;
    V2E_REQUIRE(h && recs_host, "null");
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    V2E_HIP(hipMemcpyAsync(recs_host, rec_slot(h, frame_idx), sizeof(v2e_frame_rec) * h->n_clips, hipMemcpyDeviceToHost, s));
    V2E_HIP(hipStreamSynchronize(s));
    return 0;
}

int v2e_emu_reserve_iters(v2e_emu *h, int max_events, void *stream)
{
    V2E_REQUIRE(h, "null");
    if (max_events <= h->max_iters) return 0;
    V2E_HIP(hipSetDevice(h->device));
    V2E_HIP(hipStreamSynchronize((hipStream_t)stream));
    int want = h->max_iters;
    while (want < max_events) want *= 2;
    return alloc_iter_scratch(h, want);
}

int v2e_emu_rank(v2e_emu *h, const v2e_emu_params *p, uint32_t frame_idx, const float *ts_table, int n_ts,
                 void *stream)
{
    int rc = enter(h, p, stream);
    if (rc) return rc;
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    KArgs a = make_kargs(h, p);
    if ((rc = launch_rank_scan(h, a, ctl_slot(h, frame_idx), rec_slot(h, frame_idx), ts_table, n_ts, s))) return rc;
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_emu_emit(v2e_emu *h, const v2e_emu_params *p, uint32_t frame_idx, const float *ts_table, int n_ts,
                 float *events, uint64_t cap, const uint64_t *ev_offset0, void *stream)
{
    int rc = enter(h, p, stream);
    if (rc) return rc;
    V2E_REQUIRE(events || cap == 0, "null events");
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    KArgs a = make_kargs(h, p);
    unsigned long long *d_off = nullptr;
    if (ev_offset0) { // host array -> pinned staging -> device (frame-at-a-time API syncs every frame)
        for (int c = 0; c < h->n_clips; ++c) h->off_host[c] = ev_offset0[c];
        d_off = h->off_dev;
        V2E_HIP(hipMemcpyAsync(d_off, h->off_host, sizeof(unsigned long long) * h->n_clips, hipMemcpyHostToDevice, s));
    }
    launch_emit(h, a, p->f64_state, ctl_slot(h, frame_idx), rec_slot(h, frame_idx), rec_slot(h, frame_idx + RING - 1), d_off, nullptr, frame_idx,
                ts_table, n_ts, events, cap, s);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_emu_read_iter_counts(v2e_emu *h, uint32_t frame_idx, int n_iters, uint32_t *counts_host, void *stream)
{
    (void)frame_idx;
    V2E_REQUIRE(h && counts_host && n_iters >= 0 && n_iters <= h->max_iters, "bad read_iter_counts args");
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const int nk = 2 * (n_iters + 1);
    for (int c = 0; c < h->n_clips; ++c)
        V2E_HIP(hipMemcpyAsync(counts_host + (size_t)c * nk, h->tot + (size_t)c * h->nkeys_cap, sizeof(uint32_t) * nk,
                               hipMemcpyDeviceToHost, s));
    V2E_HIP(hipStreamSynchronize(s));
    return 0;
}

int v2e_emu_permute(v2e_emu *h, const float *events_in, float *events_out, const int32_t *idx, uint64_t row0,
                    uint64_t n, void *stream)
{
    V2E_REQUIRE(h && events_in && events_out && idx, "null");
    if (n == 0) return 0;
    V2E_HIP(hipSetDevice(h->device));
    k_permute<<<v2e_cdiv((int64_t)n, BLOCK), BLOCK, 0, (hipStream_t)stream>>>((const float4 *)events_in, (float4 *)events_out,
                                                                              idx, row0, n);
    V2E_HIP(hipGetLastError());
    return 0;
}

// One frame of the frame-at-a-time API in ONE call (Philox mode, one clip): what a v2e.py caller of generate_events pays
// per frame used to be five C calls with three stream synchronisations between them.  Here: frame -> pinned staging ->
// device, count / rank / scan enqueued back to back, ONE read-back of the frame record and the per-key totals (which
// gives M and the event count), emit, ONE read-back of exactly that many rows into pinned memory.
// Returns 0, or 1 when the frame needs more iteration scratch than the handle has (M > max_iters; the caller grows it
// with v2e_emu_reserve_iters and finishes the frame with v2e_emu_rank / v2e_emu_emit: the count is done and stays valid),
// or 2 when the rows do not fit `cap` (same: nothing was emitted).
int v2e_emu_frame(v2e_emu *h, const v2e_emu_params *p, const void *frame, int frame_on_host, int dtype, double t_prev, double t_frame,
                  uint32_t frame_idx, float *events_dev, uint64_t cap, uint32_t *out8, const float **events_host, void *stream)
{
    int rc = enter(h, p, stream);
    if (rc) return rc;
    V2E_REQUIRE(frame && out8 && events_host && events_dev, "null");
    V2E_REQUIRE(h->n_clips == 1 && p->rng_mode == V2E_RNG_PHILOX && !p->photoreceptor_noise, "v2e_emu_frame: one clip, Philox mode, no photoreceptor noise");
    V2E_REQUIRE(dtype == V2E_DT_U8 || dtype == V2E_DT_F32 || dtype == V2E_DT_F64, "bad frame dtype");
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t fbytes = dtype_size(dtype) * (size_t)h->npx;
    // (no copy engine on the way in or out: see FrameScratch in emu_kernels.h)
    if (frame_on_host && fbytes > h->fr_stage.cap) {
        V2E_HIP(hipStreamSynchronize(s));
        if ((rc = h->fr_stage.grow(fbytes))) return rc;
    }
    if (!h->fr_dev) {
        V2E_HIP(hipMalloc((void **)&h->fr_dev, sizeof(FrameScratch)));
        V2E_HIP(hipMemset(h->fr_dev, 0, sizeof(FrameScratch))); // both records zero: the first frame counts into a clean one
        V2E_HIP(hipDeviceSynchronize());                        // (ordered on the default stream only; once per handle)
        V2E_HIP(hipHostMalloc((void **)&h->fr_par, sizeof(FrameCtl), hipHostMallocMapped));
        V2E_HIP(hipHostGetDevicePointer((void **)&h->fr_par_dev, h->fr_par, 0));
        h->fr_flip = 0;
    }
    if ((rc = h->fr_rec_host.grow(sizeof(v2e_frame_rec) + sizeof(uint32_t) * h->nkeys_cap))) return rc; // (nkeys_cap only ever grows)
    const void *frame_dev = frame;
    if (frame_on_host) {
        memcpy(h->fr_stage.host, frame, fbytes); // (the previous frame's kernels have completed: every call ends synchronised)
        frame_dev = h->fr_stage.dev;
    }
    // destination of the rows: the caller's pinned buffer for this frame (v2e_emu_frame_host_rows; one frame only), else the
    // handle's own
    float *user_rows = h->fr_user_rows, *user_rows_dev = h->fr_user_rows_dev;
    const uint64_t user_cap = h->fr_user_cap;
    h->fr_user_rows = h->fr_user_rows_dev = nullptr; h->fr_user_cap = 0;
    uint64_t est = std::min<uint64_t>(std::max<uint64_t>(h->fr_est, 1024), cap);
    if (user_rows) est = std::min<uint64_t>(est, user_cap);
    // the handle's own rows hold `rows` (twice that, 1 MB at the least), the first `keep` of what they held kept
    auto own_rows = [&](uint64_t rows, uint64_t keep) -> int {
        if (rows <= h->fr_ev_rows()) return 0;
        return h->fr_ev_host.grow(sizeof(float) * 4 * std::max<uint64_t>(2 * rows, 1u << 16), sizeof(float) * 4 * keep);
    };
    if (!user_rows && est > h->fr_ev_rows()) {
        V2E_HIP(hipStreamSynchronize(s));
        if ((rc = own_rows(est, 0))) return rc;
    }
    // Five launches, no copy engine, no host step between them: the frame's times go to k_count by value, its workgroup 0 copies
    // the frame's scalars from pinned host memory to the device for the kernels behind it; the record a frame counts into was
    // zeroed by the frame before (two records alternate); the event writer goes out before the host has seen the totals
    // (k_emit checks them against cap itself), and with it the copy of the rows the frame is expected to have: one
    // synchronisation per frame unless the estimate was short.  (Replaying the launches as a hipGraph was measured: the host
    // spends 10 us instead of 19 us enqueueing, the graph's start latency leaves the frame's wall time where it was.)
    const FrameCtl ctl_host = make_ctl(t_prev, t_frame, p->cutoff_hz, p->shot_noise_rate_hz, p->refractory_period_s);
    *(FrameCtl *)h->fr_par = ctl_host;
    FrameScratch *sc = (FrameScratch *)h->fr_dev;
    v2e_frame_rec *rec = &sc->rec[h->fr_flip], *rec_next = &sc->rec[h->fr_flip ^ 1];
    h->fr_flip ^= 1;
    FrameCtl *ctl = &sc->ctl;
    KArgs a = make_kargs(h, p);
    a.emit_guard = 1;
    v2e_frame_rec *rh = (v2e_frame_rec *)h->fr_rec_host.host;
    if ((rc = launch_count(h, a, p->f64_state, frame_dev, dtype, nullptr, nullptr, frame_idx, nullptr, nullptr, rec, s,
                           (const FrameCtl *)h->fr_par_dev, ctl, t_prev, t_frame))) return rc;
    if ((rc = launch_rank_scan(h, a, ctl, rec, nullptr, 0, s))) return rc;
    launch_emit(h, a, p->f64_state, ctl, rec, nullptr, h->off_zero, nullptr, frame_idx, nullptr, 0, events_dev, cap, s);
    k_frame_rows_to_host<<<256, 256, 0, s>>>((const float4 *)events_dev, rec, (float4 *)(user_rows ? user_rows_dev : (float *)h->fr_ev_host.dev),
                                             (v2e_frame_rec *)h->fr_rec_host.dev, 0ull, est, rec_next);
    V2E_HIP(hipGetLastError());
    V2E_HIP(hipStreamSynchronize(s));
    const int M = rh->max_events;
    memset(out8, 0, sizeof(uint32_t) * 8);
    out8[4] = (uint32_t)M;
    *events_host = nullptr;
    if (M > h->max_iters || (rh->flags & V2E_FLAG_EVENTS_DROPPED)) {
        // not emitted (nothing of the state touched): hand the counted frame to the step-wise entry points, which read
        // the ring's record and scalars
        const int slot = frame_idx % RING;
        V2E_HIP(hipMemcpyAsync(h->rec_ring + slot, rec, sizeof(v2e_frame_rec), hipMemcpyDeviceToDevice, s));
        V2E_HIP(zero_async(&h->rec_ring[slot].flags, sizeof(uint32_t), s));
        V2E_HIP(hipMemcpyAsync(h->ctl_ring + slot, ctl, sizeof(FrameCtl), hipMemcpyDeviceToDevice, s));
        h->ctl_host[slot] = ctl_host;
        if (M > h->max_iters) { V2E_HIP(hipStreamSynchronize(s)); return 1; }
        uint32_t *th = (uint32_t *)(h->fr_rec_host.host + sizeof(v2e_frame_rec));
        V2E_HIP(hipMemcpyAsync(th, h->tot, sizeof(uint32_t) * (2 * M + 2), hipMemcpyDeviceToHost, s));
        V2E_HIP(hipStreamSynchronize(s));
        uint64_t n_on = 0, n_off = 0, n_sig = 0;
        for (int k = 0; k < 2 * M + 2; ++k) {
            ((k & 1) ? n_off : n_on) += th[k];
            if (k < 2 * M) n_sig += th[k];
        }
        out8[0] = (uint32_t)(n_on + n_off); out8[1] = (uint32_t)n_on; out8[2] = (uint32_t)n_off; out8[3] = (uint32_t)n_sig;
        return 2;
    }
    const uint64_t n = rh->n_events;
    out8[0] = (uint32_t)n; out8[1] = rh->n_on; out8[2] = rh->n_off; out8[3] = rh->n_signal;
    h->fr_est = n + n / 4 + 256;
    // The first copy put rows [0, est) into the caller's buffer if there is one, else into the handle's own.  A caller's buffer that
    // cannot hold the frame is given up: all rows into the handle's own.  Otherwise the rest of the rows, if the estimate was short.
    const bool own = !user_rows || n > user_cap;
    const uint64_t first = (user_rows && own) ? 0 : est; // rows [0, first) are where they belong already
    if (n > first) {
        if (own && (rc = own_rows(n, first))) return rc;
        float *dst_dev = own ? (float *)h->fr_ev_host.dev : user_rows_dev;
        k_frame_rows_to_host<<<(unsigned)std::min<uint64_t>(v2e_cdiv((int64_t)(n - first), 256), 4096), 256, 0, s>>>(
            (const float4 *)events_dev, rec, (float4 *)dst_dev, nullptr, first, n - first, nullptr);
        V2E_HIP(hipGetLastError());
        V2E_HIP(hipStreamSynchronize(s));
    }
    if (n > 0) *events_host = own ? (const float *)h->fr_ev_host.host : user_rows;
    return 0;
}

int v2e_emu_frame_host_rows(v2e_emu *h, float *pinned_rows, uint64_t cap_rows)
{
    V2E_REQUIRE(h, "null");
    h->fr_user_rows = h->fr_user_rows_dev = nullptr; h->fr_user_cap = 0;
    if (!pinned_rows || cap_rows == 0) return 0;
    V2E_HIP(hipSetDevice(h->device));
    void *dev = nullptr;
    V2E_HIP(hipHostGetDevicePointer(&dev, pinned_rows, 0)); // fails for memory that is not pinned (hipHostMalloc / hipHostRegister)
    h->fr_user_rows = pinned_rows; h->fr_user_rows_dev = (float *)dev; h->fr_user_cap = cap_rows;
    return 0;
}

} // extern "C"
// Enqueue the whole multi-frame sequence on stream s (no host sync).
static int enqueue_run(v2e_emu *h, const v2e_emu_params *p, const KArgs &a, const void *frames, int dtype, int n_frames,
                       float *events, uint64_t cap, v2e_frame_rec *recs, hipStream_t s, hipEvent_t *evs = nullptr)
{
#define V2E_MARK(i) do { if (evs) V2E_HIP(hipEventRecord(evs[(i)], s)); } while (0)
    const RunScratch &r = h->cur();
    const size_t esz = dtype_size(dtype);
    V2E_HIP(zero_async(recs, sizeof(v2e_frame_rec) * (size_t)n_frames * h->n_clips, s));
    // v2e_emu_set_probes: the taps below carry no marks of their own (a profiled run times them with the kernel they follow)
    const V2EProbeSet &ps = h->probe_run;
    const size_t probe_stride = (size_t)ps.n * V2E_PROBE_FIELDS;
    const size_t probe_words = (size_t)n_frames * ps.n * 2 + 1;
    if (ps.n) V2E_HIP(zero_async(h->probe_cnt, sizeof(unsigned int) * probe_words, s));
    for (int f = 0; f < n_frames; ++f) {
        const void *fr = (const char *)frames + (size_t)f * h->n_clips * h->npx * esz;
        const FrameCtl *ctl = r.run_ctl + (size_t)f * h->n_clips;
        v2e_frame_rec *rec = recs + (size_t)f * h->n_clips;
        const v2e_frame_rec *rec_prev = f > 0 ? rec - h->n_clips : nullptr;
        V2E_MARK(4 * f + 0);
        if (h->cs_sur) { // emulator.py:707-708: the surround is stepped against the coming frame's lp_log_frame, on the stream
            int rcs = launch_cs_lp(h, a, p->f64_state, fr, dtype, ctl, h->csr_lp, s);
            if (rcs) return rcs;
            rcs = v2e_csdvs_enqueue_frame(h->csr_lp, const_cast<void *>(h->cs_sur), h->csr_scratch, h->H, h->W, p->f64_state,
                                              h->csr_ap[f], h->csr_ah[f], h->csr_steps[f], h->csr_thr, h->csr_slots, h->csr_steps_dev + f, s);
            if (rcs) return rcs;
        }
        int rc = launch_count(h, a, p->f64_state, fr, dtype, ctl, r.run_fidx, (uint32_t)f, nullptr, nullptr, rec, s);
        if (rc) return rc;
        if (ps.n && (rc = v2e_probe_tap_count(ps, fr, dtype, a.dbg_lognew, a.dbg_diff, h->probe_out + (size_t)f * probe_stride, s))) return rc;
        V2E_MARK(4 * f + 1);
        if ((rc = launch_rank_scan(h, a, ctl, rec, nullptr, 0, s, evs ? evs[4 * f + 2] : nullptr))) return rc;
        V2E_MARK(4 * f + 3);
        launch_emit(h, a, p->f64_state, ctl, rec, rec_prev, nullptr, r.run_fidx, (uint32_t)f, nullptr, 0, events, cap, s);
        if (ps.n && (rc = v2e_probe_tap_emit(ps, a.lp, a.base, p->f64_state, a.pos_thres, a.neg_thres, a.scalar_thres, p->pos_thres_scalar,
                                             p->neg_thres_scalar, h->probe_out + (size_t)f * probe_stride, s))) return rc;
    }
    V2E_MARK(4 * n_frames);
#undef V2E_MARK
    if (ps.n) { // the signal ON / OFF rows at the probed pixels, frame by frame: one pass over the run's rows
        int rc = v2e_probe_count_rows(ps, events, cap, recs, n_frames, h->W, h->probe_cnt, h->probe_cnt + probe_words - 1, h->probe_out,
                                      h->n_cu, s);
        if (rc) return rc;
    }
    V2E_HIP(hipGetLastError());
    return 0;
}

#include "emu_chain_host.h"

// ---- v2e_emu_run, one function per mode
// Everything a run's kernels read that is sized by its length: the two pinned staging sets (all scratch sets' device buffers go with
// them) and the current set's device buffer.
static int reserve_run(v2e_emu *h, int n_frames, hipStream_t s)
{
    if (n_frames > h->run_cap) {
        h->sync_runs();
        V2E_HIP(hipStreamSynchronize(s));
        for (RunScratch &r : h->sets) { hipFree(r.run_ctl); r.run_ctl = nullptr; }
        for (int q = 0; q < 2; ++q) if (h->run_ctl_host2[q]) V2E_HIP(hipHostFree(h->run_ctl_host2[q]));
        h->run_cap = n_frames;
        for (int q = 0; q < 2; ++q) V2E_HIP(hipHostMalloc(&h->run_ctl_host2[q], sizeof(FrameCtl) * (size_t)h->run_cap * h->n_clips));
        h->drop_graphs();
    }
    RunScratch &r = h->cur();
    if (!r.run_ctl) { V2E_HIP(hipMalloc(&r.run_ctl, sizeof(FrameCtl) * (size_t)h->run_cap * h->n_clips)); h->drop_graphs(); }
    return 0;
}

// The run's frame times, first frame index, frames' address and stamp slot to the current scratch set's device variables, on `s_up`:
// through k_upload_ctl, which reads one of two pinned staging sets (round 5; before: three hipMemcpyAsync -- A/B x 3 on the benchmark
// loop 11.9 -> 12.15 Gev/s: in the rocprofv3 timeline the copy-engine upload started 40-90 us behind the command before it, the kernel
// 10 us).  Each staging set is guarded by the event of the upload that last read it: the host prepares run n + 1 while run n executes.
static int upload_run(v2e_emu *h, const v2e_emu_params *p, int n_frames, const double *t_prev, const double *t_frame,
                      uint32_t frame_idx0, const void *frames, hipStream_t s_up)
{
    const RunScratch &r = h->cur();
    const int sq = h->run_stage ^= 1;
    if (!h->ev_stage[sq]) V2E_HIP(hipEventCreateWithFlags(&h->ev_stage[sq], hipEventDisableTiming));
    else V2E_HIP(hipEventSynchronize(h->ev_stage[sq]));
    static_assert(sizeof(FrameCtl) >= 2 * sizeof(double), "the staging set holds two doubles per frame");
    const size_t nct = (size_t)n_frames * h->n_clips;
    double *const tp_host = (double *)h->run_ctl_host2[sq], *const tf_host = tp_host + nct;
    memcpy(tp_host, t_prev, sizeof(double) * nct);
    memcpy(tf_host, t_frame, sizeof(double) * nct);
    uint32_t *fidx_host = h->run_fidx_host + sq;
    *fidx_host = frame_idx0;
    const void **frames_host = h->run_frames_host + sq; // the chain pipeline reads the frames' address from a device variable:
    *frames_host = frames;                              // runs over different frame buffers replay the same captured graph
    unsigned long long **slot_host = h->stamp_slot_host + sq;
    *slot_host = h->stamps_runs > 0 ? h->stamps + (size_t)(h->stamp_seq++ % (unsigned long long)h->stamps_runs) * 2 * STAMP_LAUNCHES : nullptr;
    k_upload_ctl<<<(unsigned)std::min<size_t>((nct + BLOCK - 1) / BLOCK, 1024), BLOCK, 0, s_up>>>(tp_host, tf_host, r.run_ctl, nct, p->cutoff_hz, p->shot_noise_rate_hz,
                                                                                               p->refractory_period_s, fidx_host, r.run_fidx, frames_host, r.run_frames,
                                                                                               slot_host, r.stamp_slot);
    V2E_HIP(hipGetLastError());
    V2E_HIP(hipEventRecord(h->ev_stage[sq], s_up));
    return 0;
}

// PIPELINED runs (round 6).  The chain of run n + 1 needs the chain of run n and nothing else of it, but a run begins with an upload,
// zero fills and its first records (k_ahead) and ends with the emission of its last frames: measured with the device stamps
// (v2e_emu_launch_stamps), 145-165 us of every 820 us step of the benchmark passed between the last chain launch of one run and the
// first of the next with one graph per run.  Here the caller's stream carries the chain's launches only, run after run in one hardware
// queue (33 us between two runs' chains); the handle's k_ahead stream carries the run's head and runs ahead of the chain, beside the
// run before; the emission streams follow the chain batch by batch and finish beside the run after.  The run has scratch set `par`.
static int run_pipelined(v2e_emu *h, const v2e_emu_params *p, const KArgs &a, const void *frames, int dtype, int n_frames,
                         const double *t_prev, const double *t_frame, uint32_t frame_idx0, float *events, uint64_t cap,
                         v2e_frame_rec *recs_dev, bool frames_resident, hipStream_t s)
{
    if (!h->probed || h->probed_for != s) {
        const int rc = assign_pipelined_streams(h, s);
        if (rc) return rc;
    }
    const int par = h->scratch_par;
    for (int q = 0; q < 2; ++q) {
        if (!h->ev_main_done2[q]) V2E_HIP(hipEventCreateWithFlags(&h->ev_main_done2[q], hipEventDisableTiming));
        if (!h->ev_tail_done2[q]) V2E_HIP(hipEventCreateWithFlags(&h->ev_tail_done2[q], hipEventDisableTiming));
    }
    hipStream_t s_up = h->ahead; // the run's head
    // the k_ahead stream reads the frames: it is ordered behind what the caller's stream holds now -- unless the caller vouches that
    // the frames are resident; otherwise it would wait for the chain of the run before, which is on that stream, and the run's head
    // would not overlap it
    if (!frames_resident) {
        if (!h->ev_user) V2E_HIP(hipEventCreateWithFlags(&h->ev_user, hipEventDisableTiming));
        V2E_HIP(hipEventRecord(h->ev_user, s));
        V2E_HIP(hipStreamWaitEvent(s_up, h->ev_user, 0));
    }
    // this scratch set's last user (two runs ago): its chain and its emission have finished
    if (h->piece_pending[par]) {
        V2E_HIP(hipStreamWaitEvent(s_up, h->ev_main_done2[par], 0));
        V2E_HIP(hipStreamWaitEvent(s_up, h->ev_tail_done2[par], 0));
    }
    if (h->piece_pending[par ^ 1] && (events == h->last_events || (const void *)recs_dev == h->last_recs))
        V2E_HIP(hipStreamWaitEvent(s_up, h->ev_tail_done2[par ^ 1], 0));
    int rc = upload_run(h, p, n_frames, t_prev, t_frame, frame_idx0, frames, s_up);
    if (rc) return rc;
    // ev_main_done2[par], the run's chain (the pixel state): the stop event of its last chain launch, not a record behind it
    rc = enqueue_run_chain(h, p, a, dtype, n_frames, events, cap, recs_dev, s, ChainMode::pipelined, nullptr, h->ev_main_done2[par]);
    if (rc) return rc;
    hipStream_t rows_stream = h->side2;
    // the run's records to pinned host memory behind its last rows (v2e_emu_run_recs): what result() reads -- no copy of the
    // caller's own, no stream of the caller's to synchronise
    const size_t rbytes = sizeof(v2e_frame_rec) * (size_t)n_frames * h->n_clips;
    if (rbytes > h->recs_host_cap[par]) {
        if (h->recs_host[par]) V2E_HIP(hipHostFree(h->recs_host[par]));
        h->recs_host[par] = nullptr;
        V2E_HIP(hipHostMalloc(&h->recs_host[par], rbytes));
        h->recs_host_cap[par] = rbytes;
    }
    V2E_HIP(hipMemcpyAsync(h->recs_host[par], recs_dev, rbytes, hipMemcpyDeviceToHost, rows_stream));
    h->recs_host_n[par] = (size_t)n_frames * h->n_clips;
    V2E_HIP(hipEventRecord(h->ev_tail_done2[par], rows_stream)); // its last event rows (and the records' copy)
    h->piece_pending[par] = true;
    h->last_events = events; h->last_recs = recs_dev;
    return 0;
}

// V2E_RUN_PROFILE through k_chain (blocking): chain time from events on `s`, emission batches from events around the event rows
static int run_profiled_chain(v2e_emu *h, const v2e_emu_params *p, const KArgs &a, int dtype, int n_frames, float *events, uint64_t cap,
                              v2e_frame_rec *recs_dev, hipStream_t s)
{
    ChainMarks mk;
    int rc = enqueue_run_chain(h, p, a, dtype, n_frames, events, cap, recs_dev, s, ChainMode::profiled, &mk);
    if (rc == 0) {
        std::vector<hipEvent_t> &em = mk.chain, &es = mk.rows;
        V2E_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < 4; ++k) h->prof_ms[k] = 0.0;
        float ms = 0.f;
        V2E_HIP(hipEventElapsedTime(&ms, em.front(), em.back()));
        h->prof_ms[0] = ms; // first launch's start to last launch's end: the chain's launch-to-launch period x launches
        h->prof_chain_us.clear();
        for (size_t i = 0; i + 1 < em.size(); i += 2) { // the kernels alone
            V2E_HIP(hipEventElapsedTime(&ms, em[i], em[i + 1]));
            h->prof_ms[1] += ms;
            h->prof_chain_us.push_back(ms * 1e3f);
        }
        h->prof_step_launches = (int)(em.size() / 2);
        for (size_t i = 0; i + 1 < es.size(); i += 2) {
            V2E_HIP(hipEventElapsedTime(&ms, es[i], es[i + 1]));
            h->prof_ms[3] += ms;
        }
        h->prof_launches = n_frames;
        h->prof_emit_batches = (int)(es.size() / 2);
    }
    for (hipEvent_t e : mk.chain) hipEventDestroy(e);
    for (hipEvent_t e : mk.rows) hipEventDestroy(e);
    return rc;
}

// V2E_RUN_PROFILE through the per-frame kernels (blocking): a hipEvent before every launch
static int run_profiled_frames(v2e_emu *h, const v2e_emu_params *p, const KArgs &a, const void *frames, int dtype, int n_frames,
                               float *events, uint64_t cap, v2e_frame_rec *recs_dev, hipStream_t s)
{
    const int ne = 4 * n_frames + 4;
    std::vector<hipEvent_t> evs(ne);
    for (int i = 0; i < ne; ++i) V2E_HIP(hipEventCreate(&evs[i]));
    int rc = enqueue_run(h, p, a, frames, dtype, n_frames, events, cap, recs_dev, s, evs.data());
    if (rc == 0) {
        V2E_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < 4; ++k) h->prof_ms[k] = 0.0;
        for (int i = 0; i < 4 * n_frames; ++i) {
            float ms = 0.f;
            V2E_HIP(hipEventElapsedTime(&ms, evs[i], evs[i + 1]));
            h->prof_ms[i & 3] += ms;
        }
        h->prof_launches = n_frames;
        h->prof_emit_batches = 0;
        h->prof_step_launches = n_frames;
    }
    for (int i = 0; i < ne; ++i) hipEventDestroy(evs[i]);
    return rc;
}

// Everything a captured run bakes in (buffers, sizes, parameters, the current scratch set's pointers): the key of its cached graph
static std::vector<unsigned char> graph_key(const v2e_emu *h, const v2e_emu_params *p, const KArgs &a, const void *frames, int dtype,
                                            int n_frames, float *events, uint64_t cap, v2e_frame_rec *recs_dev, bool chain)
{
    const RunScratch &r = h->cur();
    std::vector<unsigned char> key;
    auto push = [&key](const void *ptr, size_t n) { const unsigned char *b = (const unsigned char *)ptr; key.insert(key.end(), b, b + n); };
    push(&a, sizeof(a)); push(&dtype, sizeof(dtype)); push(&n_frames, sizeof(n_frames));
    if (!chain) push(&frames, sizeof(frames)); // the chain pipeline reads the frames' address from RunScratch::run_frames
    push(&events, sizeof(events)); push(&cap, sizeof(cap)); push(&recs_dev, sizeof(recs_dev));
    int f64 = p->f64_state; push(&f64, sizeof(f64));
    int lg = chain ? 3 : 1; push(&lg, sizeof(lg)); push(&h->dbg, sizeof(h->dbg));
    push(&r.run_ctl, sizeof(r.run_ctl)); push(&r.run_fidx, sizeof(r.run_fidx)); push(&r.run_off, sizeof(r.run_off));
    { const int mk = h->stamps_runs > 0 ? 1 : 0; push(&mk, sizeof(mk)); }
    if (h->cs_sur) { // everything the diffuser's launches bake in
        push(&h->cs_sur, sizeof(h->cs_sur)); push(&h->csr_scratch, sizeof(void *)); push(&h->csr_lp, sizeof(void *));
        push(&h->csr_steps_dev, sizeof(void *)); push(&h->csr_slots, sizeof(void *)); push(&h->csr_thr, sizeof(double));
        push(h->csr_ap.data(), sizeof(double) * h->csr_ap.size()); push(h->csr_ah.data(), sizeof(double) * h->csr_ah.size());
        push(h->csr_steps.data(), sizeof(int) * h->csr_steps.size());
    }
    if (h->probe_run.n) { // the probed pixels travel in the launches; their buffers are baked in
        push(&h->probe_run, sizeof(h->probe_run)); push(&h->probe_out, sizeof(h->probe_out)); push(&h->probe_cnt, sizeof(h->probe_cnt));
    }
    if (chain) {
        push(&h->ch_K, sizeof(h->ch_K)); push(&h->ch_E, sizeof(h->ch_E)); push(&h->ch_fused, sizeof(h->ch_fused)); push(&h->ch_nD, sizeof(h->ch_nD));
        push(&h->ch_max_blocks, sizeof(h->ch_max_blocks));
        push(&r.ch_gM, sizeof(r.ch_gM)); push(&r.ch_tsold, sizeof(r.ch_tsold)); push(&h->ch_ck, sizeof(h->ch_ck)); push(&r.ch_cnt, sizeof(r.ch_cnt));
        push(&r.ch_msk, sizeof(r.ch_msk));
    }
    return key;
}

// V2E_RUN_GRAPH: the run's cached graph (captured on a miss, the least recently used one dropped beyond 24), launched on `s`
static int run_graph(v2e_emu *h, const v2e_emu_params *p, const KArgs &a, const void *frames, int dtype, int n_frames, float *events,
                     uint64_t cap, v2e_frame_rec *recs_dev, bool chain, hipStream_t s)
{
    std::vector<unsigned char> key = graph_key(h, p, a, frames, dtype, n_frames, events, cap, recs_dev, chain);
    hipGraphExec_t exec = nullptr;
    for (auto &cg : h->graphs)
        if (cg.key == key) { exec = cg.exec; cg.used = ++h->graph_clock; memcpy(h->last_queue_ops, cg.ops, sizeof(cg.ops)); break; }
    if (!exec) {
        if (h->graphs.size() >= 24) { // (two scratch sets x the caller's buffer sets)
            size_t lru = 0;
            for (size_t i = 1; i < h->graphs.size(); ++i) if (h->graphs[i].used < h->graphs[lru].used) lru = i;
            hipGraphExecDestroy(h->graphs[lru].exec);
            h->graphs.erase(h->graphs.begin() + lru);
        }
        hipGraph_t g = nullptr;
        hipStream_t cs;
        V2E_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        V2E_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        const int rc = chain ? enqueue_run_chain(h, p, a, dtype, n_frames, events, cap, recs_dev, cs, ChainMode::captured)
                             : enqueue_run(h, p, a, frames, dtype, n_frames, events, cap, recs_dev, cs);
        hipError_t e = hipStreamEndCapture(cs, &g);
        hipStreamDestroy(cs);
        if (rc) { if (g) hipGraphDestroy(g); return rc; }
        V2E_HIP(e);
        V2E_HIP(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
        V2E_HIP(hipGraphDestroy(g));
        h->graphs.push_back({std::move(key), exec, ++h->graph_clock, {h->last_queue_ops[0], h->last_queue_ops[1], h->last_queue_ops[2]}});
    }
    V2E_HIP(hipGraphLaunch(exec, s));
    return 0;
}
extern "C" {

int v2e_emu_run(v2e_emu *h, const v2e_emu_params *p, const void *frames, int dtype, int n_frames, const double *t_prev,
                const double *t_frame, uint32_t frame_idx0, float *events, uint64_t cap, v2e_frame_rec *recs_dev,
                int flags, void *stream)
{
    if (h) { // v2e_emu_set_probes is one shot: this run takes the setting, whatever becomes of it
        h->probe_run = h->probe_next; h->probe_out = h->probe_next_out;
        h->probe_next.n = 0; h->probe_next_out = nullptr;
    }
    int rc = check_params(h, p);
    if (rc) return rc;
    const bool probed = h->probe_run.n > 0;
    V2E_REQUIRE(p->rng_mode == V2E_RNG_PHILOX, "v2e_emu_run is the device-resident Philox path");
    V2E_REQUIRE(frames && t_prev && t_frame && events && recs_dev && n_frames > 0, "bad run args");
    V2E_REQUIRE(dtype == V2E_DT_U8 || dtype == V2E_DT_F32 || dtype == V2E_DT_F64, "bad frame dtype");
    V2E_REQUIRE(!h->cs_sur || ((int)h->csr_steps.size() == n_frames && h->n_clips == 1),
                "a run with a CSDVS surround needs v2e_emu_set_csdvs_run for exactly these frames (one clip)");
    const bool chain_ok = chain_eligible(h, p, dtype);
    V2E_REQUIRE(!(flags & V2E_RUN_REQUIRE_CHAIN) || chain_ok, "k_chain cannot run this configuration (max_iters, photoreceptor noise or float64 log frames)");
    V2E_REQUIRE(!(flags & V2E_RUN_REQUIRE_CHAIN) || !probed, "k_chain records no single-pixel states: a run with probes set (v2e_emu_set_probes) goes through the per-frame kernels");
    const bool chain = chain_ok && !probed && ((flags & V2E_RUN_REQUIRE_CHAIN) || !(flags & V2E_RUN_PER_FRAME_KERNELS));
    const int mode = flags & 3; // 0 plain launches, V2E_RUN_GRAPH, V2E_RUN_PROFILE
    const bool pipelined = (flags & V2E_RUN_PIPELINED) && mode == 0 && chain;
    V2E_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (pipelined) h->scratch_par ^= 1; // (the other scratch set than the run before)
    h->last_ticket = pipelined ? h->scratch_par : -1;
    rc = reserve_run(h, n_frames, s);
    if (rc) return rc;
    if (chain) {
        rc = chain_alloc(h, p, dtype, n_frames, flags, pipelined);
        if (rc) return rc;
    }
    h->last_kind = chain ? (h->ch_fused ? 4 : 3) : 0;
    h->last_fpl = chain ? h->ch_K : 1;
    h->last_fpb = chain ? h->ch_E : 1;
    h->ch_last_launches = (chain && p->refractory_period_s > 0) ? (n_frames + h->ch_K - 1) / h->ch_K + 1 : 0; // (chain_plan's length)
    KArgs a = make_kargs(h, p);
    if (probed) {
        rc = probe_reserve(h, n_frames);
        if (rc) return rc;
        if (!a.dbg_diff) { a.dbg_lognew = h->probe_planes; a.dbg_cms = a.dbg_lognew + h->npx_pad; a.dbg_diff = a.dbg_cms + h->npx_pad; }
    }
    if (pipelined)
        return run_pipelined(h, p, a, frames, dtype, n_frames, t_prev, t_frame, frame_idx0, events, cap, recs_dev,
                             (flags & V2E_RUN_FRAMES_RESIDENT) != 0, s);
    if (h->join_runs(s)) { // every other run goes whole on the caller's stream, behind every piece still in flight
        v2e_set_error("hipStreamWaitEvent failed");
        return V2E_EHIP;
    }
    rc = upload_run(h, p, n_frames, t_prev, t_frame, frame_idx0, frames, s);
    if (rc) return rc;
    if (mode == V2E_RUN_PROFILE)
        return chain ? run_profiled_chain(h, p, a, dtype, n_frames, events, cap, recs_dev, s)
                     : run_profiled_frames(h, p, a, frames, dtype, n_frames, events, cap, recs_dev, s);
    if (mode != 0) return run_graph(h, p, a, frames, dtype, n_frames, events, cap, recs_dev, chain, s);
    return chain ? enqueue_run_chain(h, p, a, dtype, n_frames, events, cap, recs_dev, s, ChainMode::plain)
                 : enqueue_run(h, p, a, frames, dtype, n_frames, events, cap, recs_dev, s);
}

// host-blocking: every piece of the LAST pipelined run that used scratch set `ticket` (v2e_emu_run_ticket right after that run) is complete
int v2e_emu_run_wait(v2e_emu *h, int ticket)
{
    V2E_REQUIRE(h && (ticket == 0 || ticket == 1), "bad ticket");
    if (h->piece_pending[ticket]) {
        V2E_HIP(hipEventSynchronize(h->ev_main_done2[ticket]));
        V2E_HIP(hipEventSynchronize(h->ev_tail_done2[ticket]));
    }
    return 0;
}
int v2e_emu_run_ticket(v2e_emu *h) { return h ? h->last_ticket : -1; }
int v2e_emu_event_writer(v2e_emu *h) { return (h && h->ch_K > 0) ? (h->ch_pull ? 1 : 0) : -1; }
const v2e_frame_rec *v2e_emu_run_recs(v2e_emu *h, int ticket, uint64_t *n_recs)
{
    if (!h || (ticket != 0 && ticket != 1)) return nullptr;
    if (n_recs) *n_recs = h->recs_host_n[ticket];
    return (const v2e_frame_rec *)h->recs_host[ticket];
}

// `stream` waits for every piece of every pipelined run (v2e_emu_run, V2E_RUN_PIPELINED) enqueued on this handle so far
int v2e_emu_run_join(v2e_emu *h, void *stream)
{
    V2E_REQUIRE(h, "null");
    V2E_HIP(hipSetDevice(h->device));
    if (h->join_runs((hipStream_t)stream)) { v2e_set_error("hipStreamWaitEvent failed"); return V2E_EHIP; }
    return 0;
}

int v2e_emu_launch_stamps(v2e_emu *h, int runs, uint64_t *out_ns, int cap_runs, int *n_runs, int *launches_per_run)
{
    V2E_REQUIRE(h && runs >= 0, "bad args");
    V2E_HIP(hipSetDevice(h->device));
    if (out_ns || n_runs) { // read back (blocking): the last min(stamp_seq, stamps_runs) runs, oldest first
        V2E_HIP(hipDeviceSynchronize());
        const unsigned long long have = std::min<unsigned long long>(h->stamp_seq, (unsigned long long)h->stamps_runs);
        const int n = (int)std::min<unsigned long long>(have, (unsigned long long)std::max(cap_runs, 0));
        if (n_runs) *n_runs = n;
        if (launches_per_run) *launches_per_run = STAMP_LAUNCHES;
        if (out_ns && n > 0) {
            std::vector<unsigned long long> tmp((size_t)h->stamps_runs * 2 * STAMP_LAUNCHES);
            V2E_HIP(hipMemcpy(tmp.data(), h->stamps, tmp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int r = 0; r < n; ++r) {
                const unsigned long long seq = h->stamp_seq - (unsigned long long)n + (unsigned long long)r;
                const unsigned long long *src = tmp.data() + (size_t)(seq % (unsigned long long)h->stamps_runs) * 2 * STAMP_LAUNCHES;
                for (int l = 0; l < STAMP_LAUNCHES; ++l) { // wall clock: 100 MHz (s_memrealtime); the start is kept complemented
                    const unsigned long long a = src[2 * l], b = src[2 * l + 1];
                    out_ns[((size_t)r * STAMP_LAUNCHES + l) * 2] = a ? (~a) * 10ull : 0ull;
                    out_ns[((size_t)r * STAMP_LAUNCHES + l) * 2 + 1] = b * 10ull;
                }
            }
        }
    }
    if (runs != h->stamps_runs) {
        V2E_HIP(hipDeviceSynchronize());
        hipFree(h->stamps);
        h->stamps = nullptr;
        h->stamps_runs = 0;
        h->stamp_seq = 0;
        if (runs > 0) {
            V2E_HIP(hipMalloc(&h->stamps, sizeof(unsigned long long) * (size_t)runs * 2 * STAMP_LAUNCHES));
            V2E_HIP(hipMemset(h->stamps, 0, sizeof(unsigned long long) * (size_t)runs * 2 * STAMP_LAUNCHES));
            V2E_HIP(hipDeviceSynchronize()); // (the fill is ordered on the default stream only: see chain_alloc)
            h->stamps_runs = runs;
        }
    }
    return 0;
}

// dev tool (not part of the public header): enable / read back the in-kernel timeline of one mid-run k_chain launch
int v2e_emu_debug_timeline(v2e_emu *h, unsigned long long *out_host /* [ngroups][16] or NULL to enable */, int *ngroups)
{
    V2E_REQUIRE(h, "null");
    V2E_HIP(hipSetDevice(h->device));
    if (!h->dbg) {
        V2E_HIP(hipMalloc(&h->dbg, sizeof(unsigned long long) * 16 * h->ngroups));
        V2E_HIP(hipMemset(h->dbg, 0, sizeof(unsigned long long) * 16 * h->ngroups));
        h->drop_graphs();
    }
    if (ngroups) *ngroups = h->ngroups;
    if (out_host) {
        V2E_HIP(hipDeviceSynchronize());
        V2E_HIP(hipMemcpy(out_host, h->dbg, sizeof(unsigned long long) * 16 * h->ngroups, hipMemcpyDeviceToHost));
    }
    return 0;
}

// dev tool (not part of the public header; scripts/chain_rounds.py, tests/test_chain_redo_gpu.py): the rule-on rows of the last
// run's chain launches, [launches][K + 1 rows][n_clips][K] -- row 0 what a launch's own pass flagged, row r what the r-th redo pass
// on it flagged.  *launches: the last run's launch count (0: it had no refractory chain); the buffer holds ch_launch_cap launches,
// and those beyond the last run's were not cleared by it.
int v2e_emu_debug_chain_rows(v2e_emu *h, uint32_t *out, size_t cap_words, int *launches, int *K)
{
    V2E_REQUIRE(h && launches && K, "null");
    *launches = h->ch_last_launches; *K = h->ch_K;
    if (!h->cur().ch_gM || !out || h->ch_last_launches <= 0) return 0;
    V2E_HIP(hipSetDevice(h->device));
    V2E_HIP(hipDeviceSynchronize());
    const size_t n = (size_t)h->ch_last_launches * (h->ch_K + 1) * h->n_clips * h->ch_K;
    V2E_HIP(hipMemcpy(out, h->cur().ch_gM, sizeof(uint32_t) * std::min(n, cap_words), hipMemcpyDeviceToHost));
    return 0;
}

int v2e_emu_last_profile(v2e_emu *h, double *ms_count, double *ms_rank, double *ms_scan, double *ms_emit, int *launches)
{
    V2E_REQUIRE(h && ms_count && ms_rank && ms_scan && ms_emit && launches, "null");
    *ms_count = h->prof_ms[0]; *ms_rank = h->prof_ms[1]; *ms_scan = h->prof_ms[2]; *ms_emit = h->prof_ms[3];
    *launches = h->prof_launches;
    return 0;
}

int v2e_emu_chain_plan(int n_frames, int frames_per_launch, int frames_per_batch, int ring_batches, int has_refractory,
                       int fused_records, int32_t *out, int cap)
{
    V2E_REQUIRE(n_frames > 0 && frames_per_launch >= 1 && frames_per_launch <= CHAIN_K_MAX && frames_per_batch >= frames_per_launch &&
                frames_per_batch % frames_per_launch == 0 && ring_batches >= 3, "bad plan arguments");
    const std::vector<ChainLaunch> plan = chain_plan(n_frames, frames_per_launch, frames_per_batch, ring_batches, has_refractory != 0,
                                                     fused_records != 0);
    if (out) {
        V2E_REQUIRE(cap >= (int)plan.size(), "plan buffer too small");
        for (size_t i = 0; i < plan.size(); ++i) {
            const ChainLaunch &c = plan[i];
            const int32_t row[8] = {c.f0, c.nf, c.pf0, c.pnf, c.wait_join, c.wait_ahead, c.ahead_next, c.emit_batch};
            memcpy(out + 8 * i, row, sizeof(row));
        }
    }
    return (int)plan.size();
}

int v2e_emu_last_pipeline(v2e_emu *h, int *kind, int *frames_per_launch, int *frames_per_batch)
{
    V2E_REQUIRE(h && kind && frames_per_launch && frames_per_batch, "null");
    *kind = h->last_kind; *frames_per_launch = h->last_fpl; *frames_per_batch = h->last_fpb;
    return 0;
}

int v2e_emu_last_run_queue_ops(v2e_emu *h, int out[3])
{
    V2E_REQUIRE(h && out, "null");
    V2E_REQUIRE(h->last_kind >= 3, "the last run did not go through k_chain");
    memcpy(out, h->last_queue_ops, sizeof(h->last_queue_ops));
    return 0;
}

int v2e_emu_last_profile_launches(v2e_emu *h, float *us, int cap, int *n)
{
    V2E_REQUIRE(h && n, "null");
    *n = (int)h->prof_chain_us.size();
    for (int i = 0; us && i < cap && i < *n; ++i) us[i] = h->prof_chain_us[i];
    return 0;
}

int v2e_emu_last_profile_pipe(v2e_emu *h, int *emit_batches, int *frames_per_batch, int *step_launches)
{
    V2E_REQUIRE(h && emit_batches && frames_per_batch, "null");
    *emit_batches = h->prof_emit_batches;
    *frames_per_batch = h->last_fpb;
    if (step_launches) *step_launches = h->prof_step_launches;
    return 0;
}

} // extern "C"
