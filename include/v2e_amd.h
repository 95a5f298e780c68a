/*
 * v2e_amd.h -- C ABI of libv2e_amd.so, the MI355X (gfx950) implementation of the
 * v2e hot path.  Plain pointers and sizes only; no torch types.  Every device
 * pointer is memory owned by the caller (PyTorch-ROCm tensors in the Python host);
 * the library allocates only its private scratch at create().
 *
 * All functions return 0 on success or a negative V2E_E* code; nothing throws
 * across the boundary.  Unless stated otherwise a call only enqueues work on the
 * given hipStream_t (passed as void*) and returns.
 *
 * Reference interfaces replaced (paths relative to the SensorsINI/v2e tree):
 *   v2ecore/emulator.py:439-511   EventEmulator._init            -> v2e_emu_init_state
 *   v2ecore/emulator.py:656-775   generate_events, front half    -> v2e_emu_count
 *     (lin_log emulator_utils.py:18-45, rescale_intensity_frame :48-54,
 *      low_pass_filter :57-109, subtract_leak_current :114-134,
 *      compute_event_map :137-173, generate_shot_noise :297-351)
 *   v2ecore/emulator.py:791-942   iteration loop, refractory, event list,
 *      shot-noise events, base update (get_event_list_from_coords :1024-1059)
 *                                                                -> v2e_emu_rank + v2e_emu_emit
 *   v2ecore/emulator.py:867-869   randperm shuffle               -> v2e_emu_permute
 *   v2ecore/model.py:10-226       UNet / down / up               -> v2e_unet_forward
 *   v2ecore/model.py:229-300      backWarp                       -> v2e_slomo_prep / _fuse
 *   v2ecore/slomo.py:404-433      per-t blend, warps, fusion     -> v2e_slomo_prep / _fuse
 */
#ifndef V2E_AMD_H
#define V2E_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V2E_OK 0
#define V2E_EINVAL (-22)
#define V2E_ENOMEM (-12)
#define V2E_EHIP (-5)      /* a HIP runtime call failed; see v2e_last_error() */
#define V2E_ENODEV (-19)
#define V2E_EOVERFLOW (-75)

/* frame element types accepted by the emulator (emulator.py:663 converts all to f64) */
#define V2E_DT_U8 0
#define V2E_DT_F32 1
#define V2E_DT_F64 2

#define V2E_RNG_TAPE 0   /* random numbers / timestamps / permutations supplied by host */
#define V2E_RNG_PHILOX 1 /* counter-based Philox4x32-10 in-kernel (include/v2e_detmath.h) */

/* record flags */
#define V2E_FLAG_EVENTS_DROPPED 1u /* event buffer capacity exceeded; counts are still exact */
#define V2E_FLAG_ITERS_CLAMPED 2u  /* max events per pixel exceeded max_iters: frame NOT emitted */
#define V2E_FLAG_SYNC_TIMEOUT 4u   /* in-kernel workgroup rendezvous timed out: results invalid */

/*
 * DVS model parameters, read at every call (the reference reads plain attributes
 * lazily, so callers may change them between frames, e.g. set_dvs_params()).
 * Scalars that the reference computes in Python doubles stay doubles here.
 */
typedef struct v2e_emu_params {
    int32_t f64_state;      /* 1: lp/base planes are double (cutoff_hz > 0), 0: float   */
    int32_t scalar_thres;   /* 1: sigma_thres == 0, thresholds are Python floats        */
    int32_t rng_mode;       /* V2E_RNG_TAPE / V2E_RNG_PHILOX                            */
    int32_t shuffle;        /* philox mode: apply the keyed bijection per iteration     */
    double pos_thres_nominal, neg_thres_nominal;
    double pos_thres_scalar, neg_thres_scalar; /* used when scalar_thres                */
    double sigma_thres;
    double cutoff_hz;
    double leak_rate_hz;
    double leak_jitter_fraction;
    double noise_rate_cov_decades;
    double refractory_period_s;
    double shot_noise_rate_hz;
    double shot_noise_inten_factor; /* emulator.py:210, 0.25 */
    float pos_pre_scalar, neg_pre_scalar; /* nominal/thres when scalar_thres (host torch.div) */
    uint64_t seed;          /* philox key */
    int32_t log_input;      /* hdr=True (emulator.py:304, 666): frames are already log intensity, no lin_log;
                               the state is float64 even without a cutoff (f64_state must be 1) */
    int32_t photoreceptor_noise; /* emulator.py:694-703: low-passed Gaussian noise on the photoreceptor output instead of
                                    Poisson shot events (frame-at-a-time API only); pass shot_noise_rate_hz = 0 with it */
    double photoreceptor_noise_vrms; /* emulator_utils.py:177-290, evaluated by the host */
} v2e_emu_params;

/* Per-(frame, clip) result record, written on device. */
typedef struct v2e_frame_rec {
    int32_t max_events;  /* max_num_events_any_pixel (emulator.py:773) */
    uint32_t flags;
    uint32_t n_signal;   /* signal events after refractory filtering   */
    uint32_t n_events;   /* signal + shot                              */
    uint32_t n_on, n_off;/* totals incl. shot (emulator.py:1038-1040)  */
    uint64_t ev_offset;  /* first row of this frame in the clip's event region */
} v2e_frame_rec;

typedef struct v2e_emu v2e_emu;

const char *v2e_last_error(void);
int v2e_version(void);

/*
 * H, W: sensor size; n_clips: independent pixel arrays advanced in lock-step by one
 * launch (state planes are [n_clips][npx_pad], npx_pad = v2e_emu_npx_pad(H,W));
 * max_iters: cap on events per pixel per frame (hist scratch is sized by it).
 */
int v2e_emu_create(int H, int W, int n_clips, int max_iters, int device, v2e_emu **out);
int v2e_emu_destroy(v2e_emu *h);
int64_t v2e_emu_npx_pad(int H, int W);

/* Device pointers to the persistent per-pixel state (caller-owned, [n_clips][npx_pad]).
 * lp/base are double planes when params.f64_state else float planes. */
int v2e_emu_bind_state(v2e_emu *h, void *lp, void *base, float *ts_mem,
                       float *pos_thres, float *neg_thres, float *noise_rate);

/*
 * First frame (emulator.py:681-717 + _init :439-511).  frame: [n_clips][H*W] of
 * `dtype`.  Tape mode: thres_pos/thres_neg hold the torch.normal draws (pre-clamp)
 * and noise_rate the final exp() values (or NULL when unused); Philox mode: pass
 * NULL and they are generated in-kernel.
 */
int v2e_emu_init_state(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype,
                       double t_frame, const float *thres_pos, const float *thres_neg,
                       const float *noise_rate, void *stream);

/* Photoreceptor-noise state (emulator.py:684, 694-703): pn_arr is the float64 plane [n_clips][npx_pad]
 * `photoreceptor_noise_arr` (caller-owned, zero on the first frame); randn_tape the float32 draws
 * torch.randn(shape) of the coming frame in tape mode (NULL in Philox mode).  Both are consumed by the next
 * v2e_emu_count when params.photoreceptor_noise is set; NULL pn_arr switches the feature off. */
/* SCIDVS pixel (emulator.py:56-80, 719-725, 747): device planes [n_clips][npx_pad] scidvs_highpass and
 * scidvs_previous_photo (state dtype) and scidvs_tau_arr (float32; filled by v2e_emu_init_state in Philox mode, by the
 * caller in tape mode).  first_frame_idx: the frame index at which scidvs_previous_photo is taken from the frame itself
 * (emulator.py:720-722).  All NULL switches it off.  Runs on the count / rank / scan / emit kernels. */
int v2e_emu_set_scidvs(v2e_emu *h, void *highpass, void *previous_photo, float *tau, uint32_t first_frame_idx);

/* Model-state planes the reference keeps as attributes and the kernels otherwise never store: log_new_frame (emulator.py:666),
 * c_minus_s_frame (:753, zero without CSDVS) and diff_frame (:749-754), float64 [n_clips][npx_pad] each (caller-owned), written
 * by every v2e_emu_count from then on -- what show_dvs_model_state / record_single_pixel_states (emulator.py:756-764, 985-1006)
 * read.  All three or none (NULL switches it off).  Frame-at-a-time kernels only. */
int v2e_emu_set_model_state_planes(v2e_emu *h, double *log_new_frame, double *c_minus_s_frame, double *diff_frame);

int v2e_emu_set_pnoise(v2e_emu *h, void *pn_arr, const float *randn_tape);

/* Single-pixel model states inside v2e_emu_run (emulator.py:985-1009 per frame, the recorder behind --record_single_pixel_states,
 * emulator.py:279-300; plotted by scripts/plot_single_pixel_states.py): the NEXT v2e_emu_run records, for each of n probed pixels
 * (pixel_index: host array, row * W + col, the reference's plane[row, col]; the same pixel may be named twice) and each of its
 * frames, the reference's ten series minus `time`, which the host knows, as float64 out_dev[n_frames][n][V2E_PROBE_FIELDS] in the
 * order
 *   0 new_frame        the frame's input value at the pixel                                            (emulator.py:988)
 *   1 base_log_frame   after the frame's base update (emulator.py:936-942)                             (:989)
 *   2 lp_log_frame                                                                                     (:990)
 *   3 log_new_frame    the float32 value lin_log returns (emulator_utils.py:45)                        (:991)
 *   4 pos_thres, 5 neg_thres   the pixel's thresholds, or the scalars when params.scalar_thres         (:992-995)
 *   6 diff_frame       emulator.py:749-754                                                             (:996)
 *   7 final_neg_evts_frame, 8 final_pos_evts_frame   the frame's SIGNAL events at the pixel, OFF and ON (:997-998)
 * out_dev is device memory of the caller that holds the next run's n_frames blocks; the run writes every element and does not clear
 * or read it.  The setting is consumed by that run (one shot: a later run is unprobed unless the call is made again); n == 0 cancels
 * it.  n <= V2E_PROBE_MAX, every index in [0, H * W), handles of one clip only.  A probed run goes through the per-frame kernels
 * (v2e_emu_last_pipeline reports kind 0; with V2E_RUN_REQUIRE_CHAIN it fails), never pipelined, with three small launches beside
 * them: a tap behind k_count and one behind k_emit of every frame, and one pass over the run's event rows at the end.  The run
 * keeps the model-state planes on (v2e_emu_set_model_state_planes; planes of the library's own where the caller has bound none).
 * A run without probes launches nothing of this. */
#define V2E_PROBE_FIELDS 9
#define V2E_PROBE_MAX 64
int v2e_emu_set_probes(v2e_emu *h, const int32_t *pixel_index, int n, double *out_dev);

/* Centre-surround DVS (cs_lambda_pixels; emulator.py:245-272, 707-716, 753-754, 1061-1124).  The surround plane
 * cs_surround_frame [n_clips][npx_pad] (state dtype, caller-owned) is what v2e_emu_count subtracts from the photoreceptor
 * output: diff = (photoreceptor + noise - surround) - base; NULL switches the feature off.  Per frame the caller
 *   1. v2e_emu_lp_preview: the frame's lp_log_frame (the low-pass of emulator.py:685-690 applied to the state as it is,
 *      written to lp_out, the state untouched),
 *   2. v2e_csdvs_update:   steps the diffuser against it (below),
 *   3. v2e_emu_count ...:  the frame itself (recomputes the same lp_log_frame).
 * On the first frame the surround is a copy of lp_log_frame and base_log_frame is zero (emulator.py:1062-1063, 715). */
int v2e_emu_set_csdvs(v2e_emu *h, const void *surround);
int v2e_emu_lp_preview(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype, const double *t_prev,
                       const double *t_frame, uint32_t frame_idx, void *lp_out, void *stream);
/* EventEmulator._update_csdvs (emulator.py:1098-1124) on device planes of H x W values (float64 if f64 else float32):
 * up to num_steps Euler steps  h += alpha_p (p - h) + alpha_h conv2d(ReplicationPad2d(1)(h.float()), [[0,1,0],[1,-4,1],[0,1,0]])
 * stopping after the first step whose max |change| is <= max_change_to_stop (1e-5 in the reference).  The float32 5-point
 * sum is taken in kernel order ((((top + left) - 4 centre) + right) + bottom) -- what torch's CPU convolution does on planes
 * of 200 x 200 and more (DAVIS346 included; on small planes its backend sums in another order, see csdvs.hip).  h_scratch: a
 * second plane of the same size.  steps_taken: the reference's `steps`; last_max_change (may be NULL): its `max_change`.
 * Synchronises the stream once per 32 steps. */
/* CSDVS inside a device-resident run (v2e_emu_run; one clip): per frame of the COMING run the Euler parameters the host
 * computes as emulator.py:1066-1096 does (alpha_p, alpha_h, num_steps), a scratch surround plane and a plane for the frame's
 * lp_log_frame (state dtype, [npx_pad] each, caller-owned), and steps_taken_dev (device int32 [n_frames]: the reference's `steps`
 * per frame, readable after the run).  The run then steps the diffuser on the stream before every frame: every one of the frame's
 * num_steps launches is enqueued and the ones after the step that settles (max |change| <= max_change_to_stop, evaluated on the
 * device) return at once -- no host step, capturable in the run's hipGraph.  n_frames = 0 clears it. */
int v2e_emu_set_csdvs_run(v2e_emu *h, void *h_scratch, void *lp_scratch, const double *alpha_p, const double *alpha_h,
                          const int *num_steps, int n_frames, double max_change_to_stop, int *steps_taken_dev);
int v2e_csdvs_update(const void *p_plane, void *h_plane, void *h_scratch, int H, int W, int f64, double alpha_p, double alpha_h,
                     int num_steps, double max_change_to_stop, int *steps_taken, double *last_max_change, void *stream);

/*
 * Front half of one time step for all clips: photoreceptor, IIR, leak, event
 * counts, shot-noise decisions, global max.  leak_randn/shot_rand: [n_clips][npx_pad]
 * host-drawn tapes (tape mode) or NULL (Philox).  frame_idx: Philox counter word and
 * record slot (rec slot = frame_idx % ring).  t_prev/t_frame: per-clip host arrays.
 */
int v2e_emu_count(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype,
                  const double *t_prev, const double *t_frame, uint32_t frame_idx,
                  const float *leak_randn, const float *shot_rand, void *stream);

/* Blocking: copy the per-clip records of `frame_idx` to host (syncs the stream). */
int v2e_emu_read_rec(v2e_emu *h, uint32_t frame_idx, v2e_frame_rec *recs_host, void *stream);

/* Shot-noise decisions as their own pass (tape mode only: the reference draws `rand`
 * after the per-iteration randperms, emulator.py:868 then :906 / emulator_utils.py:338). */
int v2e_emu_shot(v2e_emu *h, const v2e_emu_params *p, const void *frame, int dtype,
                 uint32_t frame_idx, const float *shot_rand, void *stream);

/* Grow the per-iteration scratch if max_events exceeds the create()-time max_iters
 * (blocking; frame-at-a-time API only, after v2e_emu_read_rec). */
int v2e_emu_reserve_iters(v2e_emu *h, int max_events, void *stream);

/*
 * Back half, step 1: refractory filter (emulator.py:830-846) and per-(iteration,
 * polarity) histograms + exclusive scan; no state is modified.  ts_table: device
 * [n_clips][n_ts] float32 timestamps (torch.linspace drawn by the host, tape mode)
 * or NULL for the in-kernel formula.  Totals are readable with
 * v2e_emu_read_iter_counts afterwards.
 */
int v2e_emu_rank(v2e_emu *h, const v2e_emu_params *p, uint32_t frame_idx, const float *ts_table,
                 int n_ts, void *stream);

/*
 * Back half, step 2 (after v2e_emu_rank): dense [N,4] float32 (t,x,y,p) list in
 * reference order (emulator.py:861-923), base/ts_mem update (:936-942), record.
 * events: device [n_clips][cap][4] float32.  ev_offset0: per-clip host array of the
 * row at which this frame's events start (NULL: continue after the previous frame).
 */
int v2e_emu_emit(v2e_emu *h, const v2e_emu_params *p, uint32_t frame_idx,
                 const float *ts_table, int n_ts, float *events, uint64_t cap,
                 const uint64_t *ev_offset0, void *stream);

/* Blocking: per-iteration (on_i, off_i) totals of the last emitted frame,
 * host array [n_clips][2*(max_events+1)]; the last pair is the shot-noise pair. */
int v2e_emu_read_iter_counts(v2e_emu *h, uint32_t frame_idx, int n_iters, uint32_t *counts_host,
                             void *stream);

/* out[dst0 + j] = in[src0 + idx[j]], j < n   (events_curr_iter[idx], emulator.py:869) */
int v2e_emu_permute(v2e_emu *h, const float *events_in, float *events_out, const int32_t *idx,
                    uint64_t row0, uint64_t n, void *stream);

/* One frame of the frame-at-a-time API in one call (Philox mode, one clip; replaces the sequence v2e_emu_count /
 * read_rec / rank / read_iter_counts / emit + the row copy of EventEmulator.generate_events, emulator.py:619-1022): the
 * frame (host pointer if frame_on_host, else device) is counted, ranked and scanned, the frame record and per-key totals
 * come back in ONE read, the rows are emitted into events_dev[0 .. n) and copied to pinned host memory owned by the
 * handle (*events_host, valid until the next call; NULL when n = 0).  out8 = {n_events, n_on, n_off, n_signal, M, 0, 0, 0}.
 * Returns 0; 1 if M > the handle's max_iters (counted, nothing emitted: grow with v2e_emu_reserve_iters, then
 * v2e_emu_rank / v2e_emu_emit); 2 if n_events > cap (same); negative on error.  Synchronises `stream`. */
int v2e_emu_frame(v2e_emu *h, const v2e_emu_params *p, const void *frame, int frame_on_host, int dtype, double t_prev,
                  double t_frame, uint32_t frame_idx, float *events_dev, uint64_t cap, uint32_t *out8,
                  const float **events_host, void *stream);
/* Where the NEXT v2e_emu_frame call puts its rows: a caller-owned PINNED host buffer of cap_rows rows of 4 floats (hipHostMalloc
 * / hipHostRegister memory, e.g. a torch pin_memory tensor), written by the frame's last kernel directly -- *events_host then
 * equals pinned_rows and the caller needs no copy.  One frame only; a frame with more rows than cap_rows is delivered in the
 * handle's own buffer as before (*events_host says which).  NULL / 0 cancels. */
int v2e_emu_frame_host_rows(v2e_emu *h, float *pinned_rows, uint64_t cap_rows);

/* v2e_emu_run flags (an OR of these; the low two bits are one of 0 plain launches, V2E_RUN_GRAPH, V2E_RUN_PROFILE). */
#define V2E_RUN_GRAPH 1                  /* capture the run into a hipGraph, cached while everything baked into it is unchanged */
#define V2E_RUN_PROFILE 2                /* instrumented and blocking: see v2e_emu_last_profile */
#define V2E_RUN_PER_FRAME_KERNELS 16     /* count / rank / scan / emit one frame at a time instead of k_chain (also what photoreceptor
                                            noise, SCIDVS, CSDVS, float64 log frames and > 1024 events per pixel and frame always run) */
#define V2E_RUN_ONE_FRAME_PER_LAUNCH 128 /* k_chain with one frame per launch (clips whose refractory rule is active on most frames) */
#define V2E_RUN_REQUIRE_CHAIN 256        /* k_chain or an error where it cannot run */
#define V2E_RUN_PIPELINED 1024           /* plain launches only: consecutive runs overlap (below) */
#define V2E_RUN_FRAMES_RESIDENT 2048     /* with V2E_RUN_PIPELINED: nothing enqueued on `stream` still writes `frames` */

/*
 * Philox-mode, fully device-resident multi-frame run: frames [n_frames][n_clips][H*W],
 * t_prev/t_frame host arrays [n_frames][n_clips].  Records for frame f go to
 * recs_dev[f][clip] (device, caller-owned).  No host synchronisation inside.  Every mode gives identical results.
 * The k_chain pipeline (K frames per launch, the per-pixel state in registers, the event list built behind it in batches on
 * streams of the handle) runs wherever it can; otherwise the per-frame kernels.  The pipeline reads the run's frame scalars, first
 * frame index and the ADDRESS of `frames` from device variables the run's upload fills: a cached graph is replayed over whatever
 * `frames` buffer a call names, while `events` / `recs_dev` are baked in (callers alternate between fixed buffer sets).
 * Without V2E_RUN_PIPELINED the run's work is complete on `stream` when it ends there.
 * PIPELINED runs (V2E_RUN_PIPELINED with plain launches, wherever k_chain runs): `stream` carries the chain's launches and nothing
 * else, so it orders the PIXEL STATE only; the run's upload, zero fills and k_ahead records go to a stream of the handle that runs
 * ahead of the chain, the emission's tables and rows to two more that finish beside the run after.  The run's event rows and records
 * are complete behind v2e_emu_run_wait (host) / v2e_emu_run_join (a stream), which the caller must call before reading them; every
 * other entry point of the handle joins by itself.  Everything two runs in flight would share exists twice: callers alternate two
 * sets of `events` / `recs_dev` buffers (a run that names the buffers of the run before it waits for that run).  With
 * V2E_RUN_FRAMES_RESIDENT the run's head does not wait for `stream`, i.e. for the chain of the run before.
 */
int v2e_emu_run(v2e_emu *h, const v2e_emu_params *p, const void *frames, int dtype, int n_frames,
                const double *t_prev, const double *t_frame, uint32_t frame_idx0, float *events,
                uint64_t cap, v2e_frame_rec *recs_dev, int flags, void *stream);
/* `stream` waits (device side, no host block) for every piece of every pipelined run enqueued on the handle so far. */
int v2e_emu_run_join(v2e_emu *h, void *stream);
/* The scratch set (0 / 1) the run enqueued last took if the library enqueued it in pieces (the ticket of that run, valid until the
 * second-next such run), or -1: that run is whole on its stream. */
int v2e_emu_run_ticket(v2e_emu *h);
/* Host-blocking: every piece of the last pipelined run with that ticket has completed (its rows and records can be read). */
int v2e_emu_run_wait(v2e_emu *h, int ticket);
/* The records [n_frames][n_clips] of the last pipelined run with that ticket in pinned host memory of the handle (copied there behind
 * the run's last rows; valid behind v2e_emu_run_wait, until the second-next pipelined run); *n_recs = how many. */
const v2e_frame_rec *v2e_emu_run_recs(v2e_emu *h, int ticket, uint64_t *n_recs);

/* After an instrumented v2e_emu_run (blocking): summed milliseconds per kernel class and frames.
 * k_chain pipeline (a HIP event before and after every chain launch, on its stream): ms_count = first
 * launch's start to last launch's end (gaps included), ms_rank = the sum of the chain kernels' own
 * durations, ms_emit = the k_cemit launches (v2e_emu_last_profile_pipe), ms_scan 0;
 * V2E_RUN_PER_FRAME_KERNELS: k_count, k_rank, k_scan, k_emit (a hipEvent before every launch). */
int v2e_emu_last_profile(v2e_emu *h, double *ms_count, double *ms_rank, double *ms_scan,
                         double *ms_emit, int *launches);

/* The launch schedule v2e_emu_run uses for a run of n_frames frames (no GPU needed; for tests and tooling): returns the
 * number of chain launches and, if out != NULL, writes per launch 8 int32: the frames it advances (f0, nf; nf = 0: the
 * tail launch that only validates), the frames of its predecessor it validates (pf0, pnf), the emission batch it must wait
 * for before reusing ring slots, the k_ahead batch it needs, the k_ahead batch enqueued behind it, the emission batch
 * that is final once it is enqueued; -1 = none.  Batch b = frames [b * frames_per_batch, (b + 1) * frames_per_batch). */
int v2e_emu_chain_plan(int n_frames, int frames_per_launch, int frames_per_batch, int ring_batches, int has_refractory,
                       int fused_records, int32_t *out, int cap);

/* Emission batches timed by the last instrumented run, the frames per emission batch, and the
 * number of chain launches ms_count covers (step_launches may be NULL). */
int v2e_emu_last_profile_pipe(v2e_emu *h, int *emit_batches, int *frames_per_batch, int *step_launches);
/* The chain launches of the last instrumented run one by one, in launch order (microseconds; the last one is the tail launch
 * that only validates): *n = how many there were, the first min(cap, *n) written to us (may be NULL). */
int v2e_emu_last_profile_launches(v2e_emu *h, float *us, int cap, int *n);

/* Device time stamps of the chain kernel, per launch, in the configuration that is actually timed (graph replay, side streams running):
 * every k_chain launch of the runs enqueued after v2e_emu_launch_stamps(h, runs > 0, NULL, 0, NULL, NULL) leaves the wall-clock time
 * of its first workgroup's start and of its last workgroup's end (two atomics per workgroup; s_memrealtime, 100 MHz) in a ring of
 * `runs` runs.  With out_ns != NULL or n_runs != NULL the call first synchronises the device and copies the last min(cap_runs, runs
 * stamped) runs out, oldest first: out_ns[run][launch][2] = {start, end} in nanoseconds of the device clock, *launches_per_run
 * entries per run (0 / 0: the run had no such launch); then `runs` takes effect (0 switches the stamps off; a changed value
 * re-allocates the ring and forgets what it held).  What bench.py's roofline object divides the chain's algorithmic bytes by. */
int v2e_emu_launch_stamps(v2e_emu *h, int runs, uint64_t *out_ns, int cap_runs, int *n_runs, int *launches_per_run);

/* The event writer of the handle's k_chain pipeline: 1 = k_cpull (a thread per output row; needs 32 bytes of pixel ballots per frame
 * of the table sets, group and key: 281 MB at 346x260 with max_iters = 64), 0 = k_cemit (the push writer: same rows, 1.5x the bytes
 * written), -1 = no such run yet.  Chosen when the pipeline's scratch is allocated: the pull where its tables fit a quarter of the free
 * device memory AND an absolute budget (24 GB per scratch set; V2E_AMD_PULL_BUDGET_MB), V2E_AMD_EMIT_PULL=0 forces the push writer. */
int v2e_emu_event_writer(v2e_emu *h);

/* Which pipeline the last v2e_emu_run on this handle used: kind 0 = unfused count/rank/scan/emit, 3 = k_chain (K frames
 * per launch, state in registers; records from k_ahead), 4 = k_chain with the per-frame records built inside the chain;
 * frames_per_launch of the dependency chain and frames per emission batch. */
int v2e_emu_last_pipeline(v2e_emu *h, int *kind, int *frames_per_launch, int *frames_per_batch);
/* What the schedule of the last v2e_emu_run through k_chain put on the caller's stream: out = {kernel launches, stream waits, event
 * records} (a graph run: what its capture held).  A pipelined run's schedule puts the chain's launches there, one wait for the run's
 * head plus one per batch where the ring wraps, and no record: every event that says "this chain launch has finished" is that
 * launch's stop event.  (Not the schedule's and not counted: without V2E_RUN_FRAMES_RESIDENT one record IN FRONT of the run orders
 * its head behind the caller's earlier work.)  Fails where the last run had no k_chain. */
int v2e_emu_last_run_queue_ops(v2e_emu *h, int out[3]);

/* ------------------------------------------------------------- SuperSloMo */

/* one 2-D convolution layer of the UNet (model.py: nn.Conv2d + leaky_relu 0.1) */
typedef struct v2e_conv_desc {
    const float *weight; /* device, pre-packed [Cin][k][k][Cout] (v2e_pack_conv_weight) */
    const float *bias;   /* device [Cout] */
    int32_t cin, cout, ksize;
    int32_t split_kind;  /* what weight_s3 holds: 0 three bf16 pieces (v2e_pack_conv_weight_s3); 2 | (scale_log2 << 8): two float16
                          * pieces of the weights times 2^scale_log2 (v2e_pack_conv_weight_h2) */
    const void *weight_s3; /* device, split weights or NULL: f32-MFMA kernel only */
} v2e_conv_desc;

/* repack torch [Cout][Cin][k][k] -> [Cin][k][k][Cout] on device */
int v2e_pack_conv_weight(const float *w_oihw, float *w_packed, int cout, int cin, int k, void *stream);

/*
 * The same weights split exactly into three bf16 pieces (w = p0 + p1 + p2) for the bf16-matrix-core convolution that
 * keeps f32 accuracy (six piece products per multiply, f32 accumulation; v2e_amd/csrc/slomo_s3.h):
 * [ceil(Cin/16)][k*k][3][2][Cout][8 bf16] = 6 bytes per weight of the padded tensor (a last partial 16-channel chunk
 * is padded with zero weights): w_s3 must hold ceil(cin/16)*16 * k*k * cout * 6 bytes.
 */
int v2e_pack_conv_weight_s3(const float *w_oihw, void *w_s3, int cout, int cin, int k, void *stream);
/* The same with TWO float16 pieces (w = h0 + h1 + r, |r| <= 2^-22 |w|) for the three-product convolution (conv_math "fp16x2":
 * half the matrix-core work, a product good to ~2^-21; v2e_amd/csrc/slomo_s3.h): [ceil(Cin/16)][k*k][2][2][Cout][8 f16] =
 * 4 bytes per weight of the padded tensor.  The weights are split times 2^scale_log2 (choose it so that the layer's largest
 * |w| 2^scale_log2 is below 2^14: nothing overflows float16 and no weight piece falls into its subnormal range); the
 * convolution divides it out again exactly.  Set v2e_conv_desc.split_kind = 2 | (scale_log2 << 8) with it. */
int v2e_pack_conv_weight_h2(const float *w_oihw, void *w_h2, int cout, int cin, int k, int scale_log2, void *stream);
/* Range guard of the two-float16-piece convolutions inside v2e_unet_forward: while a device flag is set here (per host thread;
 * NULL switches it off), a forward pass ORs 1 into it if the network input holds an inf or a NaN, or a convolution's output an inf
 * (seen in the range slot the producer left: the largest |value| of the input and of every convolution's output is tracked on the
 * device -- a NaN counts for the input only; one in a convolution's output needs an inf or a NaN upstream, which was flagged there
 * -- and a two-piece convolution stages its activations times the power of two that puts that maximum in [2^13, 2^14): finite
 * activations of any magnitude stay in float16's normal range).  The caller zeroes the flag, runs the pass, reads it back, and on 1 redoes it with the exact three-piece
 * weights -- what SloMoEngine's default conv math "auto" does.  A two-piece v2e_conv2d_lrelu called on its own stages unscaled and
 * is not watched. */
int v2e_conv_set_range_flag(int *device_flag);

/* activations in the same split form: x [n][c][h][w] f32 -> xs [3 pieces][n][c/8][h][w][8 bf16] (6 bytes per element;
 * c a multiple of 8).  A convolution takes such an input with pre = 3 (3x3 layers with split weights). */
int v2e_split3_nchw(const float *x, void *xs, int n, int c, int h, int w, void *stream);

/*
 * y = leaky_relu(conv2d(cat(x0, x1), W) + b, 0.1), stride 1, zero pad (k-1)/2, NCHW f32.
 * x1 may be NULL (c1 = 0).  pre: 0 none, 1 avg_pool2d(x0,2) fused on load (x0 is
 * [N][c0][2H][2W]), 2 bilinear x2 upsample (align_corners=False) fused on load
 * (x0 is [N][c0][H/2][W/2]), 3 x0 is a pre-split tensor (v2e_split3_nchw; 3x3 layers with split weights only).
 */
int v2e_conv2d_lrelu(const float *x0, int c0, const float *x1, int c1, int pre,
                     const v2e_conv_desc *conv, float *y, int n, int h, int w, void *stream);

/* 23-conv UNet forward (model.py:198-226).  convs: 23 descriptors in forward order;
 * workspace: device scratch of v2e_unet_workspace_bytes(n,h,w) bytes. */
int64_t v2e_unet_workspace_bytes(int n, int h, int w, int cin);
int v2e_unet_forward(const float *x, int cin, const v2e_conv_desc *convs, int cout, float *y,
                     int n, int h, int w, void *workspace, void *stream);

/*
 * slomo.py:405-419 for `n_t` time points of one batch: flow blend, two backWarps and
 * assembly of the 12-channel interpolation input
 * [I0,I1,F01(2),F10(2),Ft1(2),Ft0(2),g1,g0] -> x12 [n_t*b][12][h][w].
 * flow: flow-UNet output [b][4][h][w]; tcoef: DEVICE array [n_t][6] float32 =
 * {fCoeff[0..3], wCoeff[0..1]} of slomo.py:406-407,429, evaluated by the host in doubles.
 */
int v2e_slomo_prep(const float *i0, const float *i1, const float *flow, const float *tcoef, int n_t,
                   int b, int h, int w, float *x12, void *stream);

/* slomo.py:421-433: refine flows, visibility, two backWarps, fusion -> out [n_t*b][1][h][w] */
int v2e_slomo_fuse(const float *i0, const float *i1, const float *x12, const float *intrp,
                   const float *tcoef, int n_t, int b, int h, int w, float *out, void *stream);

/* slomo.py:352-368 (auto_upsample): max over the batch and both flow pairs of the SQUARED flow magnitude vx*vx + vy*vy (float32,
 * each operation rounded) of flow [b][4][h][w] = [F_0_1 x, y, F_1_0 x, y], as float32 bits in *out_bits (device); the host takes
 * one float32 sqrt of it (sqrt is monotone: the same number as the reference's max of sqrt planes).  0xffffffff: a NaN flow. */
int v2e_slomo_max_speed2(const float *flow, int b, int h, int w, uint32_t *out_bits, void *stream);

/* v2e_slomo_max_speed2 per batch of a flow chunk in one launch: flow [b][4][h][w] cut into consecutive batches of `seg` pairs (the
 * last one may be shorter); out_bits[ceil(b / seg)] (device) gets each batch's value, bit for bit what v2e_slomo_max_speed2 gives
 * for that batch alone (0xffffffff: a NaN flow in that batch). */
int v2e_slomo_max_speed2_seg(const float *flow, int b, int seg, int h, int w, uint32_t *out_bits, void *stream);

/* Ragged interpolation batches (auto_upsample: every batch has its own number of time points).  tab: DEVICE int32 [n][3], one row
 * per sample = {pair index into i0 / i1 / flow, row of tcoef [rows][6], output frame}; v2e_slomo_prep_tab / _fuse_tab do for
 * sample s exactly what v2e_slomo_prep / _fuse do for the sample of that pair and time row, x12 [n][12][h][w], out [n][1][h][w]. */
int v2e_slomo_prep_tab(const float *i0, const float *i1, const float *flow, const float *tcoef, const int32_t *tab, int n,
                       int h, int w, float *x12, void *stream);
int v2e_slomo_fuse_tab(const float *i0, const float *i1, const float *x12, const float *intrp, const float *tcoef,
                       const int32_t *tab, int n, int h, int w, float *out, void *stream);

/* ------------------------------------------- SloMo <-> emulator hand-off */

/*
 * Pillow-exact 8-bit resampling of n images [ih][iw] -> [oh][ow] (dataloader.py:142 LANCZOS,
 * slomo.py:439 BILINEAR).  Tables from v2e_amd/resample.py (libImaging/Resample.c
 * precompute_coeffs + normalize_coeffs_8bpc): bounds [out][2] = (first tap, taps), coef
 * [out][ksize] 22-bit fixed point.  tmp: device scratch [n][ih][ow] (horizontal pass output).
 */
int v2e_resample_u8(const uint8_t *in, uint8_t *tmp, uint8_t *out, int n, int ih, int iw, int oh, int ow,
                    const int32_t *hbounds, const int32_t *hcoef, int hksize, const int32_t *vbounds,
                    const int32_t *vcoef, int vksize, void *stream);

/* ToTensor + Normalize(mean, 1): out = in / 255 - mean (slomo.py:148-162) */
int v2e_u8_to_f32_norm(const uint8_t *in, float *out, int64_t n, float mean, void *stream);

/* revNormalize + ToPILImage: out = (uint8)(int)((in + mean) * 255) (slomo.py:437); reorder != 0:
 * in is [U][B][hw] (interpolation batch order), out is [B][U][hw] (time order, slomo.py:441) */
int v2e_f32_to_u8_trunc(const float *in, uint8_t *out, int U, int B, int hw, float mean, int reorder, void *stream);

/* the same conversion for the samples of a v2e_slomo_fuse_tab call: in [n][hw], sample s written to frame tab[s][2] of out */
int v2e_f32_to_u8_trunc_tab(const float *in, uint8_t *out, const int32_t *tab, int n, int hw, float mean, void *stream);

/* ------------------------------------------- stage-1 pre-processing (v2e.py:687-738) -- PARITY UNPINNED:
 * OpenCV 4.x's published INTER_AREA / BGR2GRAY 8-bit algorithms restated (see v2e_amd/csrc/preproc.hip); cv2 is in neither
 * tree nor this image, so the restatement has not been compared with cv2 itself. */

/* cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) of n uint8 images [sh][sw][cn] (cn = 1 or 3, interleaved), shrinking
 * only.  Integer scale factors: pass xofs = NULL (box sums).  Otherwise the tables of computeResizeAreaTab, grouped per
 * destination index (v2e_amd/preproc.py area_tab): entries [xofs[dx], xofs[dx + 1]) of (xsi, xalpha) feed column dx, in order;
 * the same for rows. */
int v2e_resize_area_u8(const uint8_t *src, uint8_t *dst, int n, int sh, int sw, int dh, int dw, int cn, const int32_t *xofs,
                       const int32_t *xsi, const float *xalpha, const int32_t *yofs, const int32_t *ysi, const float *yalpha, void *stream);
/* cv2.cvtColor(src, cv2.COLOR_BGR2GRAY) of npx interleaved BGR uint8 pixels.  gray_shift 15: OpenCV 4.x's RGB2Gray<uchar>
 * ((3735 B + 19235 G + 9798 R + 2^14) >> 15); 14: OpenCV 3.x's ((1868 B + 9617 G + 4899 R + 2^13) >> 14). */
int v2e_bgr2gray_u8(const uint8_t *src_bgr, uint8_t *dst, int64_t npx, int gray_shift, void *stream);

/* ----------------------------------------------------- event sinks */

/* AEDAT-2.0 records of aedat2_output.py:155-173: out_bytes gets n x 8 bytes (big-endian int32 address,
 * big-endian int32 timestamp in us).  Layout constants as set in aedat2_output.py:41-77 for the sensor
 * (346x260 / 240x180: xshift 12, yshift 22, pshift 11, flipx = flipy = 1; 640x480: 1, 11, 0).
 * noise_from >= 0: events [noise_from, n) get the special-event bit (label_signal_noise). */
int v2e_events_pack_aedat2(const float *events, void *out_bytes, int64_t n, int sizex, int sizey, int xshift,
                           int yshift, int pshift, int flipx, int flipy, int64_t noise_from, void *stream);

/* The same records for a whole run: frame f's rows start at recs[f].ev_offset (non-decreasing; a row belongs to the last
 * frame whose ev_offset is <= its index) and its first recs[f].n_signal rows are signal, the rest get the special-event bit.
 * recs: device array of nrec records (only ev_offset and n_signal are read); NULL: no labels. */
int v2e_events_pack_aedat2_run(const float *events, void *out_bytes, int64_t n, int sizex, int sizey, int xshift,
                               int yshift, int pshift, int flipx, int flipy, const v2e_frame_rec *recs, int nrec,
                               void *stream);

/* Text lines of ae_text_output.py:86-101, one per row in row order:
 *     t = (events[:, 0]).astype(np.float)              '{}'.format(t[i]): the shortest repr of the float64
 *     x = events[:, 1].astype(np.int32), y likewise    (no flips)
 *     p = ((events[:, 3] + 1) / 2).astype(np.int32)
 *     '{} {} {} {}\n'.format(t[i], x[i], y[i], p[i]), or with labels ' {}' int(signnoise_label[i]) before the '\n'
 * labels != 0: label 1 for a frame's first n_signal rows, 0 after them; the frames as for v2e_events_pack_aedat2_run (recs
 * on the device), or recs == NULL: one frame of n_signal signal rows.  scratch: device int64
 * [v2e_events_format_text_scratch_words(n)]; after the call scratch[0] is the text's length in bytes.  If that exceeds cap,
 * nothing is written to out (the caller grows the buffer and calls again).  n == 0: scratch[0] = 0, no launch. */
int v2e_events_format_text(const float *events, int64_t n, const v2e_frame_rec *recs, int nrec, int64_t n_signal,
                           int labels, char *out, int64_t cap, int64_t *scratch, void *stream);
int64_t v2e_events_format_text_scratch_words(int64_t n);
/* The same lines on the host, from the same __host__ __device__ code (v2e_amd/csrc/text_format.h): host rows and recs.
 * *total = the text's length; V2E_EOVERFLOW (nothing written) if it exceeds cap. */
int v2e_events_format_text_host(const float *events, int64_t n, const v2e_frame_rec *recs, int nrec, int64_t n_signal,
                                int labels, char *out, int64_t cap, int64_t *total);

/* ----------------------------------------------------- event readers: the sinks inverted (v2e_amd/csrc/readers.hip) */

/* items per workgroup of the readers' ordered compaction (records, and 16-byte pieces of text) */
#define V2E_READER_BLOCK 1024
/* counters of v2e_events_unpack_aedat2: device int64 [V2E_READER_COUNTERS], zeroed by the caller before a file's first call and
 * accumulated over its calls; CALL_ROWS is set by each call to the rows it wrote, LAST_TS / HAVE_LAST carry the last kept time
 * stamp to the next call so that a decreasing pair on a chunk boundary is counted. */
#define V2E_READER_COUNTERS 8
#define V2E_A2C_ROWS 0
#define V2E_A2C_APS 1
#define V2E_A2C_SPECIAL 2
#define V2E_A2C_OUTSIDE 3
#define V2E_A2C_NONMONOTONIC 4
#define V2E_A2C_LAST_TS 5
#define V2E_A2C_HAVE_LAST 6
#define V2E_A2C_CALL_ROWS 7
/* counters of v2e_events_parse_text (same rules): LINES every line seen; CALL_ROWS the rows this call wrote or -1 when the text
 * has more lines than cap_rows (then CALL_LINES says how many and nothing else changed); CALL_FLAGGED the entries of `flagged`. */
#define V2E_TXC_ROWS 0
#define V2E_TXC_COMMENT 1
#define V2E_TXC_BAD 2
#define V2E_TXC_FLAGGED 3
#define V2E_TXC_LINES 4
#define V2E_TXC_CALL_ROWS 5
#define V2E_TXC_CALL_LINES 6
#define V2E_TXC_CALL_FLAGGED 7

/* AEDAT-2.0 records back into rows, v2e_events_pack_aedat2 inverted: bytes holds n_records x 8 bytes (device, 8-byte aligned).
 * A record with address bit 31 (APS / IMU) is dropped and counted (APS).  Address bit 10 (special event): special_mode 0 drops
 * and counts it (SPECIAL: a jAER recording), 1 keeps it with labels[i] = 0 and 1 for every other row (a label_signal_noise file).
 * Where bit 10 lies inside the x, y or p field (the 640x480 layout keeps x in bits 1 .. 10) it is data: no record is special,
 * and special_mode 1 is refused.
 * x = (addr >> xshift) & mask, mask the bits that hold 0 .. sizex - 1, un-flipped when flipx; y likewise; p = +1 with the
 * polarity bit, else -1; t = (float)((double)ts * 1e-6); t_us[i] = ts (NULL: not wanted; labels likewise).  A row outside
 * [0,sizex) x [0,sizey) is kept and counted (OUTSIDE); a kept record whose ts is below the kept one before it is counted
 * (NONMONOTONIC).  Rows keep the records' order.  rows, labels, t_us: room for n_records rows (rows 16-byte aligned);
 * scratch: device bytes [v2e_events_unpack_aedat2_scratch_bytes(n_records)], 16-byte aligned. */
int v2e_events_unpack_aedat2(const void *bytes, int64_t n_records, int sizex, int sizey, int xshift, int yshift, int pshift,
                             int flipx, int flipy, int special_mode, float *rows, uint8_t *labels, int64_t *t_us,
                             int64_t *counters, void *scratch, void *stream);
int64_t v2e_events_unpack_aedat2_scratch_bytes(int64_t n_records);

/* Text lines back into rows, v2e_events_format_text inverted: bytes holds n_bytes of whole lines (device, 16-byte aligned); a
 * line ends at '\n' (a '\r' before it is dropped), a last line without one counts.  Grammar and the exact decimal -> float32
 * conversion of t (np.float32(float(s))): v2e_amd/csrc/text_parse.h.  Empty and '#' lines are counted (COMMENT), malformed
 * ones too (BAD); want_labels != 0: a fifth field 0 / 1 is required and goes to labels.  A time stamp outside the domain the
 * parser decides exactly (more than 19 significant digits, a decimal exponent outside +-62) still gives a row, with a best
 * effort t, and an entry flagged[2 j] = the line's byte offset, flagged[2 j + 1] = its row index of this call (device int64
 * [cap_flagged][2], in no particular order; CALL_FLAGGED may exceed cap_flagged, the entries beyond it are not written).
 * rows / labels: room for cap_rows rows; scratch: device bytes [v2e_events_parse_text_scratch_bytes(n_bytes, cap_rows)]. */
int v2e_events_parse_text(const char *bytes, int64_t n_bytes, int want_labels, float *rows, uint8_t *labels, int64_t cap_rows,
                          int64_t *counters, int64_t *flagged, int64_t cap_flagged, void *scratch, void *stream);
int64_t v2e_events_parse_text_scratch_bytes(int64_t n_bytes, int64_t cap_rows);
/* The same on the host, from the same __host__ __device__ code: host bytes, rows, labels, counters and flagged, a plain loop. */
int v2e_events_parse_text_host(const char *bytes, int64_t n_bytes, int want_labels, float *rows, uint8_t *labels,
                               int64_t cap_rows, int64_t *counters, int64_t *flagged, int64_t cap_flagged);

/* HDF5 "events" rows of emulator.py:955-965: uint32 [n][4] = (t*1e6 in float32, x, y, p with -1 -> 0) */
int v2e_events_pack_h5(const float *events, uint32_t *out, int64_t n, void *stream);

/* Lossless 8-byte wire format of an event row [t, x, y, p] (emulator.py:1024-1059 builds them as float32[4]):
 * bits 63..32 the float32 bits of t, 31..18 x, 17..4 y, bit 0 (p > 0); x, y < 16384.  Used by the multi-GPU
 * all-gather of the event streams (half the bytes over xGMI); unpack restores the float32 rows exactly.
 * Domain: x and y integer values in [0, 16384), p = +-1 (any p > 0 is restored as +1, any other as -1); t may be any float32,
 * NaN payloads and -0.0 included.  There is no flag channel: a coordinate outside the domain (negative, fractional, NaN, 16384
 * or more) gives an unspecified word, and the caller must not send such rows. */
int v2e_events_pack64(const float *events, uint64_t *out, int64_t n, void *stream);
int v2e_events_unpack64(const uint64_t *in, float *events, int64_t n, void *stream);

/* Lossless 4-byte wire format for sensors up to 2048 x 1024: the rows of a run come in blocks of one time stamp (all events
 * of one (frame, iteration) share it: emulator.py:793-796, 861-870), so t travels once per block.  payload[i] = x | y << 11
 * | (p > 0) << 21; runs[0] = number of blocks R in its low 32 bits (never more than cap_runs) and the overflow flags below in
 * bits 62 (coordinate) and 63 (table too small), so that a receiver of the table sees them too; runs[1 + r] = float32 bits of t << 32 | index of the block's first event
 * (in order).  cap_runs: entries the run table holds besides runs[0] (a bound is sum over frames of max(iterations, 1));
 * scratch: device uint32 [v2e_events_pack32_scratch_words(n)], scratch[0] after the call: bit 0 a coordinate did not fit,
 * bit 1 the run table was too small (the caller then sends pack64).  unpack32 restores the float32 rows bit for bit.
 * A coordinate "does not fit" iff x is not an integer value in [0, 2048) or y is not one in [0, 1024): negative, fractional, NaN
 * and infinite coordinates raise the flag like 2048 / 1024 and beyond (-0.0 is the integer 0 and is restored as +0.0).  The payload
 * word of such a row is unspecified; the host refuses a flagged table.  Blocks split on the BITS of t: -0.0 and +0.0, or two NaNs
 * with different payloads, are different time stamps; two NaNs with the same bits are one. */
int v2e_events_pack32(const float *events, int64_t n, uint32_t *payload, uint64_t *runs, int64_t cap_runs,
                      uint32_t *scratch, void *stream);
int64_t v2e_events_pack32_scratch_words(int64_t n);
int v2e_events_unpack32(const uint32_t *payload, int64_t n, const uint64_t *runs, float *events, void *stream);

/* EventRenderer.accumulate_event_frame (renderer.py:368-400, hist2d_numba_seq v2e_utils.py:474-486):
 * current_frame (float64 [bins_y][bins_x], device) = clip(current_frame + hist(ON) - hist(OFF), +-full_scale).
 * scratch_diff: device int32 [bins_y][bins_x], zero on entry, left zero. */
int v2e_events_accumulate_frame(const float *events, int64_t n, double *current_frame, int32_t *scratch_diff,
                                int bins_y, int bins_x, double y_lo, double y_hi, double x_lo, double x_hi,
                                double full_scale, void *stream);

/* Finished DVS frame in 0..1: (current_frame + full_scale) / (2 full_scale) in float64 (renderer.py:245-247, normalize_frame). */
int v2e_frame_normalize(const double *current_frame, double *out, int n, double full_scale, void *stream);

/* EventRenderer.render_events_to_frames on a device-resident packet (renderer.py:161-366; v2e_amd/csrc/render.hip).
 * v2e_render_area_segments: the AREA_COUNT windows of a packet of n events (renderer.py:253-266, 292-298): area_counts
 * (device int32 [nw][nh], carried from packet to packet, updated), seg_end[k] = end index (exclusive) of complete window k
 * (the event that filled a cell; it opens the next window and is counted again there), out2[0] = number of complete windows,
 * out2[1] = 1 if the walk ended on a trigger at the packet's last event. */
int v2e_render_area_segments(const float *events, int64_t n, int32_t *area_counts, int nw, int nh, double area_dimension,
                             int area_count, int32_t *seg_end, int64_t cap, int32_t *out2, void *stream);
/* v2e_render_packet: every event i < n_used (= n - 1: the packet's last event is never accumulated, renderer.py:303-306)
 * goes into the frame(s) of its exposure window -- mode 1 DURATION: bounds[0..n_bounds) the frame start times T_k, frame k =
 * [T_k, T_k+1] (both ends inclusive, as searchsorted left / right), the open frame from T_{n_bounds-1}; 2 COUNT: frame
 * i / count_per_frame; 3 AREA_COUNT: seg_end[0..n_seg); 4 SOURCE: frame 0 -- as hist(ON) - hist(OFF) over bins_y x bins_x bins
 * (hist2d_numba_seq, v2e_utils.py:474-486).  frames_out [n_complete][bins_y][bins_x] float64 = (clip(+-full_scale) +
 * full_scale) / (2 full_scale) (renderer.py:245-247, 396-400); cur_out (if has_open) = the clipped, un-normalised frame the
 * packet ends in.  diff: device int32 scratch [(n_complete + has_open)][bins_y * bins_x]. */
int v2e_render_packet(const float *events, int64_t n_used, int mode, const double *bounds, int n_bounds,
                      int64_t count_per_frame, const int32_t *seg_end, int n_seg, int n_complete, int has_open, int32_t *diff,
                      double *frames_out, double *cur_out, int bins_y, int bins_x, double y_lo, double y_hi, double x_lo,
                      double x_hi, double full_scale, void *stream);

/* EventRenderer.render_run: a whole device-resident run in one pass (v2e_amd/csrc/render.hip).  The run is events[n_rows][4]
 * plus a packet table pkt_off[0..n_packets] (device int64, strictly increasing from 0: packet p = rows [pkt_off[p],
 * pkt_off[p + 1]), the packets v2e.py:837-850 hands render_events_to_frames); every packet is rendered as the reference
 * renders it on its own (renderer.py:271 resets the running frame, :296-306 leaves the packet's last event out, the frame a
 * packet ends in is not emitted), its complete frames numbered across the run from pkt_frame0[p] on (device int32
 * [n_packets + 1], the last entry the run's total).
 * v2e_render_run_windows: DURATION (renderer.py:207-213, 314-318).  One lane walks the packets in order, advancing the frame
 * start time with separate additions -- float32 additions of (float)interval if f32_time (numpy >= 2 keeps the time stamp's
 * float32 through `+= frameIntevalS`), float64 ones otherwise -- while the packet's second-to-last time stamp lies past the next
 * frame's start.  time_state: device double[3], {currentFrameStartTime, 1.0 once it is set}, carried from run to run and written
 * only if commit, and [2] = the start time after this run, written always (the host's copy).  Writes pkt_frame0, packet p's start times T_0 .. T_m to bounds[pkt_frame0[p] + p ...] (needs total +
 * n_packets entries) and every complete frame's time, the start after the increment plus interval / 2 (renderer.py:350), to
 * frame_times; both may be null with a capacity of 0 (the counting pass).  out2[0] = complete frames, out2[1] = 1: the interval
 * does not advance the time, 2: more than max_frames frames. */
int v2e_render_run_windows(const float *events, const int64_t *pkt_off, int n_packets, double interval, int f32_time,
                           double *time_state, int commit, int32_t *pkt_frame0, double *bounds, int64_t cap_bounds,
                           double *frame_times, int64_t cap_times, int64_t max_frames, int32_t *out2, void *stream);
/* v2e_render_run_area_segments: v2e_render_area_segments over all packets of the run in one launch (renderer.py:253-266,
 * 292-298), area_counts carried across the packets; seg_end[pkt_frame0[p] + k] = end (exclusive, within packet p) of its
 * complete window k, out2[0] = complete windows of the run (more than cap: seg_end was too small), out2[1] as above for the
 * last packet. */
int v2e_render_run_area_segments(const float *events, const int64_t *pkt_off, int n_packets, int32_t *area_counts, int nw, int nh,
                                 double area_dimension, int area_count, int32_t *seg_end, int64_t cap, int32_t *pkt_frame0,
                                 int32_t *out2, void *stream);
/* v2e_render_run_frame_times: the time of every complete frame (renderer.py:343-349) -- mode 4 SOURCE: the packet's ts[0];
 * 2 COUNT, 3 AREA_COUNT: (ts[start] + ts[end]) / 2 of the frame's window, a float32 sum -- as float64 [n_frames]. */
int v2e_render_run_frame_times(const float *events, const int64_t *pkt_off, int n_packets, int mode, int64_t count_per_frame,
                               const int32_t *seg_end, const int32_t *pkt_frame0, int n_frames, double *frame_times, void *stream);
/* v2e_render_run: one histogram launch for the run -- every event finds its packet (binary search over pkt_off), its window
 * by v2e_render_packet's rule and adds +-1 to the int32 plane of its global frame -- and one launch that clips and normalises:
 * frames_out float64 [n_complete][bins_y][bins_x] in 0..1, or frames_u8_out, the bytes (img * 255).astype(uint8) the reference
 * hands its AVI writer (renderer.py:339); cur_out (if has_open) = the clipped frame the LAST packet ends in.  want_frames 0:
 * only cur_out.  diff: device int32 scratch [(want_frames ? n_complete : 0) + has_open][bins_y * bins_x]. */
int v2e_render_run(const float *events, int64_t n_rows, const int64_t *pkt_off, int n_packets, int mode, const double *bounds,
                   int64_t count_per_frame, const int32_t *seg_end, const int32_t *pkt_frame0, int n_complete, int has_open,
                   int want_frames, int32_t *diff, double *frames_out, uint8_t *frames_u8_out, double *cur_out, int bins_y,
                   int bins_x, double y_lo, double y_hi, double x_lo, double x_hi, double full_scale, void *stream);

/* The reference's synthetic input sources (v2e.py:580-612, --synthetic_input=scripts.<name>) rendered on the device
 * (v2e_amd/csrc/synth.hip; host side v2e_amd/synthetic.py).  Every entry writes a block of n consecutive frames into the
 * caller's device buffer out[n][H][W] in one launch and nothing outside it; all arithmetic is float64 in the reference's
 * order of operations.
 * v2e_synth_dots: scripts/moving_dot.py:26-54, 156-183 and scripts/particles.py:187-197, 213-241 (fill_dot over a background
 * frame).  Frame f draws the dots offs[f] .. offs[f + 1] (device int32 [n + 1], from 0) in list order: centres (device
 * float64 [dots][2]: x, y) and boxes (device int32 [dots][2]: x0, y0, the rounded centre as the host's Python round() gave
 * it).  A pixel in [x0 - d, x0 + d) x [y0 - d, y0 + d) becomes bg + (fg - bg) * v, v = peak * exp(-dist2 / (sigma * sigma))
 * with dist2 from the float centre, v > 1 -> 1, else v < low_cut -> 0 (moving_dot.py:44-49: peak 10, low_cut .01;
 * particles.py:236-240: peak 2, no low cut: pass a negative one); clip != 0 clamps the result to 0..255 (moving_dot.py:50-53).
 * Where boxes overlap the dot later in the list wins, as in the reference's sequential loop; a pixel no box covers is bg; a
 * box is clipped at the frame edge (particles.py:232).  out_dtype: V2E_DT_U8 (the C conversion numpy applies when a double is
 * stored into a uint8 array), V2E_DT_F32 (particles' float32 frame) or V2E_DT_F64. */
int v2e_synth_dots(const double *centres, const int32_t *boxes, const int32_t *offs, int n, int H, int W, void *out, int out_dtype,
                   double bg, double fg, double sigma, int d, double peak, double low_cut, int clip, void *stream);
/* v2e_synth_gradients: gradients.im_function (scripts/gradients.py:117-140) as uint8.  p: device float64 [n], the bump centre
 * of every frame (gradients.py:125; p2 = p + w2 * 2 follows from it); low, high, slope = -diff / w2 and w2 are the call's
 * constants as the host computes them (gradients.py:121-124).  The three masked assignments are applied in the reference's order. */
int v2e_synth_gradients(const double *p, int n, int H, int W, uint8_t *out, double low, double high, double slope, double w2,
                        void *stream);
/* v2e_synth_barberpole: barberpole.bb_func (scripts/barberpole.py:155-163) inside the pole mask, bg outside
 * (barberpole.py:85-98, 139-140).  t: device float64 [n], the frame times.  Pole pixels (minx < x < maxx and miny < y < maxy,
 * strict) are uint8(floor(low + diff * 0.5 * (1 + tanh(10 * sin(two_pi * (y - tan_a * x - t * speed) / wavelength))))). */
int v2e_synth_barberpole(const double *t, int n, int H, int W, uint8_t *out, double low, double diff, double tan_a, double speed,
                         double two_pi, double wavelength, int minx, int maxx, int miny, int maxy, int bg, void *stream);

/* Dense event tensors from the rows of a device-resident run (v2e_amd/csrc/tensorize.hip; host side v2e_amd/tensors.py,
 * EventTensorizer).  Rows are events[n][4] = (t, x = column, y = row, p = +-1), in any order.  Window k of the clip is [B_k, B_k+1) in
 * float64 with the float32 t widened: B_k = t_start + (double)k * window_s (bounds null), or the ascending device table
 * bounds[] (then bounds[0] is the start of the launch's first window and nk + 1 entries are read).  A launch covers the nk
 * windows from clip index k0 on; with has_open the last of them is the clip's open window, whose planes are the carried *_open
 * buffers; the planes of the complete windows lie in count / voxel_acc / surf_keys.  Every update is a no-return integer atomic, so
 * the result does not depend on the order of the rows.
 * v2e_tensorize_scatter: one pass over the rows; each representation is enabled by its *_open pointer.  count: int32 [.,2,H,W]
 * (channel 0 OFF, 1 ON), += 1.  voxel: int64 [.,voxel_bins,H,W] in units of 2^-24: tau = (bins - 1) * ((t - B_k) / (B_k+1 - B_k)),
 * b0 = floor(tau), q1 = llrint((tau - b0) * 2^24), q0 = 2^24 - q1; p * q0 is added to bin b0 and, when q1 != 0, p * q1 to bin
 * b0 + 1; voxel_acc holds only the complete windows v_a .. v_b - 1 (launch-local), the others are skipped.  surface: uint32
 * [.,2,H,W], the maximum of an order-preserving key of t (0 = none).  A row with x outside [0,W), y outside [0,H), a fractional
 * coordinate, p other than +-1 or a NaN t is written nowhere and counted in counters[0] (n_bad); a row before the launch's first
 * window in counters[1] (n_before), at or after its last bound in counters[2] (n_after); counters (device uint64 [3]) may be null.
 * events must be 16-byte aligned. */
int v2e_tensorize_scatter(const float *events, int64_t n, int H, int W, double t_start, double window_s, const double *bounds,
                          int64_t k0, int nk, int has_open, int32_t *count, int32_t *count_open, int64_t *voxel_acc,
                          int64_t *voxel_open, int v_a, int v_b, int voxel_bins, uint32_t *surf_keys, uint32_t *surf_open,
                          uint64_t *counters, void *stream);
/* v2e_tensorize_move_zero: 32-bit words; dst[0 .. n_words) = carry[0 .. n_carry_words) followed by zeros, then carry = 0 (the
 * plane of the window that was open becomes the first plane of the output).  16-byte stores where dst, carry and the counts allow. */
int v2e_tensorize_move_zero(void *dst, int64_t n_words, void *carry, int64_t n_carry_words, void *stream);
/* v2e_tensorize_voxel_finish: out[i] = (float)((double)acc[i] * 2^-24), i < n; clear != 0 zeroes acc behind the read. */
int v2e_tensorize_voxel_finish(int64_t *acc, int64_t n, float *out, int clear, void *stream);
/* v2e_tensorize_surface_finish: in place on planes [n_planes][plane_words] of keys: the running maximum over the planes, starting
 * from state[plane_words] (keys; a pixel without an event holds the key of -inf), decoded to the float32 time stamp; state = the
 * maximum after the last plane. */
int v2e_tensorize_surface_finish(void *planes, int n_planes, int64_t plane_words, uint32_t *state, void *stream);

/* Event counts of one clip for many thresholds in one pass (v2e_amd/csrc/sweep.hip; host side v2e_amd/sweep.py, ThresholdSweep).
 * Replaces the reference's threshold searches, which run the whole clip through one emulator per threshold:
 * dataset_scripts/ddd/ddd_find_thresholds.py:120-155 (reset, generate_events per frame, select_events_in_roi, count the polarities;
 * 95 thresholds) and v2ecore/thres_estimator.py (all of v2e.py per threshold).
 * Column j is the emulator EventEmulator(pos_thres = pos[j], neg_thres = neg[j], rng_mode = "philox", shot_noise_rate_hz = 0) with
 * the model parameters of *p, fresh, given the F frames one by one (clip 0; the first frame initialises it and emits nothing; the
 * state is float64 when cutoff_hz > 0, float32 otherwise).  counts_dev[j] = { ON, OFF } events with roi[0] <= x <= roi[1] and
 * roi[2] <= y <= roi[3] (inclusive, v2e_utils.select_events_in_roi) -- exact while the refractory rule (emulator.py:830) never
 * switches on in column j.  The kernel runs every column as if the rule were off; rule_on_dev[j] = 1 says that it would have
 * switched on in some frame, and that the column's counts are to be recomputed with the emulator itself.
 * frames: device uint8 [F][H][W] (frame_dtype must be V2E_DT_U8); t_frames: host, F strictly increasing times, t_frames[0] >= 0;
 * pos, neg: host, T positive thresholds; counts_dev (uint64 [T][2]) and rule_on_dev (int32 [T]) are device buffers of the caller's,
 * overwritten.  The library's only scratch of its own is the table of per-frame scalars and thresholds, uploaded from host memory
 * by the call (which is therefore not for stream capture).  Everything is enqueued on `stream`.  V2E_EINVAL for another frame type, F < 2, T < 1, an empty or out-of-sensor ROI, times that do not increase, a
 * threshold that is not positive. */
typedef struct v2e_sweep_params {
    double sigma_thres;
    double cutoff_hz;
    double leak_rate_hz;
    double leak_jitter_fraction;
    double noise_rate_cov_decades;
    double refractory_period_s;
    uint64_t seed;
    int32_t cols_per_thread; /* columns a thread carries in registers: 0 (the library's default), 4, 8 or 16 */
    int32_t reserved_;       /* 0 */
} v2e_sweep_params;
int v2e_thres_sweep(const void *frames, int frame_dtype, int F, int H, int W, const double *t_frames, const v2e_sweep_params *p,
                    const double *pos, const double *neg, int T, const int roi[4], uint64_t *counts_dev, int32_t *rule_on_dev,
                    void *stream);
/* v2e_thres_sweep_chunk: the same sweep for a clip that arrives in chunks: the call runs v2e_thres_sweep's per-frame arithmetic
 * over the F >= 1 frames of one chunk, whose first frame is the clip's frame frame0, and carries every column's state from call to
 * call in device planes of the caller's: lp [H*W] of R (the same for every column) and base [T][H*W] of R, R = double when
 * cutoff_hz > 0 and float otherwise.  The state at the start of the chunk is read from lp_in / base_in and the state behind its
 * last frame is written to lp_out / base_out, which must be other planes: the kernel never writes what it reads, so the state at
 * the start of the chunk is still there when the chunk's flags are known.  frame0 == 0: frames[0] is the clip's first frame, which
 * initialises the state and emits nothing; lp_in / base_in are not read (and may be null) and t_previous must be 0.  frame0 > 0:
 * every frame is an ordinary one, and t_previous is the emulator's t_previous when it is given frames[0]: the time of the clip's
 * frame frame0 - 1, except that it is 0 for frame0 == 1 (the first frame does not advance it, emulator.py:717); t_frames[0] must
 * lie after it.  The Philox keys use the clip's frame index frame0 + f, whichever half of a frame pair the chunk begins on.
 * counts_dev is ADDED to and rule_on_dev OR-ed into -- zero both before the clip's first chunk -- so that after the last chunk they
 * hold what v2e_thres_sweep gives for the whole clip, bit for bit, in every column whose flag is 0.  A pixel's own 32-bit ON / OFF
 * total is per chunk.  Same model parameters, thresholds and ROI in every call of a clip; everything else as for v2e_thres_sweep
 * (V2E_EINVAL also for F < 1, frame0 < 0 or frame0 + F >= 2^31, a null or aliased state plane). */
int v2e_thres_sweep_chunk(const void *frames, int frame_dtype, int F, int H, int W, const double *t_frames, int64_t frame0,
                          double t_previous, const v2e_sweep_params *p, const double *pos, const double *neg, int T, const int roi[4],
                          const void *lp_in, const void *base_in, void *lp_out, void *base_out, uint64_t *counts_dev,
                          int32_t *rule_on_dev, void *stream);
/* v2e_thres_sweep_info: the kernel a sweep with this state type / kind of thresholds / cols_per_thread runs: the columns per
 * thread in force, its vector registers per lane, and how many of its 256-thread workgroups a CU holds.  Outputs may be null. */
int v2e_thres_sweep_info(int f64_state, int scalar_thres, int cols_per_thread, int *cols_out, int *vgprs, int *workgroups_per_cu);
/* v2e_thres_sweep_chunk_info: the same of the kernel v2e_thres_sweep_chunk runs (the instantiation that carries the state). */
int v2e_thres_sweep_chunk_info(int f64_state, int scalar_thres, int cols_per_thread, int *cols_out, int *vgprs, int *workgroups_per_cu);

/* The spatio-temporal correlation filter (STCF; with one supporting neighbour jAER's BackgroundActivityFilter) scored for every
 * (k, tau) in one pass over the rows of a device-resident run (v2e_amd/csrc/denoise.hip; host side v2e_amd/denoise.py,
 * DenoiseSweep).  Rows are events[n][4] = (t, x = column, y = row, p), processed in row order; p is not read.  A row is bad if t is
 * not finite or x / y is not an integer value inside [0,W) / [0,H): it reads and writes nothing, enters no histogram, is counted
 * and gets keep = 0.  For a valid row i at pixel (x, y), each of the 8 neighbours q inside the sensor (centre excluded) gives
 * age_q = (double)t_i - (double)T_q, T_q the t of the latest row j < i at q in this pass, else the carried last_t[q] (float32
 * [H][W], -inf where no row has been yet); a neighbour outside the sensor or T_q = -inf gives +inf, a T_q later than t_i a negative
 * age, kept as it is.  With a_1 <= ... <= a_8 the sorted ages, the row passes STCF(k, tau) iff a_k <= tau; after its ages are read
 * the row sets last_t[x,y] = t_i whatever the filters say.  taus: device float64 [n_taus], 1 <= n_taus <= 256, finite, >= 0,
 * strictly ascending (the caller checks); bin(a) = the number of taus strictly below a (bin n_taus: passes none), and
 * hist[k-1][label][bin(a_k)] += 1 for k = 1 .. 8, hist a device uint64 [8][2][n_taus+1], label 1 = signal, 0 = noise.  All sums are
 * integer atomics: the result depends on the row order only, not on scheduling, and a clip cut into passes gives the same sums.
 * One pass (n <= 2^31 - 1 rows, H * W <= 2^31 - 1) is four calls with a sort of the keys between the first and the second:
 * v2e_denoise_keys: keys[i] = pixel << 32 | i, or 0x7fffffffffffffff for a bad row (sorts last as int64); keep (uint8 [n] or null)
 * gets 0 at bad rows.
 * v2e_denoise_segments: sorted_keys = keys in ascending order; seg (int32 [H*W+1]): pixel p's rows are sorted_keys[seg[p] ..
 * seg[p+1]), seg[H*W] = the number of valid rows; counters (device uint64 [2] or null): [0] += valid rows, [1] += bad rows.
 * v2e_denoise_ages: ages, histogram and, with keep != null, keep[i] = (a_keep_k <= keep_tau) for every valid row.  The label of row
 * i is labels[i] != 0 (uint8 [n]), or, with label_bounds (ascending int64 row indices of the whole call, this pass's row 0 having
 * index row0: frame f's signal rows start at label_bounds[2f], its noise rows at label_bounds[2f+1]), signal iff an odd number
 * of entries is <= row0 + i; with neither every row is signal.  last_t is only read.
 * v2e_denoise_map_update: last_t[p] = the t of pixel p's last row of the pass; behind v2e_denoise_ages on the same stream.
 * events must be 16-byte aligned. */
int v2e_denoise_keys(const float *events, int64_t n, int H, int W, int64_t *keys, uint8_t *keep, void *stream);
int v2e_denoise_segments(const int64_t *sorted_keys, int64_t n, int H, int W, int32_t *seg, uint64_t *counters, void *stream);
int v2e_denoise_ages(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                     const double *taus, int n_taus, const uint8_t *labels, const int64_t *label_bounds, int n_label_bounds,
                     int64_t row0, uint64_t *hist, uint8_t *keep, int keep_k, double keep_tau, void *stream);
int v2e_denoise_map_update(const float *events, const int64_t *sorted_keys, const int32_t *seg, int H, int W, float *last_t,
                           void *stream);

/* Per-event time-surface patches: for every row of a device-resident run the (2r+1) x (2r+1) patch of ages and polarities around
 * it, as the maps were just before the row (v2e_amd/csrc/patches.hip; host side v2e_amd/patches.py, EventPatches).
 * Rows and validity: rows are events[n][4] = (t, x = column, y = row, p), taken in row order.  A row is bad under exactly
 * DenoiseSweep's rule: t not finite, or x / y not an integer value inside [0,W) / [0,H); p is not examined for validity.  A bad row
 * reads and writes no map and gets valid = 0; its features are the "none" values below.
 * Carried maps: last_t is float32 [H][W] and starts at -inf; last_p is int8 [H][W] and starts at 0; both are carried on the device
 * from call to call.
 * Per-row patch: for a valid row i at (x, y) and every offset (dy, dx) in [-r, r]^2, r = 1, 2 or 3, the centre included, the patch
 * index is [dy + r][dx + r].  Let q = (x + dx, y + dy).  If q is outside the sensor the entry is none.  Otherwise T_q and P_q are
 * taken from the latest valid row j < i at q in this call: T_q is its t, P_q the sign of its p (+1 if p > 0, else -1).  If no such
 * row exists in this call, the carried maps supply T_q and P_q; a carried T_q of -inf means none.  age = (double)t_i - (double)T_q;
 * a T_q later than t_i gives a negative age, which is kept.  The centre entry is the previous event at the same pixel: the row is
 * never in its own patch.
 * After reading, the row stamps last_t[y][x] = t_i and last_p[y][x] = sign(p_i).
 * Output: out is float32 [n][2][P][P], P = 2r + 1.  mode 0 ("age"): channel 0 is (float)age, rounded to nearest even, +inf where
 * none; channel 1 is P_q as +-1.0, 0 where none.  mode 1 ("linear", tau > 0 finite): channel 0 is 0 where none or age >= tau, 1
 * where age <= 0, otherwise (float)(1 - age / tau), the division and the subtraction each rounded in float64; channel 1 is P_q
 * where channel 0's entry is not of the first kind, that is, not none and age < tau, otherwise 0.
 * Invariance: the result depends on the row order alone; a clip cut into several calls, or a call cut into passes, gives identical
 * features and identical final maps.
 * One pass (n <= 2^31 - 1 rows, H * W <= 2^31 - 1) is v2e_denoise_keys, a sort of the keys, v2e_denoise_segments, then:
 * v2e_patches_features: writes EVERY element of out[n][2][P][P] and valid[n] (uint8), bad rows included, whatever the buffers held;
 * the maps are only read.  Per entry one binary search of q's stretch of the sorted keys for the largest row index below i and one
 * 16-byte gather of that row.  Element offsets into out are 64-bit.  events must be 16-byte aligned.
 * v2e_patches_map_update: last_t[p], last_p[p] from pixel p's last row of the pass; behind v2e_patches_features on the same stream. */
int v2e_patches_features(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                         const int8_t *last_p, int radius, int mode, double tau, float *out, uint8_t *valid, void *stream);
int v2e_patches_map_update(const float *events, const int64_t *sorted_keys, const int32_t *seg, int H, int W, float *last_t, int8_t *last_p,
                           void *stream);

/* A learned patch filter in one pass: the patch of v2e_patches_features in mode 1 ("linear") gathered, a one-hidden-layer MLP
 * evaluated on it and one float32 score per row written, with no feature in global memory (v2e_amd/csrc/mlpf.hip; host side
 * v2e_amd/mlpf.py, MLPFilter).
 * Rows, validity, carried maps and the per-row patch are exactly v2e_patches_features' with mode 1 and the same tau (finite, > 0).
 * The input of row i is its patch flattened as [2][P][P], P = 2 * radius + 1: x[c * P * P + (dy + r) * P + (dx + r)], K = 2 * P * P
 * entries (18, 50 or 98), all finite.
 * Network: w1 float32 [hidden][K], b1 [hidden], w2 [hidden], b2 [1], device arrays, 1 <= hidden <= 64, all finite (the caller checks).
 * Arithmetic: a_j = (double)b1[j]; for k = 0 .. K-1 ascending a_j = a_j + (double)w1[j][k] * (double)x[k] (the product of two
 * float32 values is exact in float64, so each step is one float64 rounding, with or without an fma).  h_j = (float)a_j, rounded to
 * nearest even; h_j = h_j > 0 ? h_j : 0, so a NaN becomes 0.  s = (double)b2; for j ascending s = s + (double)w2[j] * (double)h_j;
 * scores[i] = (float)s.  No transcendental: the score is the logit.
 * valid[i] (uint8) = 1 for a valid row; a bad row gets valid 0, the quiet NaN 0x7fc00000 as its score and mask 0.
 * mask_or_null (uint8 [n]): mask[i] = valid[i] && (double)scores[i] >= threshold (threshold not NaN).
 * Writes EVERY element of scores[n], valid[n] and mask[n]; the maps are only read.  One pass (n <= 2^31 - 1 rows, H * W <= 2^31 - 1)
 * is v2e_denoise_keys, a sort of the keys, v2e_denoise_segments, this call, then v2e_patches_map_update on the same stream.
 * events must be 16-byte aligned.  Bad arguments return V2E_EINVAL before anything is launched. */
int v2e_patches_mlp_scores(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                           const int8_t *last_p, int radius, double tau, const float *w1, const float *b1, int hidden, const float *w2,
                           const float *b2, float *scores, uint8_t *valid, double threshold, uint8_t *mask_or_null, void *stream);

/* A stream's own statistics: per-pixel counts, same-pixel inter-event intervals and time-bin counts of the rows of device-resident
 * runs (v2e_amd/csrc/stats.hip; host side v2e_amd/stats.py, EventStats).
 * Rows and validity: rows are events[n][4] = (t, x = column, y = row, p), taken in row order; a row is bad under exactly
 * DenoiseSweep's rule, is counted by v2e_denoise_segments and touches nothing.  A valid row is ON iff p > 0; its label is
 * v2e_denoise_ages' (labels, or label_bounds with row0, or neither: signal).  With c = 2 * label + ON:
 * count (uint64 [4][H][W]): count[c][y][x] += 1 for every valid row.  Everything else takes the valid rows inside the ROI
 * x0 <= x <= x1, y0 <= y <= y1 only:
 * the previous event of row i is the latest valid row j < i at its pixel in this pass, else the carried last_t (float32 [H][W],
 * starts at -inf: none) / last_p (int8 [H][W], +-1, starts at 0).  None: sums[c] += 1 (n_first).  Otherwise
 * d = (double)t_i - (double)T_prev, tr = 2 * (previous ON) + ON, isi_hist[label][tr][the number of isi_edges <= d] += 1 (uint64
 * [2][4][n_edges+1]; 1 to 256 edges, ascending: the caller checks); d < 0: sums[4 + label] += 1 (n_backwards); d >= 0:
 * sums[8 + 4 * label + tr] = the unsigned minimum of itself and d's bit pattern (min_isi; the caller starts it at +inf's bits).
 * time_bounds (n_bins + 1 ascending doubles, 1 <= n_bins <= 2^20; or null with n_bins 0): k = (the number of bounds <= (double)t)
 * - 1; time_hist[c][k] += 1 (uint64 [4][n_bins]) for 0 <= k < n_bins, else sums[6] += 1 (before) or sums[7] += 1 (after).
 * sums[16] / sums[17]: the minimum / maximum over ALL valid rows of key(t), key(v) = bits ^ 0xffffffff for a negative float32,
 * bits | 0x80000000 otherwise (the caller starts them at 0xffffffff / 0).  sums is uint64 [18].
 * isi_hist and time_hist are given as isi_replicas / time_replicas (1 to 2048) copies of those shapes, all zero at the start; workgroup
 * b of the kernel adds to copy b % replicas and the histogram is the sum of the copies (one copy of a small table is one contended
 * atomic per row).
 * Integer atomics only: the result depends on the row order alone.
 * One pass (n <= 2^31 - 1 rows, H * W <= 2^31 - 1) is v2e_denoise_keys, a sort of the keys, v2e_denoise_segments, then:
 * v2e_stats_rows: all sums; the maps are only read.  events must be 16-byte aligned.
 * v2e_stats_map_update: last_t[p], last_p[p] from pixel p's last row of the pass; behind v2e_stats_rows on the same stream. */
int v2e_stats_rows(const float *events, int64_t n, int H, int W, const int64_t *sorted_keys, const int32_t *seg, const float *last_t,
                   const int8_t *last_p, int x0, int x1, int y0, int y1, const double *isi_edges, int n_edges, const double *time_bounds,
                   int n_bins, const uint8_t *labels, const int64_t *label_bounds, int n_label_bounds, int64_t row0, uint64_t *count,
                   uint64_t *isi_hist, int isi_replicas, uint64_t *time_hist, int time_replicas, uint64_t *sums, void *stream);
int v2e_stats_map_update(const float *events, const int64_t *sorted_keys, const int32_t *seg, int H, int W, float *last_t, int8_t *last_p,
                         void *stream);

/* The fixed-window filter (FWF of the DND21 denoising benchmark) scored for every (L, sigma, k) in one pass over the rows of a
 * device-resident run (v2e_amd/csrc/window.hip; host side v2e_amd/window.py, WindowSweep).
 * Rows and validity: rows are events[n][4] = (t, x = column, y = row, p), taken in row order; neither p nor the value of t is used.
 * A row is bad under exactly DenoiseSweep's rule: it is counted, never enters the window, enters no histogram and gets keep = 0.
 * The stream: the valid rows of all passes, v_0, v_1, ...; the window of v_m is v_{m-1} (depth 1) ... v_{m-D}, D = min(m, lmax),
 * lmax the longest length of the table.  For a sigma and k = 1 .. 4, d = the smallest depth j at which k of the rows at depth
 * 1 .. j have |x - x'| + |y - y'| <= sigma (a row at the same pixel counts), lmax + 1 if the window holds fewer.  The row passes
 * FWF(L, sigma, k) iff d <= L: with bin(d) = the number of lengths strictly below d (bin n_lengths: passes none),
 * hist[k-1][s][label][bin(d)] += 1, hist a device uint64 [4][n_sigmas][2][n_lengths+1], label 1 = signal, 0 = noise.  After its
 * depths are read the row enters the window whatever any filter says.  All sums are integer atomics: the result depends on the row
 * order only, and a clip cut into passes gives the same sums.
 * A row of the stream is the word x | y << 16; 0xffffffff is "no row yet" (H, W <= 65535 leave it free).  tail (device uint32
 * [lmax]) carries the last lmax words from pass to pass, the latest last, and starts as lmax words 0xffffffff.
 * One pass (1 <= n <= 2^30 rows) is three calls on one stream; no call waits for the device or learns the number of valid rows:
 * v2e_window_compact: xy (uint32 [lmax + n]) = the tail, then the words of the pass's valid rows in order; idx (int32 [n]): the
 * row of the pass behind each of those words; n_valid (int32 [1]) = their number; blk: scratch, int32 [(n + 255) / 256]; both
 * counters (device uint64 [2], the call's and the sweep's): [0] += valid rows, [1] += bad rows; keep (uint8 [n] or null) gets 0 at
 * bad rows.  events must be 16-byte aligned.
 * v2e_window_depths: depths, histogram and, with keep != null, keep[i] = (d <= keep_length) for every valid row, d taken for
 * keep_sigma (any value >= 0) and keep_k (1 .. 4), keep_length in 1 .. lmax; none of the three has to be a table entry.  lengths:
 * device int32 [n_lengths], 1 <= n_lengths <= 64, strictly ascending, 1 <= L <= 1024, the last one lmax (the caller checks);
 * sigmas: HOST int32 [n_sigmas], 1 <= n_sigmas <= 8, strictly ascending, 0 .. 65535.  Labels as for v2e_denoise_ages.
 * v2e_window_tail: tail = the last lmax words of xy; behind v2e_window_depths on the same stream. */
int v2e_window_compact(const float *events, int64_t n, int H, int W, const uint32_t *tail, int lmax, uint32_t *xy, int32_t *idx,
                       int32_t *blk, int32_t *n_valid, uint64_t *call_counters, uint64_t *seen_counters, uint8_t *keep, void *stream);
int v2e_window_depths(const uint32_t *xy, const int32_t *idx, int64_t n, const int32_t *n_valid, const int32_t *lengths, int n_lengths,
                      int lmax, const int32_t *sigmas, int n_sigmas, const uint8_t *labels, const int64_t *label_bounds,
                      int n_label_bounds, int64_t row0, uint64_t *hist, uint8_t *keep, int keep_length, int64_t keep_sigma, int keep_k,
                      void *stream);
int v2e_window_tail(const uint32_t *xy, const int32_t *n_valid, int64_t n, int lmax, uint32_t *tail, void *stream);

/* The double-window filter (DWF of the same benchmark, jAER's DoubleWindowFilter) scored for every (L, sigma, k) of three tables
 * (v2e_amd/csrc/dwindow.hip; host side v2e_amd/dwindow.py, DoubleWindowSweep).  Rows, validity and the packed words are the
 * fixed-window filter's.  A setting owns two windows R and N of at most L rows each, empty at first; a valid row passes iff at
 * least k rows of R and N together lie within L1 distance sigma of it (the same pixel counts); a passing row is appended to R, a
 * failing one to N, and a window that now holds L + 1 rows drops its oldest.  Setting f = (ki * n_sigmas + si) * n_lengths + li.
 * State between passes: rings (device uint32 [F][2][lmax], lmax the longest length: window R of setting f is a ring of L slots
 * at rings[f][0][0 .. L), N at rings[f][1][0 .. L); 0xffffffff in a slot without a row and in every slot from L on: the start
 * value of all of it), pos (device int32 [F][2], zero at first: the slot the window's next row goes to, which holds its oldest
 * row once it is full) and passed (device uint64 [F][2]: passing noise rows, passing signal rows).
 * One pass (1 <= n <= 2^30 rows) is three calls on one stream, none of which waits for the device:
 * v2e_window_compact with lmax = 1 and a one-word tail: xy (uint32 [1 + n]), idx, n_valid as described there.
 * v2e_dwindow_labels: lab (uint8 [n]) = the label of each of the pass's valid rows, in their order, from labels (a byte per row of
 * the pass) or label_bounds (as for v2e_denoise_ages) or neither (all signal); totals (device uint64 [2]): [0] += valid noise
 * rows, [1] += valid signal rows.
 * v2e_dwindow_sweep: one wavefront per setting walks the pass's valid rows in order and updates rings, pos and passed; with
 * keep != null, keep[i] = the verdict of the setting (lengths[keep_length], sigmas[keep_sigma], supports[keep_support]) -- the three
 * are INDICES into the tables -- for every valid row i.  lengths, sigmas, supports: HOST int32 tables, strictly ascending, 1 to 64
 * lengths in 1 .. 512, 1 to 8 sigmas in 0 .. 65535, 1 to 4 supports in 1 .. 4. */
int v2e_dwindow_labels(const int32_t *idx, int64_t n, const int32_t *n_valid, const uint8_t *labels, const int64_t *label_bounds,
                       int n_label_bounds, int64_t row0, uint8_t *lab, uint64_t *totals, void *stream);
int v2e_dwindow_sweep(const uint32_t *xy, const int32_t *idx, const uint8_t *lab, int64_t n, const int32_t *n_valid, const int32_t *lengths,
                      int n_lengths, const int32_t *sigmas, int n_sigmas, const int32_t *supports, int n_supports, uint32_t *rings,
                      int32_t *pos, uint64_t *passed, uint8_t *keep, int keep_length, int keep_sigma, int keep_support, void *stream);

/* ------------------------------------------------------------- diagnostics */
/* include/v2e_detmath.h evaluated on the device, an array at a time (v2e_amd/csrc/detmath_eval.hip): what tests/test_detmath_gpu.py
 * compares with the CPU oracle's loops over the same header.  Nothing in the product path calls it.
 * All arrays are device arrays of 32-bit words; a float travels as its bit pattern.  Element i of n (n <= 2^26):
 *   fn                       a                                   b                                    out0 (out1)
 *   V2E_DM_PHILOX, _KS       [n][4] counter                      [2] key                              [n][4] words
 *   V2E_DM_LOGF, _EXPF       [n] x                               -                                    [n] f(x)
 *   V2E_DM_SINCOS2PI         [n] u                               -                                    [n] sine ([n] cosine)
 *   V2E_DM_NORMAL2           [n] word a                          [n] word b                           [n] cosine branch ([n] sine)
 *   V2E_DM_SLEEF_SINHF       [n] x                               -                                    [n] sinh(x)
 *   V2E_DM_PERM_APPLY, _INVERT [n] index < b[0]                  [6] n, seed low, high, clip, frame, iteration   [n] image
 *   V2E_DM_NTH_SET_BIT_256   [n][8] mask, low word first         [n] r < popcount                     [n] position
 *   V2E_DM_TS_FORMULA        [n][4] i, count, start, end         [n] step                             [n] timestamp
 *   V2E_DM_DRAW_PAIR, _KS    [n] pixel                           [5] seed low, high, clip, pair, want_normal   [n][4] randn_odd, u_odd, randn_even, u_even
 *   V2E_DM_DRAW_FRAME        [n] pixel                           [4] seed low, high, clip, frame      [n] leak normal ([n] shot uniform)
 *   V2E_DM_DRAW_PNOISE       [n] pixel                           [4] seed low, high, clip, frame      [n] normal
 *   V2E_DM_DRAW_INIT         [n] pixel                           [3] seed low, high, clip             [n][4] v2e_draw_init's n_pos, n_neg, n_rate, then v2e_draw_scidvs */
enum {
    V2E_DM_PHILOX = 0, V2E_DM_PHILOX_KS, V2E_DM_LOGF, V2E_DM_EXPF, V2E_DM_SINCOS2PI, V2E_DM_NORMAL2, V2E_DM_SLEEF_SINHF,
    V2E_DM_PERM_APPLY, V2E_DM_PERM_INVERT, V2E_DM_NTH_SET_BIT_256, V2E_DM_TS_FORMULA, V2E_DM_DRAW_PAIR, V2E_DM_DRAW_PAIR_KS,
    V2E_DM_DRAW_FRAME, V2E_DM_DRAW_PNOISE, V2E_DM_DRAW_INIT, V2E_DM_COUNT
};
int v2e_detmath_eval(int fn, const uint32_t *a, const uint32_t *b, uint32_t *out0, uint32_t *out1, int64_t n, void *stream);

/* The streaming passes a UNet forward runs between its convolutions, one at a time (v2e_amd/csrc/slomo_stream.h): what
 * tests/test_slomo_stream_gpu.py compares with the CPU oracle bit for bit.  Nothing in the product path calls it.  Device arrays:
 *   V2E_SS_AVGPOOL2, _UPSAMPLE2   x [nc][2h][2w] resp. [nc][h/2][w/2] (h, w even) -> float y [nc][h][w], through the launchers of
 *                                 v2e_unet_forward: four outputs per thread when w is a multiple of 4, else one
 *   ..._SCALAR                    the one-output-per-thread kernels at any width
 *   V2E_SS_AMAX                   x [nc * h * w] -> uint32 y [1]: the range slot of the network input, RAISED to the bits of the
 *                                 largest |x| (a NaN counts as 0x7fc00000); the caller preloads it
 * V2E_EINVAL before anything is launched for a null pointer, a size that is not positive, an odd upsampling target or another op. */
enum { V2E_SS_AVGPOOL2 = 0, V2E_SS_AVGPOOL2_SCALAR, V2E_SS_UPSAMPLE2, V2E_SS_UPSAMPLE2_SCALAR, V2E_SS_AMAX };
int v2e_slomo_stream_eval(int op, const float *x, void *y, int64_t nc, int h, int w, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* V2E_AMD_H */
