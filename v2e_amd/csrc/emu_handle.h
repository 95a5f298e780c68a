// emu_handle.h -- the emulator handle (v2e_emu), its per-run scratch sets, and what every entry point of emu.hip does first:
// kernel arguments from handle + parameters, the parameter check.  Included by emu.hip only, after its kernels.
// Everything a pipelined run's head (upload, zero fills, first records), its chain and its last emission batches touch while the run
// before / after it is still in flight: the handle holds two sets (v2e_emu::sets).  Not here: the pixel state and its ping-pong set,
// the checkpoints -- only the chain touches them, and chains never overlap.
struct RunScratch {
    FrameCtl *run_ctl = nullptr;                // device [run_cap][n_clips]
    uint32_t *run_fidx = nullptr;               // device: frame_idx0 of the run
    const void **run_frames = nullptr;          // device: the run's frames (k_ahead / k_chain read the pointer from here)
    unsigned long long **stamp_slot = nullptr;  // device: the run's slot of launch stamps (nullptr: off), read by k_chain
    unsigned long long *run_off = nullptr;      // [run_off_cap][n_clips] event offset at the start of every emission batch of the run
    // sized by the chain configuration (K, E, keys; v2e_emu::ch_*)
    uint32_t *ch_gM = nullptr;      // [ch_launch_cap][ch_K + 1][n_clips][ch_K]
    unsigned *ch_bar = nullptr;     // [ch_launch_cap][2 ch_K][n_clips]: one counter per rendezvous of a launch (passes + lock-step frames)
    uint32_t *ch_rec = nullptr;     // [ch_D][n_clips][npx_pad] k_ahead's per-(frame, pixel) records (4 bytes: see AheadArgs)
    uint4 *ch_msk = nullptr;        // [ch_D][n_clips][npx_pad / 64] k_ahead's per-(frame, wave) shot masks (see AheadArgs)
    ccnt_t *ch_cnt = nullptr;       // [ch_D][n_clips][npx_pad] the chain's 16-bit count words (CCNT_*, emu_kernels.h)
    uint32_t *ch_ruleM = nullptr;   // [ch_D][n_clips]
    float *ch_tsold = nullptr;      // [ch_D][n_clips][npx_pad] (refractory runs)
    uint16_t *ch_wmax = nullptr;    // [3][ch_E][n_clips][ch_nwp]
    uint16_t *ch_wtot = nullptr;    // [3][ch_E][n_clips][nkeys_cap][ch_nwp]
    CFrame *ch_cf = nullptr;        // [3][ch_E][n_clips]
    unsigned *ch_cdone = nullptr;   // [3][ch_E][n_clips] k_cframe's per-frame completion counters
    uint32_t *ch_cT = nullptr, *ch_ckbase = nullptr, *ch_cperm = nullptr, *ch_cpre = nullptr;
    uint32_t *ch_cmask = nullptr;   // the pull's per-(group, key) pixel ballots (CEmitArgs::cmask), three sets like the other tables
    uint32_t *ch_cpre16 = nullptr;  // every 16th entry of ch_cpre (CEmitArgs::cpre16)
    // what the chain configuration sizes
    template <typename T> static void drop(T *&b) { hipFree((void *)b); b = nullptr; }
    void free_chain()
    {
        drop(ch_gM); drop(ch_bar); drop(ch_rec); drop(ch_msk); drop(ch_cnt); drop(ch_ruleM); drop(ch_tsold); drop(ch_wmax); drop(ch_wtot);
        drop(ch_cf); drop(ch_cdone); drop(ch_cT); drop(ch_ckbase); drop(ch_cperm); drop(ch_cpre); drop(ch_cmask); drop(ch_cpre16);
    }
    void free_all()
    {
        free_chain();
        drop(run_ctl); drop(run_fidx); drop(run_frames); drop(stamp_slot); drop(run_off);
    }
};

// A pinned host buffer mapped into the device's address space: kernels read / write it in place through `dev` (v2e_emu_frame's
// staging: no copy engine on the way in or out).
struct PinnedBuf {
    unsigned char *host = nullptr, *dev = nullptr;
    size_t cap = 0; // bytes
    // at least `bytes`, the first `keep_bytes` of what it held kept; the caller has made sure that nothing on the device still uses it
    int grow(size_t bytes, size_t keep_bytes = 0)
    {
        if (bytes <= cap) return 0;
        if (keep_bytes == 0) release(); // (nothing to keep: never two buffers at once)
        unsigned char *grown = nullptr, *grown_dev = nullptr;
        V2E_HIP(hipHostMalloc((void **)&grown, bytes, hipHostMallocMapped)); // (on failure what was to be kept stays as it is)
        if (hipError_t e = hipHostGetDevicePointer((void **)&grown_dev, grown, 0)) { hipHostFree(grown); V2E_HIP(e); }
        if (host) memcpy(grown, host, keep_bytes);
        release();
        host = grown; dev = grown_dev; cap = bytes;
        return 0;
    }
    void release() { if (host) hipHostFree(host); host = dev = nullptr; cap = 0; }
};

struct v2e_emu {
    // ---- geometry
    int H, W, n_clips, max_iters, device;
    int npx, nwaves, nkeys_cap;
    long long npx_pad;
    int ngroups = 0, n_cu = 256;
    // ---- bound state planes (v2e_emu_bind_state)
    void *lp = nullptr, *base = nullptr;
    float *ts_mem = nullptr, *pos_thres = nullptr, *neg_thres = nullptr, *noise_rate = nullptr;
    // ---- per-frame scratch, look-up tables and rings
    uint32_t *cnt = nullptr, *hist = nullptr, *tot = nullptr;
    float *lut_L = nullptr;
    double *lut_I = nullptr;
    v2e_frame_rec *rec_ring = nullptr; // [RING][n_clips]
    FrameCtl *ctl_ring = nullptr;      // [RING][n_clips]
    FrameCtl *ctl_host = nullptr;      // pinned staging [RING][n_clips]
    unsigned long long *off_dev = nullptr, *off_host = nullptr; // [n_clips] explicit event offsets
    unsigned long long *off_zero = nullptr; // [n_clips] zeros
    // ---- v2e_emu_frame staging (one call per frame): pinned staging of a host frame (read by k_count in place), device scratch
    // [v2e_frame_rec | FrameCtl], pinned record (v2e_frame_rec + nkeys_cap totals) and rows (written by k_frame_rows_to_host)
    PinnedBuf fr_stage, fr_rec_host, fr_ev_host;
    unsigned char *fr_dev = nullptr;
    unsigned char *fr_par = nullptr, *fr_par_dev = nullptr; // the frame's FrameCtl, pinned
    int fr_flip = 0;                                        // which of the two frame records this call counts into
    float *fr_user_rows = nullptr, *fr_user_rows_dev = nullptr; // v2e_emu_frame_host_rows: the next frame's rows go here
    uint64_t fr_user_cap = 0, fr_est = 0;
    uint64_t fr_ev_rows() const { return fr_ev_host.cap / (4 * sizeof(float)); } // rows fr_ev_host holds
    // ---- model extensions (pnoise / SCIDVS / CSDVS / probes)
    void *pn_arr = nullptr;           // photoreceptor_noise_arr plane (v2e_emu_set_pnoise)
    const float *pn_tape = nullptr;
    void *sc_hp = nullptr, *sc_prev = nullptr; // SCIDVS planes (v2e_emu_set_scidvs)
    float *sc_tau = nullptr;
    uint32_t sc_first_frame = 0;
    const void *cs_sur = nullptr;              // CSDVS surround plane (v2e_emu_set_csdvs)
    // CSDVS in a device-resident run (v2e_emu_set_csdvs_run): per-frame Euler parameters, scratch planes, step slots
    void *csr_scratch = nullptr, *csr_lp = nullptr;
    std::vector<double> csr_ap, csr_ah;
    std::vector<int> csr_steps;
    double csr_thr = 0.0;
    int *csr_steps_dev = nullptr;
    unsigned long long *csr_slots = nullptr;
    int csr_slots_cap = 0;
    double *dbg_lognew = nullptr, *dbg_cms = nullptr, *dbg_diff = nullptr; // v2e_emu_set_model_state_planes
    // v2e_emu_set_probes: what the next run records (probe_next: consumed by v2e_emu_run into probe_run, the run being enqueued),
    // model-state planes of the library's own for callers that bound none, the row pass's counters [n_frames][P][2] + ticket
    V2EProbeSet probe_next = {0, {0}}, probe_run = {0, {0}};
    double *probe_next_out = nullptr, *probe_out = nullptr;
    double *probe_planes = nullptr;
    unsigned int *probe_cnt = nullptr;
    size_t probe_cnt_cap = 0;
    // ---- run staging (multi-frame run)
    FrameCtl *run_ctl_host2[2] = {nullptr, nullptr}; // pinned staging, two sets
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    int run_stage = 0, run_cap = 0;
    uint32_t *run_fidx_host = nullptr;      // pinned, two slots (the staging of RunScratch::run_fidx)
    const void **run_frames_host = nullptr; // pinned, two slots
    int run_off_cap = 0;
    // the two scratch sets of pipelined runs: a pipelined run flips scratch_par and takes the other set than the run before it; every
    // other run uses the current one.  A set's buffers are allocated while it is current, when a run first needs them.
    RunScratch sets[2];
    int scratch_par = 0;
    RunScratch &cur() { return sets[scratch_par]; }
    const RunScratch &cur() const { return sets[scratch_par]; }
    // ---- chain configuration: K-frames-per-launch chain (emu_chain.h); allocated on first use by v2e_emu_run
    int ch_ring_pref = 0; // ring depth in batches, chosen by the handle's first device-resident run (chain_ring_batches)
    int ch_K = 0, ch_D = 0, ch_nD = 3, ch_nwp = 0, ch_launch_cap = 0, ch_max_blocks = 0, ch_fused = -1, ch_inst = -1;
    int ch_E = 0;                   // frames per k_ahead launch / emission batch (a multiple of ch_K)
    int ch_long_batches = -1;      // large grids: 64-frame emission batches (1) or max(K, 8) (0: the ring would not fit); -1: not decided yet
    int ch_nkeys_cap = 0;           // nkeys_cap the chain scratch was sized for
    int ch_pull = 0;                // the event writer of this configuration: k_cpull (1) or k_cemit
    void *ch_ck = nullptr;          // refractory runs: 2 launch parities x (K / 8 - 1) checkpoints x (base 8 B, lp 8 B, ts 4 B) planes
    void *ch_base2 = nullptr, *ch_lp2 = nullptr; // second set of state planes (ping-pong between launches)
    float *ch_ts2 = nullptr;
    int occ_cache[32];              // workgroups of a k_chain instantiation a CU holds (-1: not queried yet)
    // what the chain configuration sizes, in both sets
    void free_chain_scratch()
    {
        sets[0].free_chain(); sets[1].free_chain();
        hipFree(ch_ck); ch_ck = nullptr;
    }
    // ---- streams and events
    hipStream_t side = nullptr;        // the event writer of the chain: k_cemit
    hipStream_t side2 = nullptr;    // the event writer of the odd batches (two batches' rows are written side by side)
    hipStream_t ahead = nullptr;    // k_ahead runs beside the chain and the emission
    hipStream_t tabs = nullptr;     // the emission tables (k_ctot, k_cframe, k_coff) of batch b + 1 beside the event writer on batch b
    std::vector<hipStream_t> spare_streams; // candidates the queue probe did not give a role (destroyed with the handle)
    hipStream_t probed_for = nullptr;       // the caller's stream the pipelined roles were last probed against
    bool probed = false;
    std::vector<hipEvent_t> ev_fork, ev_join;
    std::vector<hipEvent_t> ev_ahead, ev_chain, ev_tab;
    // ---- pipelined-run bookkeeping: runs in flight, events of the pieces
    hipEvent_t ev_main_done2[2] = {nullptr, nullptr}, ev_tail_done2[2] = {nullptr, nullptr};
    bool piece_pending[2] = {false, false}; // set `par` has a run whose pieces may still be executing
    const void *last_events = nullptr, *last_recs = nullptr; // buffers of the pipelined run enqueued last
    hipEvent_t ev_user = nullptr;
    void *recs_host[2] = {nullptr, nullptr}; // pinned: the records of the last pipelined run per scratch set (v2e_emu_run_recs)
    size_t recs_host_cap[2] = {0, 0}, recs_host_n[2] = {0, 0};
    int last_ticket = -1; // the scratch set of the run enqueued last if it went out in pieces, else -1 (v2e_emu_run_ticket)
    // every piece of every pipelined run has completed (host-blocking; before scratch is freed or re-sized)
    void sync_runs()
    {
        for (int q = 0; q < 2; ++q)
            if (piece_pending[q]) { if (ev_tail_done2[q]) hipEventSynchronize(ev_tail_done2[q]); if (ev_main_done2[q]) hipEventSynchronize(ev_main_done2[q]); piece_pending[q] = false; }
    }
    // `s` waits for every piece of every pipelined run enqueued so far (no host block)
    int join_runs(hipStream_t s)
    {
        for (int q = 0; q < 2; ++q)
            if (piece_pending[q]) {
                if (hipStreamWaitEvent(s, ev_main_done2[q], 0) != hipSuccess || hipStreamWaitEvent(s, ev_tail_done2[q], 0) != hipSuccess) return -1;
            }
        return 0;
    }
    // ---- graphs: captured runs, keyed by everything baked into them (buffers, sizes, parameters): a caller that alternates between
    // two sets of frame / event / record buffers (the asynchronous API) replays two graphs
    struct CachedGraph { std::vector<unsigned char> key; hipGraphExec_t exec; unsigned long long used; int ops[3]; };
    std::vector<CachedGraph> graphs;
    unsigned long long graph_clock = 0;
    void drop_graphs()
    {
        for (auto &g : graphs) hipGraphExecDestroy(g.exec);
        graphs.clear();
    }
    // ---- profiling and dev tools
    double prof_ms[4] = {0, 0, 0, 0}; // count, rank, scan, emit (V2E_RUN_PROFILE)
    int prof_launches = 0;
    std::vector<float> prof_chain_us; // the chain launches of the last instrumented run, one by one
    int prof_emit_batches = 0, prof_step_launches = 0;
    int last_kind = -1, last_fpl = 0, last_fpb = 0; // v2e_emu_last_pipeline
    int last_queue_ops[3] = {0, 0, 0}; // launches, waits, records the last k_chain run put on the caller's stream (v2e_emu_last_run_queue_ops)
    int ch_last_launches = 0;      // chain launches of the last run with a refractory period (their rule-on rows: v2e_emu_debug_chain_rows), 0 otherwise
    // per-launch device time stamps of the chain kernel (v2e_emu_launch_stamps): [runs_cap][STAMP_LAUNCHES][2] wall-clock words
    unsigned long long *stamps = nullptr;
    int stamps_runs = 0;                       // runs the buffer holds (0: off)
    unsigned long long stamp_seq = 0;          // runs stamped so far
    unsigned long long **stamp_slot_host = nullptr; // pinned, two slots
    unsigned long long *dbg = nullptr; // dev tool (v2e_emu_debug_timeline)
};

static thread_local char g_err[512] = "";

void v2e_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// pinned host staging -> device (v2e_emu_run): the run's frame times, from which the frame scalars (FrameCtl: the reference's Python
// doubles, the per-iteration-count timestamp tables, the refractory switch) are computed HERE, one thread per frame -- the same IEEE
// operations as on the host (make_ctl is one function for both; device float64 / float32 division is correctly rounded, and
// -ffp-contract=off holds for this file): 64 divisions per frame were ~100 us of host time per 300-frame run, on the path that
// bounds the pipelined loop -- and its first frame index, frames' address and stamp slot
static __global__ __launch_bounds__(BLOCK) void k_upload_ctl(const double *__restrict__ tp, const double *__restrict__ tf, FrameCtl *__restrict__ dst, size_t nct,
                                                      double cutoff_hz, double shot_rate_hz, double refr_s,
                                                      const uint32_t *__restrict__ fsrc, uint32_t *__restrict__ fdst,
                                                      const void *const *__restrict__ psrc, const void **__restrict__ pdst,
                                                      unsigned long long *const *__restrict__ ssrc, unsigned long long **__restrict__ sdst)
{
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < nct; i += (size_t)gridDim.x * BLOCK) dst[i] = make_ctl(tp[i], tf[i], cutoff_hz, shot_rate_hz, refr_s);
    if (blockIdx.x == 0 && threadIdx.x == 0) { *fdst = *fsrc; *pdst = *psrc; *sdst = *ssrc; }
    // the run's slot of per-launch time stamps (v2e_emu_launch_stamps; nullptr: off) starts out zero
    unsigned long long *slot = *ssrc;
    if (slot && blockIdx.x == 0)
        for (int i = threadIdx.x; i < 2 * STAMP_LAUNCHES; i += BLOCK) slot[i] = 0ull;
}

static KArgs make_kargs(const v2e_emu *h, const v2e_emu_params *p)
{
    KArgs a;
    memset(&a, 0, sizeof(a));
    a.W = h->W; a.npx = h->npx; a.nwaves = h->nwaves; a.nkeys_cap = h->nkeys_cap; a.max_iters = h->max_iters;
    a.npx_pad = h->npx_pad;
    a.scalar_thres = p->scalar_thres; a.rng_mode = p->rng_mode; a.shuffle = p->shuffle;
    a.do_leak = p->leak_rate_hz > 0; a.do_shot = p->shot_noise_rate_hz > 0;
    a.has_cutoff = p->cutoff_hz > 0; a.has_refr = p->refractory_period_s > 0;
    a.use_inten = a.has_cutoff || a.do_shot;
    a.log_input = p->log_input != 0;
    a.cutoff_two_pi = M_PI * 2 * p->cutoff_hz;
    a.pos_div = p->pos_thres_scalar; a.neg_div = p->neg_thres_scalar;
    a.pos_nom_f = (float)p->pos_thres_nominal; a.neg_nom_f = (float)p->neg_thres_nominal;
    a.pos_pre_scalar = p->pos_pre_scalar; a.neg_pre_scalar = p->neg_pre_scalar;
    a.leak_hz_f = (float)p->leak_rate_hz; a.jit_f = (float)p->leak_jitter_fraction;
    a.sigma_f = (float)p->sigma_thres;
    a.pos_mean_f = (float)p->pos_thres_scalar; a.neg_mean_f = (float)p->neg_thres_scalar;
    a.ln10cov_f = (float)(log(10.0) * p->noise_rate_cov_decades);
    a.shot_half_rate = p->shot_noise_rate_hz / 2;
    a.inten_slope = p->shot_noise_inten_factor - 1;
    a.refr = p->refractory_period_s; a.refr_f = (float)p->refractory_period_s;
    a.seed = p->seed;
    a.lp = h->lp; a.base = h->base; a.ts_mem = h->ts_mem;
    a.pos_thres = h->pos_thres; a.neg_thres = h->neg_thres; a.noise_rate = h->noise_rate;
    a.cnt = h->cnt; a.hist = h->hist; a.tot = h->tot;
    a.lut_L = h->lut_L; a.lut_I = h->lut_I;
    if (p->photoreceptor_noise) { a.pn_arr = h->pn_arr; a.pn_tape = h->pn_tape; a.pn_vrms_f = (float)p->photoreceptor_noise_vrms; }
    a.cs_sur = h->cs_sur;
    if (h->sc_hp) { a.sc_hp = h->sc_hp; a.sc_prev = h->sc_prev; a.sc_tau = h->sc_tau; a.sc_first_frame = h->sc_first_frame; }
    a.dbg_lognew = h->dbg_lognew; a.dbg_cms = h->dbg_cms; a.dbg_diff = h->dbg_diff;
    return a;
}

static int check_params(const v2e_emu *h, const v2e_emu_params *p)
{
    V2E_REQUIRE(h && p, "null handle/params");
    V2E_REQUIRE(h->lp && h->base && h->pos_thres && h->neg_thres, "state not bound (v2e_emu_bind_state)");
    V2E_REQUIRE((p->f64_state != 0) == (p->cutoff_hz > 0 || p->log_input != 0), "f64_state must equal (cutoff_hz > 0 || log_input)");
    V2E_REQUIRE(!(p->leak_rate_hz > 0) || h->noise_rate, "leak enabled but noise_rate plane not bound");
    V2E_REQUIRE(!(p->refractory_period_s > 0) || h->ts_mem, "refractory enabled but ts_mem plane not bound");
    return 0;
}

// the small helpers of the entry points are inlined into them whatever the optimiser thinks: the frame-at-a-time API is host-bound
#define V2E_INLINE inline __attribute__((always_inline))

static V2E_INLINE size_t dtype_size(int dtype) { return dtype == V2E_DT_U8 ? 1 : (dtype == V2E_DT_F32 ? 4 : 8); } // bytes of a frame element

// a frame's slot of the control / record ring of the frame-at-a-time API
static V2E_INLINE FrameCtl *ctl_slot(const v2e_emu *h, uint32_t frame_idx) { return h->ctl_ring + (size_t)(frame_idx % RING) * h->n_clips; }
static V2E_INLINE v2e_frame_rec *rec_slot(const v2e_emu *h, uint32_t frame_idx) { return h->rec_ring + (size_t)(frame_idx % RING) * h->n_clips; }

// What an entry point that enqueues on the caller's stream begins with: the stream waits for the pieces of the pipelined runs in
// flight (join_pending), then the parameter check (enter).  The entry point's own checks and hipSetDevice follow, in that order.
static V2E_INLINE int join_pending(v2e_emu *h, void *stream)
{
    if (h && (h->piece_pending[0] || h->piece_pending[1]) && h->join_runs((hipStream_t)stream)) { v2e_set_error("hipStreamWaitEvent failed"); return V2E_EHIP; }
    return 0;
}
static V2E_INLINE int enter(v2e_emu *h, const v2e_emu_params *p, void *stream)
{
    const int rc = join_pending(h, stream);
    return rc ? rc : check_params(h, p);
}
