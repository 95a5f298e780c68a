// emu_chain_host.h -- host side of the chain pipeline (kernels: emu_chain.h): the launch schedule, the scratch it needs, the enqueue of
// one run, and the probe that tells which of the handle's streams share a hardware queue.  Included by emu.hip only, after enqueue_run.
// ------------------------------------------------------------------ launch scheduling of the chain pipeline
// The run is a DAG over logical streams (chain, k_ahead, emission tables, event rows) with cross edges between them, enqueued on
// HIP streams with events -- under stream capture for a graph run (edges between the origin stream and a forked stream only:
// hipStreamEndCapture of a capture with edges between two forked streams segfaults on this runtime, ROCm 7.0 / HIP 7.0.5).
enum { ST_MAIN = 0, ST_AHEAD = 1, ST_SIDE = 2, ST_TAB = 3, ST_SIDE2 = 4, ST_COUNT = 5 };
enum { EV_FORK = 0, EV_JOIN = 1, EV_AHEAD = 2, EV_CHAIN = 3, EV_TAB = 4 };

// a logical stream -> its HIP stream; an (event kind, index) -> the handle's HIP event
struct Sched {
    v2e_emu *h;
    hipStream_t st[ST_COUNT];
    // Pipelined runs: an event that would be recorded on the chain's stream right behind a chain launch is that launch's STOP EVENT
    // instead (hipExtLaunchKernel: bound to the kernel's own dispatch, no packet of its own in the queue); where several events
    // follow one launch, one is the stop event and stands in for the others this run (stand_in: their waiters wait for it).
    struct StandIn { int kind, idx; hipEvent_t ev; };
    std::vector<StandIn> stand_in;
    int ops[3] = {0, 0, 0}; // launches, waits, records this run put on ST_MAIN (v2e_emu_last_run_queue_ops)

    hipEvent_t real_event(int kind, int idx) const
    {
        for (const StandIn &a : stand_in) if (a.kind == kind && a.idx == idx) return a.ev;
        switch (kind) {
        case EV_FORK: return h->ev_fork[idx];
        case EV_JOIN: return h->ev_join[idx];
        case EV_AHEAD: return h->ev_ahead[idx];
        case EV_CHAIN: return h->ev_chain[idx];
        default: return h->ev_tab[idx];
        }
    }
    int kernel(int s, const void *fn, dim3 grid, dim3 block, size_t lds, void **args, hipEvent_t stop = nullptr)
    {
        if (stop) V2E_HIP(hipExtLaunchKernel(fn, grid, block, args, lds, st[s], nullptr, stop, 0));
        else V2E_HIP(hipLaunchKernel(fn, grid, block, args, lds, st[s]));
        ops[0] += s == ST_MAIN;
        return 0;
    }
    int zero4(int s, void *const ptr[4], const size_t bytes[4])
    {
        ZeroRanges z;
        unsigned long long tot = 0;
        for (int r = 0; r < 4; ++r) { z.p[r] = (uint32_t *)ptr[r]; z.n[r] = ptr[r] ? (bytes[r] + 3) / 4 : 0; tot += z.n[r]; }
        if (tot == 0) return 0;
        void *args[] = {(void *)&z};
        return kernel(s, (const void *)k_zero_ranges, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, args);
    }
    int record(int kind, int idx, int s)
    {
        V2E_HIP(hipEventRecord(real_event(kind, idx), st[s]));
        ops[2] += s == ST_MAIN;
        return 0;
    }
    int wait(int s, int kind, int idx)
    {
        V2E_HIP(hipStreamWaitEvent(st[s], real_event(kind, idx), 0));
        ops[1] += s == ST_MAIN;
        return 0;
    }
};

// ------------------------------------------------------------------ K frames per launch (emu_chain.h)
static int chain_egroups(const v2e_emu *h) { return (h->npx + GROUP_PX - 1) / GROUP_PX; }
static bool chain_small_grid(const v2e_emu *h) { return (long long)h->ngroups * h->n_clips <= 2ll * h->n_cu; }

// Batches in the ring of frame slots.  Three is the minimum (batch b is read by its emission while the chain is in batch b + 1 and
// k_ahead fills batch b + 2); the chain then waits for the emission of batch b - 3 where the ring wraps.  One hipGraph per run runs
// SLOWER with a deeper ring (round 3: 8.5 Gev/s with 3 batches, 7.3 with 5 or 7; round 6: 787 -> 904 us per step with 5), 64 clips
// and 1280x720 do not care (14.5-14.6 / 11.9-12.1 Gev/s either way) -- but PIPELINED runs of a small grid, whose k_ahead runs a whole
// run ahead and whose event rows have a stream of their own, gain from never waiting inside a 300-frame run: ring 3 681-685 us per
// step, 4 668-671, 5 662-664, 6 657-673, 8 671 (profiles/r06_emulator_experiments.txt item 21).  A handle keeps the depth its FIRST
// device-resident run chose (no re-allocation when a caller mixes modes).  V2E_AMD_CHAIN_RING=3..8 overrides that choice (dev / tests:
// a pipelined 300-frame run in a ring of three batches wraps, so its chain and k_ahead wait for one another batch by batch).
static int chain_ring_batches(v2e_emu *h, bool pipelined)
{
    if (h->ch_ring_pref == 0) {
        h->ch_ring_pref = (pipelined && chain_small_grid(h) && h->n_clips == 1) ? 5 : 3;
        if (const char *ev = getenv("V2E_AMD_CHAIN_RING")) { const int v = atoi(ev); if (v >= 3 && v <= 8) h->ch_ring_pref = v; }
    }
    return h->ch_ring_pref;
}

// records built inside the chain (large grids) or by k_ahead (small grids); V2E_AMD_CHAIN_FUSED=0/1 overrides (dev / tests)
static bool chain_fused_records(const v2e_emu *h, int dtype, int nD)
{
    if (dtype != V2E_DT_U8) return true; // k_ahead's record path is instantiated for uint8 frames only
    // k_chain reads k_ahead's records and writes the count words through buffer resources (32-bit offsets): the record ring of
    // nD batches of up to 64 frames must stay below 4 GB (beyond that the chain builds the records).  The same bound covers the
    // smaller planes (count words, shot masks) and the frames of one launch, which the chain reads the pixel bytes from at
    // k * frame_stride, k < K <= 64, frame_stride = n_clips * npx bytes.
    if ((size_t)nD * 64 * h->n_clips * h->npx_pad * sizeof(uint32_t) >= (1ull << 32)) return true;
    const char *fe = getenv("V2E_AMD_CHAIN_FUSED"); // read per call: tests switch it per emulator instance
    const int fused_env = fe ? atoi(fe) : -1;
    return fused_env >= 0 ? fused_env != 0 : !chain_small_grid(h);
}

// k_chain on k_ahead's records decodes them through per-launch tables (emu_chain.h, CHAIN_TAB_MAX) wherever a launch's frames take few
// enough distinct dt_over_tau values; V2E_AMD_CHAIN_TABLES=0 keeps the record-by-record decode for every launch (A/B runs, tests)
static bool chain_decode_tables()
{
    const char *e = getenv("V2E_AMD_CHAIN_TABLES"); // read per run, as V2E_AMD_CHAIN_FUSED is
    return !(e && atoi(e) == 0);
}

// allon: every run-time feature switch of the frame loop is on (cutoff, leak, shot noise, refractory period: the v2e CLI
// defaults) -> the instantiation without those tests; built for float64 state and uint8 frames (what that configuration has)
static const void *chain_fn(bool f64, int dtype, bool fused, bool allon = false)
{
    if (allon && f64 && dtype == V2E_DT_U8)
        return fused ? (const void *)k_chain<double, uint8_t, true, true> : (const void *)k_chain<double, uint8_t, false, true>;
    if (!fused) return f64 ? (const void *)k_chain<double, uint8_t, false> : (const void *)k_chain<float, uint8_t, false>;
    switch (dtype) {
    case V2E_DT_U8: return f64 ? (const void *)k_chain<double, uint8_t, true> : (const void *)k_chain<float, uint8_t, true>;
    case V2E_DT_F32: return f64 ? (const void *)k_chain<double, float, true> : (const void *)k_chain<float, float, true>;
    default: return f64 ? (const void *)k_chain<double, double, true> : (const void *)k_chain<float, double, true>;
    }
}

// workgroups of the k_chain instantiation that will run which a CU holds (the redo rendezvous needs a clip's workgroups
// co-resident); the occupancy API can over-report by one per CU (MI355X guide), hence the margin.  Queried once per
// (handle = device, instantiation).
static int chain_blocks_per_cu(v2e_emu *h, bool f64, int dtype, bool fused, bool allon = false)
{
    // (the instantiation that will be launched: the ALLON one -- every feature switch on, the v2e CLI defaults -- needs half the
    // registers of the general fused one, so twice the clips of a multi-clip run fit beside one another)
    allon = allon && f64 && dtype == V2E_DT_U8;
    const int key = (f64 ? 1 : 0) | ((dtype & 3) << 1) | (fused ? 8 : 0) | (allon ? 16 : 0);
    if (h->occ_cache[key] >= 0) return h->occ_cache[key];
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, chain_fn(f64, dtype, fused, allon), BLOCK, 0) != hipSuccess) per_cu = 0;
    if (per_cu > 2) per_cu = std::min(per_cu - 1, 6); // LDS-bound counts (<= 2) are exact
    h->occ_cache[key] = per_cu;
    return per_cu;
}

// Frames per chain launch.  The launch boundary (~4 us) and the prologue are paid once per K frames; a redo (rule-on frame:
// ~1 % of the frames of the benchmark clip) repeats a launch from a checkpoint.  Small grids (bounded by latency) and large
// grids without a refractory period: 32 (1280x720 noisy: 16 frames 6.24, 32 frames 6.49 Gev/s); large grids where a redo is
// possible: 8.  A clip whose workgroups cannot all be resident cannot hold the redo rendezvous: one frame per launch, where
// the one frame a redo fixes is the launch's last and nothing is left to verify (V2E_RUN_ONE_FRAME_PER_LAUNCH asks for that too:
// clips on which the rule is active on most frames would redo most launches).
static int chain_frames_per_launch(const v2e_emu *h, bool has_refr, int flags, int max_blocks)
{
    // (without a refractory period nothing is speculated and nothing redone: the longest launch the kernel supports -- 1280x720 noisy,
    //  pipelined, round 6: 64 frames 13.6-14.1 Gev/s, 32 13.0-13.5, 16 12.6-13.0)
    int K = !has_refr ? CHAIN_K_MAX : (chain_small_grid(h) ? 32 : 8);
    if (const char *ev = getenv("V2E_AMD_CHAIN_K")) { const int v = atoi(ev); if (v >= 1 && v <= CHAIN_K_MAX) K = v; }
    if (has_refr && ((flags & V2E_RUN_ONE_FRAME_PER_LAUNCH) || h->ngroups > max_blocks)) K = 1;
    return K;
}

// The launch schedule of a run, as plain data (exported for the CPU tests): per chain launch the frames it advances
// [f0, f0 + nf) and validates [pf0, pf0 + pnf), the emission batch whose completion frees the ring slots it overwrites,
// the k_ahead batch it needs, the k_ahead batch enqueued behind it, the emission batch that is final once it is enqueued.
struct ChainLaunch { int f0, nf, pf0, pnf, wait_join, wait_ahead, ahead_next, emit_batch; };
static std::vector<ChainLaunch> chain_plan(int n_frames, int K, int E, int nD, bool has_refr, bool fused)
{
    const int m = E / K;
    const int nB = (n_frames + K - 1) / K;           // chain launches with frames
    const int nL = has_refr ? nB + 1 : nB;           // + the tail launch that validates the last K frames
    const int nEB = (n_frames + E - 1) / E;          // batches of the parallel kernels
    std::vector<ChainLaunch> plan;
    for (int L = 0; L < nL; ++L) {
        ChainLaunch c;
        const bool tail = L >= nB;
        c.f0 = tail ? n_frames : L * K;
        c.nf = tail ? 0 : std::min((L + 1) * K, n_frames) - L * K;
        c.pf0 = (L - 1) * K;
        c.pnf = (has_refr && L > 0) ? std::min(L * K, n_frames) - (L - 1) * K : 0;
        const bool first = !tail && L % m == 0; // first launch of batch L / m
        c.wait_join = (first && L / m >= nD) ? L / m - nD : -1;
        c.wait_ahead = (first && !fused) ? L / m : -1;
        c.ahead_next = (first && !fused && L / m + 2 < nEB) ? L / m + 2 : -1;
        const int fin = has_refr ? L - 1 : L; // what is final now: with a refractory period the launch just validated
        c.emit_batch = (fin >= 0 && ((fin + 1) % m == 0 || fin == nB - 1)) ? fin / m : -1;
        plan.push_back(c);
    }
    return plan;
}

// scratch of the chain pipeline: everything a captured run must not allocate
// The event writer: k_cpull (a thread per output row; round 5, the default) or k_cemit (a wave per pixel group pushing its rows through
// the bijection).  The pull needs 32 bytes of pixel ballots per (frame of the three table sets, group, key) -- 281 MB at 346x260 with
// the default max_iters = 64, 18 GB for 64 clips: when that would take more than a quarter of the free device memory the push writer
// stays (same rows, bit for bit; V2E_AMD_EMIT_PULL=0 forces it: tests/test_emulator_gpu.py runs both).
static bool emit_pull(size_t table_bytes)
{
    if (const char *e = getenv("V2E_AMD_EMIT_PULL")) { if (atoi(e) == 0) return false; } // (read when a handle's tables are allocated)
    // an absolute budget as well as a share of what is free NOW (round-5 advisor: a quarter of momentarily free memory alone let the
    // choice depend on who allocated first, and 18 GB of tables for 64 clips could starve a SloMo engine built later): 24 GB per
    // scratch set by default, V2E_AMD_PULL_BUDGET_MB overrides; v2e_emu_event_writer says which writer a handle got
    size_t budget = (size_t)24 << 30;
    if (const char *e = getenv("V2E_AMD_PULL_BUDGET_MB")) { const long long v = atoll(e); if (v >= 0) budget = (size_t)v << 20; }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    return table_bytes <= free_b / 4 && table_bytes <= budget;
}

static int chain_alloc(v2e_emu *h, const v2e_emu_params *p, int dtype, int n_frames, int flags, bool pipelined)
{
    const bool has_refr = p->refractory_period_s > 0;
    const int nD = chain_ring_batches(h, pipelined);
    const bool fused = chain_fused_records(h, dtype, nD);
    const int inst = (p->f64_state ? 1 : 0) | ((dtype & 3) << 1) | (fused ? 8 : 0);
    const bool allon_p = p->cutoff_hz > 0 && p->leak_rate_hz > 0 && p->shot_noise_rate_hz > 0 && has_refr;
    const int max_blocks = chain_blocks_per_cu(h, p->f64_state != 0, dtype, fused, allon_p) * h->n_cu;
    const int K = chain_frames_per_launch(h, has_refr, flags, max_blocks);
    // frames per k_ahead launch and per emission batch: a multiple of K, 64 frames (the emission kernels are bound by per-wave latency
    // and by the launch gaps between them, and this runtime runs the captured graph's chain and emission kernels one after the
    // other: fewer, larger batches -- 346x260, round 3: 64 frames 8.7 Gev/s, 32 frames 7.7; 1280x720 noisy, round 5 with the pull
    // writer: 32 frames 9.57 / 9.61, 64 frames 10.70 / 10.71 Gev/s -- until round 5 large grids took max(K, 8) for their ring's
    // memory: 64 frames of 1280x720 are 0.7 GB of count words in a ring of three batches).  Grids whose ring would take more than an
    // eighth of the free device memory, and multi-clip runs whose short batch holds 64 (frame, clip) pairs anyway, keep the short batches.
    int m = std::max(1, 64 / K);
    if (!chain_small_grid(h)) {
        if (h->ch_long_batches < 0) { // decided once per handle (the answer must not change with what the handle itself allocates)
            size_t free_b = 0, total_b = 0;
            const size_t ring = (size_t)3 * 64 * h->n_clips * h->npx_pad * (sizeof(ccnt_t) + sizeof(float) + sizeof(uint32_t));
            h->ch_long_batches = (hipMemGetInfo(&free_b, &total_b) == hipSuccess && ring <= free_b / 8) ? 1 : 0;
        }
        // (64 clips of 346x260 have 2 048 (frame, clip) pairs in a 32-frame batch already: 11.64 Gev/s with 32 frames, 11.37 with 64)
        const int m_short = std::max(1, std::max(K, 8) / K);
        if (!h->ch_long_batches || (long long)m_short * K * h->n_clips >= 64) m = m_short;
    }
    if (const char *ev = getenv("V2E_AMD_CHAIN_M")) { const int v = atoi(ev); if (v >= 1 && v <= 64) m = v; }
    m = std::max(1, std::min(m, 64 / K)); // k_cemit sums a batch's per-frame event counts one frame per lane
    const int E = m * K;
    if (h->ch_K != K || h->ch_E != E || h->ch_nkeys_cap != h->nkeys_cap || h->ch_fused != (int)fused || h->ch_nD != nD) {
        // a new configuration: everything sized by it goes, in BOTH scratch sets; what the run needs is allocated below, for the set
        // that is current
        h->sync_runs();
        h->free_chain_scratch();
        h->ch_launch_cap = 0;
        h->ch_K = K;
        h->ch_E = E;
        h->ch_fused = fused;
        // (ring of frame slots: chain_ring_batches)
        h->ch_nD = nD;
        h->ch_D = nD * E;
        h->ch_nwp = (chain_egroups(h) + 15) / 16 * 16; // emission groups (one wave each), padded to the 16 a lane of k_cframe takes
        h->ch_nkeys_cap = h->nkeys_cap;
        // The event writer (decided once per configuration, for both scratch sets): the pull needs 32 bytes per (group, key) of the
        // three table sets -- only the keys a group has events of are ever written or read (no clearing)
        const size_t mask_bytes = 3 * sizeof(uint32_t) * 2 * GPX * E * (size_t)h->n_clips * h->nkeys_cap * h->ch_nwp;
        // (beyond 2 M groups = 33 M pixels the two-level search's coarse rows would not fit the 64 KB of LDS a launch gets by default)
        h->ch_pull = (h->ch_nwp / 16 <= 8192 && emit_pull(mask_bytes)) ? 1 : 0;
        h->drop_graphs();
    }
    const size_t nc = (size_t)h->n_clips;
    RunScratch &r = h->cur();
    if (!r.ch_cnt) {
        V2E_HIP(hipMalloc(&r.ch_cnt, sizeof(ccnt_t) * h->ch_D * nc * h->npx_pad));
        V2E_HIP(hipMalloc(&r.ch_ruleM, sizeof(uint32_t) * h->ch_D * nc));
        V2E_HIP(hipMemset(r.ch_ruleM, 0, sizeof(uint32_t) * h->ch_D * nc));
        // three sets of emission tables in rotation: the tables of batches b + 1, b + 2 are built while k_cemit(b) reads its own
        V2E_HIP(hipMalloc(&r.ch_wmax, 3 * sizeof(uint16_t) * E * nc * h->ch_nwp));
        V2E_HIP(hipMemset(r.ch_wmax, 0, 3 * sizeof(uint16_t) * E * nc * h->ch_nwp));
        V2E_HIP(hipMalloc(&r.ch_wtot, sizeof(uint16_t) * 3 * E * nc * h->nkeys_cap * h->ch_nwp));
        V2E_HIP(hipMemset(r.ch_wtot, 0, sizeof(uint16_t) * 3 * E * nc * h->nkeys_cap * h->ch_nwp));
        V2E_HIP(hipMalloc(&r.ch_cf, 3 * sizeof(CFrame) * E * nc));
        V2E_HIP(hipMemset(r.ch_cf, 0, 3 * sizeof(CFrame) * E * nc));
        V2E_HIP(hipMalloc(&r.ch_cdone, 3 * sizeof(unsigned) * E * nc));
        V2E_HIP(hipMemset(r.ch_cdone, 0, 3 * sizeof(unsigned) * E * nc));
        V2E_HIP(hipMalloc(&r.ch_cT, 3 * sizeof(uint32_t) * E * nc * h->nkeys_cap));
        V2E_HIP(hipMalloc(&r.ch_ckbase, 3 * sizeof(uint32_t) * E * nc * h->nkeys_cap));
        V2E_HIP(hipMalloc(&r.ch_cperm, 3 * sizeof(uint32_t) * E * nc * h->max_iters * 8));
        V2E_HIP(hipMalloc(&r.ch_cpre, 3 * sizeof(uint32_t) * E * nc * h->nkeys_cap * h->ch_nwp));
        if (h->ch_pull) {
            V2E_HIP(hipMalloc(&r.ch_cmask, 3 * sizeof(uint32_t) * 2 * GPX * E * nc * h->nkeys_cap * h->ch_nwp));
            V2E_HIP(hipMalloc(&r.ch_cpre16, 3 * sizeof(uint32_t) * E * nc * h->nkeys_cap * (h->ch_nwp / 16)));
        }
        if (!fused) { // (zero once: k_ahead never writes a slot's padding [npx, npx_pad), and k_chain's lanes beyond the frame read it)
            V2E_HIP(hipMalloc(&r.ch_rec, sizeof(uint32_t) * (size_t)h->ch_D * nc * h->npx_pad));
            V2E_HIP(hipMemset(r.ch_rec, 0, sizeof(uint32_t) * (size_t)h->ch_D * nc * h->npx_pad));
            // (and the shot masks of a wave wholly in the padding, which k_ahead never writes and k_chain never reads, stay zero)
            V2E_HIP(hipMalloc(&r.ch_msk, sizeof(uint4) * (size_t)h->ch_D * nc * (h->npx_pad / WAVE)));
            V2E_HIP(hipMemset(r.ch_msk, 0, sizeof(uint4) * (size_t)h->ch_D * nc * (h->npx_pad / WAVE)));
        }
        // The fills above are ordered on the DEFAULT stream only, and a pipelined run's head (its k_ahead records, its tables) goes out on
        // streams of the handle that do not wait for it: enqueued behind a run still executing on the default stream, the record ring's
        // fill once ran AFTER the next run's k_ahead had written its records (round 6: wrong events in the first run on a freshly
        // allocated scratch set, only with another run in flight).  Allocation is rare: wait for the device.
        V2E_HIP(hipDeviceSynchronize());
        h->drop_graphs();
    }
    h->ch_max_blocks = max_blocks;
    h->ch_inst = inst;
    const int n_launch = (n_frames + K - 1) / K + 1;
    if (n_launch + 2 > h->run_off_cap) {
        h->sync_runs();
        for (RunScratch &q : h->sets) { hipFree(q.run_off); q.run_off = nullptr; }
        h->run_off_cap = n_launch + 2;
        h->drop_graphs();
    }
    if (!r.run_off) V2E_HIP(hipMalloc(&r.run_off, sizeof(unsigned long long) * (size_t)h->run_off_cap * h->n_clips));
    if (!h->ahead) V2E_HIP(hipStreamCreateWithFlags(&h->ahead, hipStreamNonBlocking));
    if (!h->tabs) V2E_HIP(hipStreamCreateWithFlags(&h->tabs, hipStreamNonBlocking));
    if (!h->side2) V2E_HIP(hipStreamCreateWithFlags(&h->side2, hipStreamNonBlocking));
    auto grow = [&](std::vector<hipEvent_t> &v, size_t n) -> int {
        while (v.size() < n) {
            hipEvent_t e;
            V2E_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            v.push_back(e);
        }
        return 0;
    };
    if (grow(h->ev_ahead, n_launch + 1) || grow(h->ev_chain, n_launch + 1) || grow(h->ev_fork, n_launch + 1) ||
        grow(h->ev_join, n_launch + 1) || grow(h->ev_tab, n_launch + 1)) return V2E_EHIP;
    if (has_refr) {
        if (!r.ch_tsold) V2E_HIP(hipMalloc(&r.ch_tsold, sizeof(float) * (size_t)h->ch_D * h->n_clips * h->npx_pad));
        if (!h->ch_ck && K > CHAIN_SUB) V2E_HIP(hipMalloc(&h->ch_ck, (size_t)2 * (K / CHAIN_SUB - 1 + (K % CHAIN_SUB ? 1 : 0)) * 20 * h->n_clips * h->npx_pad)); // see ChainArgs::ckc_base
        if (!h->ch_base2) {
            const size_t n = (size_t)h->n_clips * h->npx_pad;
            V2E_HIP(hipMalloc(&h->ch_base2, sizeof(double) * n));
            V2E_HIP(hipMalloc(&h->ch_lp2, sizeof(double) * n));
            V2E_HIP(hipMalloc(&h->ch_ts2, sizeof(float) * n));
            V2E_HIP(hipMemset(h->ch_base2, 0, sizeof(double) * n));
            V2E_HIP(hipMemset(h->ch_lp2, 0, sizeof(double) * n));
            V2E_HIP(hipMemset(h->ch_ts2, 0, sizeof(float) * n));
            V2E_HIP(hipDeviceSynchronize()); // (as above)
        }
        if (n_launch > h->ch_launch_cap) {
            h->sync_runs();
            for (RunScratch &q : h->sets) { hipFree(q.ch_gM); hipFree(q.ch_bar); q.ch_gM = nullptr; q.ch_bar = nullptr; }
            h->ch_launch_cap = n_launch;
            h->drop_graphs();
        }
        if (!r.ch_gM) {
            V2E_HIP(hipMalloc(&r.ch_gM, sizeof(uint32_t) * (size_t)h->ch_launch_cap * (K + 1) * h->n_clips * K));
            V2E_HIP(hipMalloc(&r.ch_bar, sizeof(unsigned) * (size_t)h->ch_launch_cap * 2 * K * h->n_clips));
            h->drop_graphs();
        }
    }
    return 0;
}

// can this run go through k_chain?  (otherwise: the count / rank / scan / emit kernels, one frame at a time)
static bool chain_eligible(const v2e_emu *h, const v2e_emu_params *p, int dtype)
{
    if (h->max_iters > CHAIN_MAX_ITERS) return false;
    if (dtype == V2E_DT_F64 && p->log_input) return false; // the frame record carries the lin-log value as float32
    if (p->photoreceptor_noise) return false;              // one more state plane and normal per pixel
    if (h->sc_hp) return false;                            // SCIDVS: two more state planes
    if (h->cs_sur) return false;                           // CSDVS: the surround is stepped between frames
    return true;
}

// How enqueue_run_chain puts a run out
enum class ChainMode {
    plain,     // on the handle's streams, forked from and joined into the caller's stream
    captured,  // the same under stream capture: edges between the origin stream and a forked stream only, so tables and rows share ST_SIDE
    pipelined, // the caller's stream carries the chain only; head and emission go to the handle's streams and are not joined
    profiled,  // as plain, but every kernel on the caller's stream, with HIP events around the chain launches and the event rows (marks)
};
struct ChainMarks { std::vector<hipEvent_t> chain, rows; }; // the events of a profiled run, in pairs (before, after)

static int enqueue_run_chain(v2e_emu *h, const v2e_emu_params *p, const KArgs &a_in, int dtype, int n_frames, float *events,
                             uint64_t cap, v2e_frame_rec *recs, hipStream_t s, ChainMode mode, ChainMarks *marks = nullptr,
                             hipEvent_t run_done = nullptr) // pipelined: completes with the run's last chain launch
{
    // Three logical streams: the chain (k_chain, K frames per launch); k_ahead and the emission tables (k_ctot, k_cframe);
    // the event writer k_cemit; the last two in batches of E = m K frames (batch b = frames [b E, (b + 1) E) = chain
    // launches [b m, (b + 1) m)).  The emission of a batch is a pipeline of its own: tables of batch b + 1 beside the rows of b.
    //   k_ahead(b)  before chain launch b m; overwrites the records of batch b - nD, last read by launch (b - nD + 1) m (its redo)
    //   tables(b)   once batch b is final: after the launch that validated its last K frames (or, without a refractory
    //               period, after its last launch); k_cemit(b) after tables(b) and k_cemit(b - 1) (running event offset)
    //   chain launch b m overwrites the ring slots of batch b - nD: after k_cemit(b - nD)   (nD = ch_D / E batches in the ring)
    const bool captured = mode == ChainMode::captured, pipelined = mode == ChainMode::pipelined;
    const RunScratch &r = h->cur();
    const size_t esz = dtype_size(dtype);
    const bool has_refr = p->refractory_period_s > 0;
    const int K = h->ch_K, E = h->ch_E, m = E / K, D = h->ch_D, NC = h->n_clips, nD = h->ch_nD;
    const bool fused_rec = h->ch_fused != 0;
    const std::vector<ChainLaunch> plan = chain_plan(n_frames, K, E, nD, has_refr, fused_rec);
    const int nL = (int)plan.size();
    const int nB = (n_frames + K - 1) / K;
    const int nEB = (n_frames + E - 1) / E;
    KArgs a = a_in; // kernel arguments are passed by address (hipLaunchKernel copies them at the call)
    Sched sc;
    sc.h = h; sc.st[ST_MAIN] = s; sc.st[ST_AHEAD] = h->ahead; sc.st[ST_SIDE] = h->side; sc.st[ST_TAB] = h->tabs; sc.st[ST_SIDE2] = h->side2;
    if (mode == ChainMode::profiled) // every kernel on the one stream, so that a launch's HIP events bracket that kernel running alone --
        for (int q = 0; q < ST_COUNT; ++q) sc.st[q] = s; // which is how the captured graph of the timed runs executes on this runtime
    auto mark = [&](bool rows, hipStream_t stq) -> int {
        if (mode != ChainMode::profiled) return 0;
        hipEvent_t e;
        V2E_HIP(hipEventCreate(&e));
        (rows ? marks->rows : marks->chain).push_back(e);
        V2E_HIP(hipEventRecord(e, stq));
        return 0;
    };
    // clips resident at once: with a refractory period every workgroup of a clip must be resident for the redo rendezvous
    // (K = 1 has no rendezvous: all clips at once)
    int gy = NC;
    if (has_refr && K > 1) gy = std::max(1, std::min(NC, h->ch_max_blocks / std::max(h->ngroups, 1)));
    dim3 grid(h->ngroups, gy);
    // Where the emission goes.  Captured: tables and rows on ST_SIDE (the only forked stream with edges to the origin), the rows
    // carrying the running event offset forward themselves.  Pipelined: tables on ST_SIDE, rows on ST_SIDE2 -- with both on one stream
    // that stream was busy ~500 of a step's 720 us and the chain waited for it where the ring wraps (717-732 -> 699-713 us per step).
    // Plain: tables on ST_TAB, rows alternating ST_SIDE / ST_SIDE2 by batch (two batches' rows side by side, k_coff behind the tables).
    const int tab_stream = captured || pipelined ? ST_SIDE : ST_TAB;
    constexpr int NSET = 3; // emission table sets (chain_alloc sizes them)
    // b: the emission's slot (event indices, table set b % NSET, event offsets run_off[b] -> run_off[b + 1]); frames [ef0, ef0 + enE).
    // A batch is normally slot b = frames [b E, (b + 1) E); the run's LAST batch may be emitted in two pieces (slots nEB - 1, nEB).
    // (Round 5 measured the tables of the run's LAST pieces on the chain's stream, beside the rows of the batch before on the side
    // stream: 12.0 -> 11.5 Gev/s -- they delay the tail launch, which the last rows wait for.  Not kept.)
    auto launch_emission = [&](int b, int ef0, int enE) -> int { // EV_FORK[b] has been recorded on the chain stream
        CEmitArgs ea;
        memset(&ea, 0, sizeof(ea));
        ea.ctl = r.run_ctl; ea.recs = recs; ea.fidx_base = r.run_fidx;
        ea.f0 = ef0; ea.nE = enE; ea.D = D; ea.n_clips = NC; ea.slot0 = ef0 % D;
        ea.nwp = h->ch_nwp; ea.nwaves = chain_egroups(h); ea.E = E; // emission groups (GROUP_PX pixels, one wave each)
        ea.cnt = r.ch_cnt; ea.tsold = has_refr ? r.ch_tsold : nullptr; ea.ruleM = has_refr ? r.ch_ruleM : nullptr;
        const size_t set = (size_t)(b % NSET) * E * NC; // table set of this batch
        ea.wmax = r.ch_wmax + set * h->ch_nwp; ea.wtot = r.ch_wtot + set * h->nkeys_cap * h->ch_nwp;
        ea.cf = r.ch_cf + set; ea.cT = r.ch_cT + set * h->nkeys_cap; ea.ckbase = r.ch_ckbase + set * h->nkeys_cap;
        ea.cperm = r.ch_cperm + set * h->max_iters * 8; ea.cpre = r.ch_cpre + set * h->nkeys_cap * h->ch_nwp;
        ea.cdone = r.ch_cdone + set;
        const bool pull = r.ch_cmask != nullptr;
        ea.cmask = pull ? r.ch_cmask + set * h->ch_nwp * h->nkeys_cap * 2 * GPX : nullptr;
        // k_cpull: small frames search a whole prefix row in LDS (346x260: 1.4 KB per key) through a bucket index, a workgroup per
        // V2E_PULL_PX_PER_WG pixels' worth of a frame's rows; large ones search every 16th entry there and one line from L2, and take more, smaller workgroups (their
        // batches are few frames: the launch needs the parallelism)
        bool two = h->ch_nwp > 1024;
        if (const char *ev = getenv("V2E_AMD_PULL_TWO_LEVEL")) two = atoi(ev) != 0;
        ea.cpre16 = pull && two ? r.ch_cpre16 + set * h->nkeys_cap * (h->ch_nwp / 16) : nullptr;
        ea.wpf = std::max(4, std::min(two ? 128 : 64, h->npx / (two ? 2048 : V2E_PULL_PX_PER_WG))); // (1280x720 noisy, round 5: 450 workgroups per frame 9.28, 128: 9.68, push 9.41 Gev/s)
        ea.p2 = two ? 16 : 64;
        while (ea.p2 < (two ? h->ch_nwp / 16 : ea.nwaves)) ea.p2 *= 2;
        ea.events = (float4 *)events; ea.cap = cap;
        ea.off_in = r.run_off + (size_t)b * NC;
        ea.off_out = r.run_off + (size_t)(b + 1) * NC;
        // event records of k_cemit: 256 x ich per group (wave) and pass.  The chain's workgroups need their LDS (5 KB per frame)
        // on every CU: 4 iterations per pass (measured at 346x260: 3 / 6 / 10 per pass 10.47 / 10.30 / 10.31 Gev/s) keep an emission workgroup of four groups at 16 KB
        ea.ich = 4;
        ea.capw = GROUP_PX * ea.ich;
        ea.coff_in_cemit = captured || pipelined ? 1 : 0; // (one row stream per run: no k_coff launch)
        // frames per workgroup (measured at 346x260, 32-frame batches: k_ctot 4 frames 13 us, 32 frames 37 us; k_cemit 1 frame
        // 34 us, 8 frames 45 us -- these kernels are bound by the latency of a wave's dependent loads, not by wave dispatch:
        // more, shorter waves win)
        ea.zpw_tot = CTOT_ZF;
        ea.zpw_emit = 1; // (k_cemit: one frame per workgroup; several per workgroup measured slower and cost 25 % more instructions)
        const int REC_LDS = (ea.capw + WAVE) * 4 * (BLOCK / WAVE);
        const int egx = (chain_egroups(h) + BLOCK / WAVE - 1) / (BLOCK / WAVE); // workgroups of four emission groups
        void *args[] = {(void *)&a, (void *)&ea};
        // NSET table sets rotate: tables(b + 1) are built while k_cemit(b) reads those of b; k_cemit(b - NSET), which read this set
        // last, is waited for (captured: it is on the same stream)
        if (sc.wait(tab_stream, EV_FORK, b)) return V2E_EHIP;
        if (b >= NSET && !captured && sc.wait(tab_stream, EV_JOIN, b - NSET)) return V2E_EHIP;
        if (sc.kernel(tab_stream, (const void *)k_ctot, dim3(egx, NC, (ea.nE + CTOT_ZF - 1) / CTOT_ZF), dim3(BLOCK), 0, args)) return V2E_EHIP;
        // a key row of a small grid is a couple of steps of one wave: one workgroup per frame; of a large grid (beyond a million
        // pixels) a segmented scan by a workgroup of its own.  (1280x720 has 3 600 groups since the groups are 256 pixels: k_cframe1,
        // 45 us per 32 frames; round 5 measured k_cframe there: 9.74 / 9.51 -> 8.89 / 9.02 Gev/s.)
        if (h->ch_nwp <= 4096) {
            if (sc.kernel(tab_stream, (const void *)k_cframe1, dim3(1, NC, ea.nE), dim3(CFRAME_THREADS), 0, args)) return V2E_EHIP;
        } else if (sc.kernel(tab_stream, (const void *)k_cframe, dim3(std::min(h->nkeys_cap, CFRAME_ROWS), NC, ea.nE), dim3(CFRAME_THREADS), 0, args)) {
            return V2E_EHIP;
        }
        const int row_stream = pipelined ? ST_SIDE2 : captured ? ST_SIDE : ((b & 1) ? ST_SIDE2 : ST_SIDE);
        if (!ea.coff_in_cemit) {
            void *oargs[] = {(void *)&ea};
            if (sc.kernel(tab_stream, (const void *)k_coff, dim3(NC), dim3(WAVE), 0, oargs)) return V2E_EHIP;
        }
        if (sc.record(EV_TAB, b, tab_stream)) return V2E_EHIP;
        if (!captured && sc.wait(row_stream, EV_TAB, b)) return V2E_EHIP;
        if (mark(true, sc.st[row_stream])) return V2E_EHIP;
        if (pull) {
            if (sc.kernel(row_stream, ea.cpre16 ? (const void *)k_cpull<true> : (const void *)k_cpull<false>, dim3(8 * ea.wpf * ((ea.nE + 7) / 8), NC), dim3(BLOCK), (size_t)(2 * ea.p2 * (ea.cpre16 ? 4 : 6)), args)) return V2E_EHIP;
        } else if (sc.kernel(row_stream, (const void *)k_cemit, dim3(egx, NC, ea.nE), dim3(BLOCK), (size_t)REC_LDS, args)) return V2E_EHIP;
        if (mark(true, sc.st[row_stream])) return V2E_EHIP;
        return sc.record(EV_JOIN, b, row_stream);
    };
    // Batch 0 of a run is split at the first chain launch's frames: the chain starts after the records of K frames, not of E
    // (its first launch idled through the whole first k_ahead: ~15 us of every 300-frame step); the rest of the batch follows on
    // the same stream and is waited for by the batch's other launches (event slot nL of EV_AHEAD: the batches use 0 .. nEB - 1).
    // (Pipelined runs: the head runs beside the run before, the chain never waits for it -- one k_ahead launch, one event and one wait
    // fewer: profiles/r06_emulator_experiments.txt item 14.)
    const bool split0 = m > 1 && n_frames > K && !pipelined;
    // Pipelined runs whose ring holds the whole run (n_frames <= D: 300 frames in five batches of 64): ONE k_ahead launch for the run, right
    // behind its upload and zero fills, and ONE wait of the chain for all of it -- in steady state it ran beside the run before.  Every
    // wait and every record on the chain's stream costs its next launch ~7 us even when the event has long completed (gap before a
    // batch's first launch 13-16 us, before its second 6-7: profiles/r06_emulator_experiments.txt item 23).
    const bool ahead_whole = pipelined && !fused_rec && n_frames <= D;
    auto launch_ahead = [&](int b) -> int {
        if (!ahead_whole && b >= nD && sc.wait(ST_AHEAD, EV_CHAIN, (b - nD + 1) * m)) return V2E_EHIP; // records of batch b - nD: last read by that launch's redo
        // frame pairs touched by a launch: at most nf / 2 + 1 (the device knows the run's first frame index, the host
        // does not when it builds a graph: one extra pair covers either alignment; threads of a pair outside the range return)
        const int b0 = ahead_whole ? 0 : b * E, b1 = ahead_whole ? n_frames : std::min((b + 1) * E, n_frames);
        const int cut = (b == 0 && split0) ? std::min(K, b1) : b1;
        for (int part = 0; part < 2; ++part) {
            const int f0 = part == 0 ? b0 : cut, f1 = part == 0 ? cut : b1;
            if (f1 <= f0) continue;
            AheadArgs aa;
            memset(&aa, 0, sizeof(aa));
            aa.frames_pp = r.run_frames; aa.frame_stride = (unsigned long long)NC * h->npx * esz;
            aa.ctl = r.run_ctl; aa.fidx_base = r.run_fidx;
            aa.f0 = f0; aa.nf = f1 - f0; aa.D = D; aa.n_clips = NC; aa.slot0 = f0 % D;
            aa.rec = r.ch_rec; aa.msk = r.ch_msk;
            // frame pairs per thread: a thread's set-up (thresholds, two divisions, the seed's ten Philox round keys) is paid once per
            // thread, so a thread takes several pairs -- as many as leave ~4 workgroups per CU (346x260, 64 frames: 3 z-blocks of 11 pairs;
            // round 6, A/B x 3 in one session: 1 pair 683-689 us per step, 4: 668-676, 11: 665-670, 16: 663-671; k_ahead's instructions
            // per 64-pixel wave-frame 133 + 81 -> 108 + 43), at most 16
            {
                const int pairs = aa.nf / 2 + 1;
                const long long wg_xy = (long long)h->ngroups * NC;
                int zb = (int)std::min<long long>(pairs, std::max<long long>((4ll * h->n_cu + wg_xy - 1) / wg_xy, (pairs + 15) / 16));
                aa.ppt = (pairs + zb - 1) / zb;
            }
            void *args[] = {(void *)&a, (void *)&aa};
            if (sc.kernel(ST_AHEAD, (const void *)k_ahead<uint8_t>, dim3(h->ngroups, NC, (aa.nf / 2 + 1 + aa.ppt - 1) / aa.ppt), dim3(BLOCK), 0, args)) return V2E_EHIP;
            if (sc.record(EV_AHEAD, part == 0 ? b : nL, ST_AHEAD)) return V2E_EHIP;
        }
        return 0;
    };
    // state planes: X[0] the caller's (bound) planes, X[1] the engine's second set; launch L reads X[L % 2], writes X[(L + 1) % 2]
    void *xb[2] = {h->base, has_refr ? h->ch_base2 : h->base}, *xl[2] = {h->lp, has_refr ? h->ch_lp2 : h->lp};
    float *xt[2] = {h->ts_mem, has_refr ? h->ch_ts2 : h->ts_mem};
    // The run's zero fills precede the fork.  (Round 5 tried the fork first -- k_ahead touches nothing the fill clears -- and lost 10 %:
    // 12.0 -> 10.8 Gev/s, A/B x 3 in one session; the enqueue order of a capture decides which branches this runtime overlaps,
    // profiles/r03_graph_scheduling.txt.)
    {   // one launch: the run's records, batch 0's event offset, and (refractory runs) the rule-on maxima and rendezvous counters
        void *const zp[4] = {recs, r.run_off, has_refr ? (void *)r.ch_gM : nullptr, has_refr ? (void *)r.ch_bar : nullptr};
        const size_t zb[4] = {sizeof(v2e_frame_rec) * (size_t)n_frames * NC, sizeof(unsigned long long) * NC,
                              sizeof(uint32_t) * (size_t)nL * (K + 1) * NC * K, sizeof(unsigned) * (size_t)nL * 2 * K * NC};
        if (sc.zero4(pipelined ? ST_AHEAD : ST_MAIN, zp, zb)) return V2E_EHIP;
    }
    // (pipelined: no forks -- the k_ahead stream carries the run's upload and zero fills itself and runs ahead of the chain, the
    // emission streams wait for the chain batch by batch; captured: the side stream joins at its first batch)
    if (!pipelined) {
        if (sc.record(EV_FORK, nL, ST_MAIN)) return V2E_EHIP;
        if (!captured && sc.wait(ST_SIDE, EV_FORK, nL)) return V2E_EHIP;
        if (!fused_rec && sc.wait(ST_AHEAD, EV_FORK, nL)) return V2E_EHIP;
        if (!captured && (sc.wait(ST_TAB, EV_FORK, nL) || sc.wait(ST_SIDE2, EV_FORK, nL))) return V2E_EHIP;
    }
    int last_ahead = -1; // the last k_ahead batch this piece enqueued (joined at the end)
    if (ahead_whole && launch_ahead(0)) return V2E_EHIP; // (all of the run's records: before the one event the chain waits for)
    if (pipelined && (sc.record(EV_FORK, nL, ST_AHEAD) || sc.wait(ST_MAIN, EV_FORK, nL))) return V2E_EHIP; // the upload and the zero fills, for the chain
    for (int b = 0; b < std::min(nEB, 2) && !fused_rec && !ahead_whole; ++b) {
        if (launch_ahead(b)) return V2E_EHIP;
        last_ahead = b;
    }
    // last batch in two pieces: only where the last launch is not the first of its batch (else there is nothing to emit early)
    const int tail_f0 = (nB - 1) * K;                          // first frame of the last chain launch with frames
    // (pipelined runs: the last emission finishes beside the next run's chain -- one piece, six API calls fewer)
    const bool split_tail = has_refr && m > 1 && nB >= 2 && (nB - 1) % m != 0 && !pipelined;
    int last_emitted = -1; // the last emission slot this piece enqueued (joined at the end)
    const bool allon = a_in.has_cutoff && a_in.do_leak && a_in.do_shot && a_in.has_refr;
    const void *kfn = chain_fn(p->f64_state != 0, dtype, fused_rec, allon);
    const int tables = (!fused_rec && chain_decode_tables()) ? 1 : 0;
    for (int L = 0; L < nL; ++L) {
        const ChainLaunch &pl = plan[L];
        const bool tail = pl.nf == 0;
        ChainArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.frames_pp = r.run_frames; ca.frame_stride = (unsigned long long)NC * h->npx * esz; ca.fidx_base = r.run_fidx;
        ca.ctl = r.run_ctl;
        ca.f0 = pl.f0; ca.nf = pl.nf; ca.pf0 = pl.pf0; ca.pnf = pl.pnf;
        ca.D = D; ca.n_clips = NC; ca.K = K; ca.ngroups = h->ngroups;
        ca.slot_f0 = pl.f0 % D; ca.slot_pf0 = pl.pf0 % D;
        ca.cnt = r.ch_cnt; ca.ruleM = r.ch_ruleM; ca.tsold = has_refr ? r.ch_tsold : nullptr;
        ca.rec = r.ch_rec; ca.msk = r.ch_msk;
        if (has_refr) {
            ca.gM_cur = r.ch_gM + (size_t)L * (K + 1) * NC * K;
            ca.gM_prev = r.ch_gM + (size_t)(L > 0 ? L - 1 : 0) * (K + 1) * NC * K;
            ca.bar_prev = r.ch_bar + (size_t)(L > 0 ? L - 1 : 0) * 2 * K * NC;
        }
        const int in = L % 2, out = tail ? 0 : (L + 1) % 2, pin = (L + 1) % 2;
        ca.base_in = xb[in]; ca.lp_in = xl[in]; ca.ts_in = xt[in];
        ca.base_fix = xb[in]; ca.lp_fix = xl[in]; ca.ts_fix = xt[in];
        ca.base_out = xb[out]; ca.lp_out = xl[out]; ca.ts_out = xt[out];
        ca.base_pin = xb[pin]; ca.lp_pin = xl[pin]; ca.ts_pin = xt[pin];
        if (has_refr && K > CHAIN_SUB && h->ch_ck) {
            const size_t plane = (size_t)(K / CHAIN_SUB - 1 + (K % CHAIN_SUB ? 1 : 0)) * NC * h->npx_pad; // elements per (parity, quantity): a checkpoint before frames 8, 16, ...
            auto ck = [&](int par, char *&bp, char *&lpp, float *&tp) {
                char *q = (char *)h->ch_ck + (size_t)par * plane * 20;
                bp = q; lpp = q + plane * 8; tp = (float *)(q + plane * 16);
            };
            char *b0, *l0, *b1, *l1; float *t0, *t1;
            ck(L % 2, b0, l0, t0);
            ck((L + 1) % 2, b1, l1, t1);
            ca.ckc_base = b0; ca.ckc_lp = l0; ca.ckc_ts = t0;
            ca.ckp_base = b1; ca.ckp_lp = l1; ca.ckp_ts = t1;
        }
        ca.recs = recs;
        ca.store_out = tail && in != 0;
        ca.prio = 3;      // wave priority of the chain (measured against 0 in round 3)
        ca.bar_light = 1; // the fence-free rendezvous (round 4; the fenced one of round 3 is still in clip_barrier)
        ca.tables = tables;
        ca.lockstep = 0;  // lock-step redo passes (emu_chain.h, V2E_CHAIN_LOCKSTEP): 10.4-10.6 against 10.8-11.0 Gev/s on the benchmark clip (round 4)
        ca.dbg = (h->dbg && L == nB / 2) ? h->dbg : nullptr;
        ca.stamp_pp = r.stamp_slot; ca.lidx = std::min(L, STAMP_LAUNCHES - 1);
        if (pl.wait_join >= 0 && sc.wait(ST_MAIN, EV_JOIN, pl.wait_join)) return V2E_EHIP; // ring slots: read by k_cemit of that batch
        if (!ahead_whole && pl.wait_ahead >= 0 && sc.wait(ST_MAIN, EV_AHEAD, pl.wait_ahead)) return V2E_EHIP;
        if (split0 && !fused_rec && !tail && L >= 1 && L < m && sc.wait(ST_MAIN, EV_AHEAD, nL)) return V2E_EHIP; // the rest of batch 0
        if (mark(false, s)) return V2E_EHIP; // profiled runs: an event before and after every chain launch
        // Pipelined: whatever would be recorded behind this launch -- the run's end, the emission batch it makes final, what a later
        // k_ahead batch waits for where the ring wraps -- is its stop event: the chain's queue holds launches and waits only (a record
        // there cost the next launch 2.4 us, and its waiter 3.8 us more: profiles/r24_chain_queue_packets.txt)
        const bool rec_chain = !ahead_whole && !fused_rec && L % m == 0;
        hipEvent_t stop = nullptr;
        if (pipelined) {
            auto follows = [&](int kind, int idx) {
                if (!stop) stop = sc.real_event(kind, idx);
                else sc.stand_in.push_back({kind, idx, stop});
            };
            if (L == nL - 1) stop = run_done;
            if (pl.emit_batch >= 0) follows(EV_FORK, pl.emit_batch);
            if (rec_chain) follows(EV_CHAIN, L);
        }
        void *args[] = {(void *)&a, (void *)&ca};
        if (sc.kernel(ST_MAIN, kfn, grid, dim3(BLOCK), 0, args, stop)) return V2E_EHIP;
        if (mark(false, s)) return V2E_EHIP;
        if (!pipelined && rec_chain && sc.record(EV_CHAIN, L, ST_MAIN)) return V2E_EHIP; // (what a later k_ahead batch waits for where the ring wraps)
        // k_ahead before the emission: the enqueue order decides how this runtime executes the captured graph -- with the emission
        // first the chain's next launch runs BEHIND the emission kernels, with k_ahead first beside them (profiles/r03_graph_scheduling.txt)
        if (!ahead_whole && pl.ahead_next >= 0) { if (launch_ahead(pl.ahead_next)) return V2E_EHIP; last_ahead = pl.ahead_next; }
        if (split_tail && L == nB - 1 && tail_f0 > (nEB - 1) * E) {
            if (sc.record(EV_FORK, nEB - 1, ST_MAIN)) return V2E_EHIP;
            if (launch_emission(nEB - 1, (nEB - 1) * E, tail_f0 - (nEB - 1) * E)) return V2E_EHIP;
            last_emitted = nEB - 1;
        }
        if (pl.emit_batch >= 0 && split_tail && pl.emit_batch == nEB - 1 && tail_f0 > (nEB - 1) * E) {
            if (sc.record(EV_FORK, nEB, ST_MAIN)) return V2E_EHIP;
            if (launch_emission(nEB, tail_f0, n_frames - tail_f0)) return V2E_EHIP;
            last_emitted = nEB;
        } else if (pl.emit_batch >= 0) {
            // (emitting the batches in PAIRS -- one record on the chain's stream per 128 frames -- was measured in round 6: gaps inside a run
            //  54 -> 46 us, but the bunched emission costs the chain's launches more than that: 614-633 -> 628-641 us per step)
            if (!pipelined && sc.record(EV_FORK, pl.emit_batch, ST_MAIN)) return V2E_EHIP;
            if (launch_emission(pl.emit_batch, pl.emit_batch * E, std::min((pl.emit_batch + 1) * E, n_frames) - pl.emit_batch * E)) return V2E_EHIP;
            last_emitted = pl.emit_batch;
        }
    }
    if (!pipelined) { // join: the run is complete on `s`
        if (last_emitted >= 0 && sc.wait(ST_MAIN, EV_JOIN, last_emitted)) return V2E_EHIP;
        if (!captured && last_emitted >= 0 && sc.wait(ST_MAIN, EV_TAB, last_emitted)) return V2E_EHIP;
        if (!captured && last_emitted >= 1 && sc.wait(ST_MAIN, EV_JOIN, last_emitted - 1)) return V2E_EHIP;
        if (!fused_rec && last_ahead >= 0 && sc.wait(ST_MAIN, EV_AHEAD, last_ahead)) return V2E_EHIP;
    }
    V2E_HIP(hipGetLastError());
    memcpy(h->last_queue_ops, sc.ops, sizeof(sc.ops));
    return 0;
}

// ---- which of the handle's streams share a HARDWARE queue with the caller's (pipelined runs)
// This runtime serves every stream of a process from four in-order hardware queues (more make every cross-queue dependency cost
// 20-50 us: profiles/r06_emulator_experiments.txt item 5), so of the five streams a pipelined run uses at least two share one -- which
// two is decided by how many streams the process happened to have when the handle created its own.  When the chain's stream shares
// its queue with the rows' or the tables' stream, their kernels take turns with the chain's: 1280x720 noisy 10.3 instead of 13.7 Gev/s
// (experiment 32: the same leg behind 0 .. 6 other live streams).  So the roles are given out by MEASUREMENT, once per handle and
// caller's stream: a kernel that spins for 100 us on one stream and a kernel that reads the clock on the other -- on one hardware queue
// the second starts when the first has ended, on two it starts at once.  Roles: k_ahead, tables, rows on three queues that are not the
// chain's; the stream left over (`tabs`, idle in pipelined runs) takes whatever remains.
extern "C" { // (the two kernels keep the unmangled names they have in the code object)
namespace {
__global__ void k_probe_spin(unsigned long long *out, unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16); // (bounded by the clock: 100 MHz ticks)
    out[0] = wall_clock64();
}
__global__ void k_probe_stamp(unsigned long long *out) { out[1] = wall_clock64(); }
} // namespace
} // extern "C"

// 1: b's kernel waited for a's (one hardware queue, or a == b); 0: it ran beside it; < 0: HIP error
static int streams_share_queue(hipStream_t a, hipStream_t b, unsigned long long *dev)
{
    if (a == b) return 1;
    int shared = 1;
    for (int trial = 0; trial < 2 && shared; ++trial) { // (a late enqueue of the second kernel looks like sharing: one clean trial decides)
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
        k_probe_spin<<<1, 64, 0, a>>>(dev, 10000ull);
        k_probe_stamp<<<1, 64, 0, b>>>(dev);
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
        unsigned long long t[2] = {0, 0};
        if (hipMemcpy(t, dev, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        shared = t[1] >= t[0] ? 1 : 0;
    }
    return shared;
}

static int assign_pipelined_streams(v2e_emu *h, hipStream_t s)
{
    if (getenv("V2E_AMD_NO_QUEUE_PROBE")) return 0;
    h->sync_runs();
    V2E_HIP(hipDeviceSynchronize());
    unsigned long long *dev = nullptr;
    V2E_HIP(hipMalloc(&dev, 2 * sizeof(unsigned long long)));
    std::vector<hipStream_t> cand = {h->ahead, h->side, h->side2, h->tabs};
    for (hipStream_t q : h->spare_streams) cand.push_back(q);
    h->spare_streams.clear();
    while (cand.size() < 8) { // (streams take the least-loaded hardware queue when they are created: eight cover all four)
        hipStream_t q = nullptr;
        if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) break;
        cand.push_back(q);
    }
    std::vector<char> used(cand.size(), 0);
    bool failed = false;
    auto pick = [&](std::initializer_list<hipStream_t> avoid) -> int {
        for (size_t i = 0; i < cand.size(); ++i) {
            if (used[i]) continue;
            bool ok = true;
            for (hipStream_t a : avoid) {
                const int sh = streams_share_queue(a, cand[i], dev);
                if (sh < 0) failed = true;
                if (sh != 0) { ok = false; break; }
            }
            if (ok) { used[i] = 1; return (int)i; }
        }
        return -1;
    };
    int ia = pick({s});
    int it = ia >= 0 ? pick({s, cand[ia]}) : -1;
    int ir = it >= 0 ? pick({s, cand[ia], cand[it]}) : -1;
    if (it >= 0 && ir < 0) ir = pick({s, cand[ia]}); // (three free queues were not found: the rows share the tables' rather than the chain's)
    if (getenv("V2E_AMD_PROBE_DEBUG")) { // dev: the candidates' relation to the caller's stream and to each other
        fprintf(stderr, "queue probe: ahead %d tables %d rows %d failed %d | shares caller:", ia, it, ir, (int)failed);
        for (size_t i = 0; i < cand.size(); ++i) fprintf(stderr, " %d", streams_share_queue(s, cand[i], dev));
        fprintf(stderr, " | with candidate 0:");
        for (size_t i = 0; i < cand.size(); ++i) fprintf(stderr, " %d", streams_share_queue(cand[0], cand[i], dev));
        fprintf(stderr, "\n");
    }
    hipFree(dev);
    if (!failed && ia >= 0 && it >= 0 && ir >= 0) {
        h->ahead = cand[ia]; h->side = cand[it]; h->side2 = cand[ir];
        bool have_tabs = false;
        for (size_t i = 0; i < cand.size(); ++i) {
            if (used[i]) continue;
            if (!have_tabs) { h->tabs = cand[i]; have_tabs = true; }
            else h->spare_streams.push_back(cand[i]);
        }
        h->drop_graphs(); // (captured with the old roles)
    } else { // leave the roles as they were; the new candidates are kept for the handle's destruction
        for (size_t i = 4; i < cand.size(); ++i) h->spare_streams.push_back(cand[i]);
    }
    h->probed = true;
    h->probed_for = s;
    return 0;
}
