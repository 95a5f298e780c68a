// probe.hip -- single-pixel model states of a device-resident run (v2e_emu_set_probes) for gfx950 / MI355X.
//
// The reference's research recorder (--record_single_pixel_states, v2ecore/emulator.py:279-300, 985-1009) reads ten numbers
// for one pixel after every frame.  A run that goes through the per-frame kernels (emu_kernels.h: k_count -> k_rank -> k_scan ->
// k_emit) gets them from three small kernels enqueued with it, for up to V2E_PROBE_MAX pixels at once:
//   k_probe_tap_count   behind k_count of frame f: new_frame, log_new_frame, diff_frame            emulator.py:666, 749-754
//   k_probe_tap_emit    behind k_emit of frame f:  base_log_frame, lp_log_frame, the thresholds   emulator.py:936-942, 985
//   k_probe_count_rows  once, behind the last frame: the signal ON / OFF rows at each probed pixel per frame
//                       (final_pos_evts_frame / final_neg_evts_frame)                              emulator.py:861-870
// All of them write float64 with plain stores into out[n_frames][P][V2E_PROBE_FIELDS] (field order: include/v2e_amd.h).  The
// probed pixels travel by value in the launch (V2EProbeSet): nothing is uploaded, and a captured run bakes them in.
#include "common.h"
#include "table_search.h"

namespace {

constexpr int ROWS_BLOCK = 256;

enum { F_NEW = 0, F_BASE = 1, F_LP = 2, F_LOGNEW = 3, F_POS = 4, F_NEG = 5, F_DIFF = 6, F_NEG_EVTS = 7, F_POS_EVTS = 8 };
static_assert(F_POS_EVTS + 1 == V2E_PROBE_FIELDS, "field order of include/v2e_amd.h");

// One lane per probe.  log_new_frame is what lin_log returns, a float32 tensor (emulator_utils.py:45; hdr frames are cast the same
// way when the attribute is read): the plane holds the double the kernels compute with, the recorder sees its float32 value.
template <typename FT>
__global__ __launch_bounds__(V2E_PROBE_MAX) void k_probe_tap_count(V2EProbeSet ps, const FT *__restrict__ frame,
                                                                   const double *__restrict__ lognew,
                                                                   const double *__restrict__ diff, double *__restrict__ out)
{
    const int j = threadIdx.x;
    if (j >= ps.n) return;
    const int px = ps.pix[j];
    double *o = out + (size_t)j * V2E_PROBE_FIELDS;
    o[F_NEW] = (double)frame[px];
    o[F_LOGNEW] = (double)(float)lognew[px];
    o[F_DIFF] = diff[px];
}

template <typename R>
__global__ __launch_bounds__(V2E_PROBE_MAX) void k_probe_tap_emit(V2EProbeSet ps, const R *__restrict__ lp, const R *__restrict__ base,
                                                                  const float *__restrict__ pos, const float *__restrict__ neg,
                                                                  int scalar_thres, double pos_scalar, double neg_scalar,
                                                                  double *__restrict__ out)
{
    const int j = threadIdx.x;
    if (j >= ps.n) return;
    const int px = ps.pix[j];
    double *o = out + (size_t)j * V2E_PROBE_FIELDS;
    o[F_BASE] = (double)base[px];
    o[F_LP] = (double)lp[px];
    o[F_POS] = scalar_thres ? pos_scalar : (double)pos[px];
    o[F_NEG] = scalar_thres ? neg_scalar : (double)neg[px];
}

// One pass over the run's rows (grid-stride; the number of rows is read from the last record, never more than cap).  A row's
// pixel is looked up in the LDS table of probed pixels -- every lane reads the same entry, a broadcast -- and only a row that
// hits one (a few in a million) searches for its frame (table_search.h: frame_of_row) and, if it is one of that frame's n_signal
// signal rows, adds one to the integer counters cnt[frame][probe][OFF, ON] (zero on entry).  The workgroup that finishes last turns the counters into the two
// float64 columns of out: integer atomics, so the result does not depend on the order of anything.
__global__ __launch_bounds__(ROWS_BLOCK) void k_probe_count_rows(V2EProbeSet ps, const float4 *__restrict__ ev, unsigned long long cap,
                                                                 const v2e_frame_rec *__restrict__ recs, int n_frames, int W,
                                                                 unsigned int *__restrict__ cnt, unsigned int *__restrict__ ticket,
                                                                 double *__restrict__ out)
{
    __shared__ int s_pix[V2E_PROBE_MAX];
    __shared__ int s_last;
    if (threadIdx.x < V2E_PROBE_MAX) s_pix[threadIdx.x] = threadIdx.x < ps.n ? ps.pix[threadIdx.x] : -1;
    __syncthreads();
    const v2e_frame_rec last = recs[n_frames - 1];
    unsigned long long total = last.ev_offset + last.n_events;
    if (total > cap) total = cap;
    const int P = ps.n;
    for (unsigned long long i = (unsigned long long)blockIdx.x * ROWS_BLOCK + threadIdx.x; i < total;
         i += (unsigned long long)gridDim.x * ROWS_BLOCK) {
        const float4 e = ev[i];
        const int px = (int)e.z * W + (int)e.y; // rows are [t, x = column, y = row, p]
        int f = -1;
        for (int j = 0; j < P; ++j) {
            if (s_pix[j] != px) continue;
            if (f < 0) {
                f = frame_of_row(recs, n_frames, (long long)i);
                if (i - recs[f].ev_offset >= (unsigned long long)recs[f].n_signal) break; // a shot-noise row
            }
            atomicAdd(&cnt[((size_t)f * P + j) * 2 + (e.w > 0.f ? 1 : 0)], 1u);
        }
    }
    // the last workgroup to arrive sees every counter (threadFenceReduction's rule: fence, then the ticket)
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const int n = n_frames * P * 2;
    for (int k = threadIdx.x; k < n; k += ROWS_BLOCK) {
        const unsigned int v = __hip_atomic_load(&cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[(size_t)(k >> 1) * V2E_PROBE_FIELDS + F_NEG_EVTS + (k & 1)] = (double)v;
    }
}

} // namespace

int v2e_probe_tap_count(const V2EProbeSet &ps, const void *frame, int dtype, const double *lognew, const double *diff, double *out_f,
                        hipStream_t s)
{
    switch (dtype) {
    case V2E_DT_U8: k_probe_tap_count<uint8_t><<<1, V2E_PROBE_MAX, 0, s>>>(ps, (const uint8_t *)frame, lognew, diff, out_f); break;
    case V2E_DT_F32: k_probe_tap_count<float><<<1, V2E_PROBE_MAX, 0, s>>>(ps, (const float *)frame, lognew, diff, out_f); break;
    case V2E_DT_F64: k_probe_tap_count<double><<<1, V2E_PROBE_MAX, 0, s>>>(ps, (const double *)frame, lognew, diff, out_f); break;
    default: v2e_set_error("bad frame dtype %d", dtype); return V2E_EINVAL;
    }
    return 0;
}

int v2e_probe_tap_emit(const V2EProbeSet &ps, const void *lp, const void *base, int f64_state, const float *pos, const float *neg,
                       int scalar_thres, double pos_scalar, double neg_scalar, double *out_f, hipStream_t s)
{
    if (f64_state)
        k_probe_tap_emit<double><<<1, V2E_PROBE_MAX, 0, s>>>(ps, (const double *)lp, (const double *)base, pos, neg, scalar_thres,
                                                            pos_scalar, neg_scalar, out_f);
    else
        k_probe_tap_emit<float><<<1, V2E_PROBE_MAX, 0, s>>>(ps, (const float *)lp, (const float *)base, pos, neg, scalar_thres,
                                                           pos_scalar, neg_scalar, out_f);
    return 0;
}

int v2e_probe_count_rows(const V2EProbeSet &ps, const float *events, uint64_t cap, const v2e_frame_rec *recs, int n_frames, int W,
                         unsigned int *cnt, unsigned int *ticket, double *out, int n_cu, hipStream_t s)
{
    // enough workgroups to fill the device, never more than the buffer has blocks of rows
    const uint64_t want = (cap + ROWS_BLOCK - 1) / ROWS_BLOCK, most = (uint64_t)(n_cu > 0 ? n_cu : 256) * 8;
    const unsigned grid = (unsigned)(want < 1 ? 1 : (want < most ? want : most));
    k_probe_count_rows<<<grid, ROWS_BLOCK, 0, s>>>(ps, (const float4 *)events, (unsigned long long)cap, recs, n_frames, W, cnt, ticket, out);
    return 0;
}
