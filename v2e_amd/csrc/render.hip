// render.hip -- EventRenderer.render_events_to_frames on a device-resident event packet.
//
// What the reference computes (v2ecore/renderer.py:161-400): a packet of n events is cut into exposure windows -- by time
// (DURATION), by event count (COUNT), by the first area cell that collects `area_count` events (AREA_COUNT), or not at all
// (SOURCE) -- every complete window becomes a frame clip(hist_ON - hist_OFF, +-full_scale) normalised to 0..1, the window the
// packet ends in stays behind as `currentFrame`; the packet's last event is never accumulated (renderer.py:303-306).
//
// Here the windows are not walked: one launch (k_render_hist) puts every event into the frame(s) its window rule assigns
// it to -- a binary search (table_search.h: count_le) over the packet's window boundaries (DURATION: time stamps, an event
// exactly on a boundary belongs to both neighbours, as searchsorted left / right give it; AREA_COUNT: the segment ends found by k_area_segments),
// an integer division (COUNT) -- and adds +-1 to that frame's bin; one launch (k_render_finish) clips and normalises all
// frames of the packet.  k_area_segments is the one sequential rule (a cell counter that resets at every trigger): a
// single wave walks the packet 64 events at a time, ranks the events of a chunk within their cells by ballot, and restarts
// at the trigger event, which the reference counts again in the next window (renderer.py:253-266).
//
// Whole runs (v2e_render_run*): the rows of a device-resident run plus a packet table are rendered in one pass -- the windows of
// all packets by one single-wave kernel (DURATION: k_run_windows_duration, AREA_COUNT: k_run_area_segments), one histogram
// launch in which every event first finds its packet, one finish launch, and the frame times on the device.
#include "common.h"
#include "table_search.h"

namespace {

constexpr int MODE_DURATION = 1, MODE_COUNT = 2, MODE_AREA_COUNT = 3, MODE_SOURCE = 4; // renderer.py:19-23

struct RenderArgs {
    const float4 *ev;
    long long n_used;          // events that take part: n - 1
    int mode;
    const double *bounds;      // DURATION: T_0 .. T_m (frame k = [T_k, T_k+1], the open frame m = [T_m, ...))
    int n_bounds;
    long long count_per_frame; // COUNT
    const int *seg_end;        // AREA_COUNT: end index (exclusive) of complete frame k
    int n_seg;
    int n_frames;              // complete frames + the open one
    int *diff;                 // [n_frames][bins_y * bins_x]
    int bins_y, bins_x;
    double y_lo, x_lo, delta_y, delta_x;
};

__global__ __launch_bounds__(256) void k_render_hist(RenderArgs r)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n_used) return;
    const float4 e = r.ev[i];
    // hist2d_numba_seq (v2e_utils.py:474-486): tracks[0] = y, tracks[1] = x
    const double fi = ((double)e.z - r.y_lo) * r.delta_y;
    const double fj = ((double)e.y - r.x_lo) * r.delta_x;
    if (!(fi >= 0.0 && fi < (double)r.bins_y && fj >= 0.0 && fj < (double)r.bins_x)) return;
    const int bin = (int)fi * r.bins_x + (int)fj;
    const int v = e.w == 1.0f ? 1 : -1; // pol_on = (p == 1), off = not on (renderer.py:379-380)
    long long k0 = 0, k1 = -1;
    if (r.mode == MODE_DURATION) {
        const double t = (double)e.x;
        const int c = count_le<double>(r.bounds, r.n_bounds, t);
        k0 = c - 1; // the frame whose start is the last boundary <= t; before T_0: none
        if (k0 >= 1 && r.bounds[k0] == t) k1 = k0 - 1; // searchsorted(next_start, side="right") keeps it in the frame before, too
    } else if (r.mode == MODE_COUNT) {
        k0 = i / r.count_per_frame;
    } else if (r.mode == MODE_AREA_COUNT) {
        k0 = count_le<int>(r.seg_end, r.n_seg, (int)i);
    }
    const size_t npx = (size_t)r.bins_y * r.bins_x;
    if (k0 >= 0 && k0 < r.n_frames) atomicAdd(&r.diff[(size_t)k0 * npx + bin], v);
    if (k1 >= 0 && k1 < r.n_frames) atomicAdd(&r.diff[(size_t)k1 * npx + bin], v);
}

// frames 0 .. n_complete-1: (clip(diff) + fs) / (2 fs) (renderer.py:245-247, 396-400); frame n_complete (if present): clip(diff)
__global__ __launch_bounds__(256) void k_render_finish(const int *__restrict__ diff, long long total, long long npx, int n_complete,
                                                      double *__restrict__ frames, double *__restrict__ cur, double fs)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double v = (double)diff[i];
    v = v < -fs ? -fs : (v > fs ? fs : v);
    const long long k = i / npx;
    if (k < n_complete) frames[i] = (v + fs) / (fs * 2);
    else if (cur) cur[i - k * npx] = v;
}

__global__ void k_zero_i32(int *p, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// AREA_COUNT windows (renderer.py:253-266, 292-298): walk the events in order, count per area cell, a window ends at the
// first event whose cell count reaches `area_count` -- that event opens the next window and is counted again there.
// One wave; counters in LDS (n_cells ints), carried in and left behind by the caller.  seg_end[nseg++] = end (exclusive, an
// index into this packet) of every complete window; returns 1 if the walk ended on a trigger (the reference then leaves
// zeroed counters behind).
__device__ __forceinline__ int area_walk_packet(const float4 *__restrict__ ev, long long n, int *s_cnt, int n_cells, int nw, int nh,
                                                float area_dim, int area_count, int *__restrict__ seg_end, long long cap, int &nseg)
{
    const int lane = threadIdx.x;
    const unsigned long long le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull), gt = ~le;
    long long pos = 0;
    int ended_on_trigger = 0;
    while (pos < n) {
        const long long i = pos + lane;
        const bool act = i < n;
        int cell = -1;
        if (act) {
            const float4 e = ev[i];
            int cx = (int)floorf(e.y / area_dim), cy = (int)floorf(e.z / area_dim); // int(events[i, 1] // area_dimension)
            cx = min(max(cx, 0), nw - 1);
            cy = min(max(cy, 0), nh - 1);
            cell = cx * nh + cy; // area_counts[x, y], shape (nw, nh)
        }
        // rank of every event among the chunk's events of its cell, in index order (1-based), and whether it is the last one
        int rank = 0;
        bool last = false, todo = act;
        unsigned long long tb;
        while ((tb = __ballot(todo)) != 0ull) {
            const int leader = (int)__builtin_ctzll(tb);
            const int v = __builtin_amdgcn_readlane(cell, leader);
            const unsigned long long m = __ballot(act && cell == v);
            if (act && cell == v) {
                rank = (int)__popcll(m & le);
                last = (m & gt) == 0ull;
                todo = false;
            }
        }
        const int cnt = act ? s_cnt[cell] + rank : 0;
        const unsigned long long trig = __ballot(act && cnt >= area_count);
        if (trig == 0ull) {
            if (act && last) s_cnt[cell] = cnt;
            __syncthreads();
            pos += 64;
            continue;
        }
        const long long end = pos + (int)__builtin_ctzll(trig);
        for (int c = lane; c < n_cells; c += 64) s_cnt[c] = 0; // area_counts = np.zeros_like(area_counts)
        __syncthreads();
        if (end >= n - 1) { ended_on_trigger = 1; break; } // doneWithTheseEvents: the open window takes the rest
        if (nseg < cap) { if (lane == 0) seg_end[nseg] = (int)end; }
        ++nseg;
        if (end == pos && __builtin_ctzll(trig) == 0 && area_count <= 1) break; // a window that cannot advance (the reference would not return)
        pos = end; // the trigger event is the first event of the next window
    }
    return ended_on_trigger;
}

// One packet: out[0] = complete windows found, out[1] = 1 if the walk ended on a trigger, seg_end[k] = end (exclusive) of window k.
__global__ __launch_bounds__(64) void k_area_segments(const float4 *__restrict__ ev, long long n, int *__restrict__ area_counts, int nw,
                                                     int nh, float area_dim, int area_count, int *__restrict__ seg_end, long long cap,
                                                     int *__restrict__ out)
{
    extern __shared__ int s_cnt[];
    const int lane = threadIdx.x;
    const int n_cells = nw * nh;
    for (int c = lane; c < n_cells; c += 64) s_cnt[c] = area_counts[c];
    __syncthreads();
    int nseg = 0;
    const int ended_on_trigger = area_walk_packet(ev, n, s_cnt, n_cells, nw, nh, area_dim, area_count, seg_end, cap, nseg);
    for (int c = lane; c < n_cells; c += 64) area_counts[c] = s_cnt[c];
    if (lane == 0) { out[0] = nseg; out[1] = ended_on_trigger; }
}

// ---------------------------------------------------------------------------------------------------------------- whole runs
// A run is rows[N] plus a packet table off[0..P] (packet p = rows [off[p], off[p+1]), the packets v2e.py:837-850 forms); every
// packet is rendered as the reference renders it on its own (the running frame reset, the last event left out, the frame it
// ends in discarded -- the last packet's stays behind), its complete frames numbered from pkt_f0[p] on across the run.

// DURATION windows of every packet, in order, by one lane (renderer.py:207-213, 314-318): the frame start time is carried from
// packet to packet and, in state[0] (state[1] != 0: it has been set), from run to run.  f32: numpy >= 2 keeps the float32 time
// stamp's type through `+= frameIntevalS`, so every addition is a float32 one of (float)interval; otherwise they are float64.
// Packet p's start times T_0 .. T_m go to bounds[pkt_f0[p] + p ...] (frame k complete while the packet's second-to-last time
// stamp lies past T_k+1), the frame times (start after the increment + interval / 2, renderer.py:350) to times.  bounds / times
// may be null (the counting pass); state[0..1] are written only when commit, state[2] = the start time after the run always.  out[0] = complete frames, out[1] = 1 if the interval
// does not advance the time, 2 if more than max_frames frames would be made.
__global__ __launch_bounds__(64) void k_run_windows_duration(const float4 *__restrict__ ev, const long long *__restrict__ off, int P,
                                                            double interval, int f32, double *__restrict__ state, int commit,
                                                            int *__restrict__ pkt_f0, double *__restrict__ bounds, long long cap_bounds,
                                                            double *__restrict__ times, long long cap_times, long long max_frames,
                                                            int *__restrict__ out)
{
    __shared__ float s_first[64], s_second_last[64];
    __shared__ int s_two[64];
    const int lane = threadIdx.x;
    double cur = state[0];
    bool init = state[1] != 0.0;
    long long f = 0;
    int err = 0;
    const float interval_f = (float)interval, half_f = (float)(interval / 2);
    for (int base = 0; base < P; base += 64) {
        const int p = base + lane;
        if (p < P) {
            const long long a = off[p], b = off[p + 1];
            s_first[lane] = ev[a].x;
            s_two[lane] = b - a >= 2;
            s_second_last[lane] = ev[b - a >= 2 ? b - 2 : a].x;
        }
        __syncthreads();
        if (lane == 0) {
            const int m = min(64, P - base);
            for (int j = 0; j < m && !err; ++j) {
                const int q = base + j;
                if (!init) { cur = (double)s_first[j]; init = true; }
                pkt_f0[q] = (int)f;
                if (bounds && f + q < cap_bounds) bounds[f + q] = cur;
                if (!s_two[j]) continue;
                const double t_sl = (double)s_second_last[j];
                for (;;) {
                    const double nxt = f32 ? (double)((float)cur + interval_f) : cur + interval;
                    if (!(t_sl > nxt)) break;
                    if (!(nxt > cur)) { err = 1; break; }
                    if (f >= max_frames) { err = 2; break; }
                    cur = nxt;
                    if (times && f < cap_times) times[f] = f32 ? (double)((float)cur + half_f) : cur + interval / 2;
                    ++f;
                    if (bounds && f + q < cap_bounds) bounds[f + q] = cur;
                }
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        pkt_f0[P] = (int)f;
        out[0] = (int)f;
        out[1] = err;
        state[2] = cur; // where the start time stands after this run, committed or not (the host mirrors it)
        if (commit && !err) { state[0] = cur; state[1] = init ? 1.0 : 0.0; }
    }
}

// AREA_COUNT windows of every packet in one launch: k_area_segments' walk packet after packet with the cell counters carried
// across.  seg_end[pkt_f0[p] + k] = end (exclusive, within packet p) of its window k; out[0] = complete windows of the run.
__global__ __launch_bounds__(64) void k_run_area_segments(const float4 *__restrict__ ev, const long long *__restrict__ off, int P,
                                                         int *__restrict__ area_counts, int nw, int nh, float area_dim, int area_count,
                                                         int *__restrict__ seg_end, long long cap, int *__restrict__ pkt_f0,
                                                         int *__restrict__ out)
{
    extern __shared__ int s_cnt[];
    const int lane = threadIdx.x;
    const int n_cells = nw * nh;
    for (int c = lane; c < n_cells; c += 64) s_cnt[c] = area_counts[c];
    __syncthreads();
    int nseg = 0, ended_on_trigger = 0;
    for (int p = 0; p < P; ++p) {
        if (lane == 0) pkt_f0[p] = nseg;
        const long long a = off[p];
        ended_on_trigger = area_walk_packet(ev + a, off[p + 1] - a, s_cnt, n_cells, nw, nh, area_dim, area_count, seg_end, cap, nseg);
    }
    for (int c = lane; c < n_cells; c += 64) area_counts[c] = s_cnt[c];
    if (lane == 0) { pkt_f0[P] = nseg; out[0] = nseg; out[1] = ended_on_trigger; }
}

// Time of every complete frame of a COUNT / AREA_COUNT / SOURCE run (renderer.py:343-349): SOURCE ts[0] of the packet, else
// (ts[start] + ts[end]) / 2 of the frame's window, a float32 sum as numpy forms it.
__global__ __launch_bounds__(256) void k_run_frame_times(const float4 *__restrict__ ev, const long long *__restrict__ off, int P, int mode,
                                                        long long count_per_frame, const int *__restrict__ seg_end,
                                                        const int *__restrict__ pkt_f0, int total, double *__restrict__ times)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= total) return;
    const int p = count_le<int>(pkt_f0, P, f) - 1; // the last packet that starts at or before frame f: the one that holds it
    const long long a = off[p], last = off[p + 1] - a - 1;
    const int k = f - pkt_f0[p];
    if (mode == MODE_SOURCE) { times[f] = (double)ev[a].x; return; }
    long long s, e;
    if (mode == MODE_COUNT) { s = k * count_per_frame; e = s + count_per_frame; }
    else { s = k ? seg_end[f - 1] : 0; e = seg_end[f]; }
    s = min(max(s, 0ll), last);
    e = min(max(e, 0ll), last);
    times[f] = (double)((ev[a + s].x + ev[a + e].x) / 2.0f);
}

struct RunArgs {
    const float4 *ev;
    long long n_rows;          // off[P]
    const long long *off;      // [P + 1]
    int P, mode;
    const double *bounds;      // DURATION: packet p's T_0 .. T_m at pkt_f0[p] + p
    long long count_per_frame; // COUNT
    const int *seg_end;        // AREA_COUNT: packet p's window ends at pkt_f0[p]
    const int *pkt_f0;         // [P + 1]
    int complete_base;         // plane of complete frame 0, or -1: complete frames are not accumulated
    int open_plane;            // plane of the last packet's open frame, or -1
    int *diff;
    int bins_y, bins_x;
    double y_lo, x_lo, delta_y, delta_x;
};

// k_render_hist for a whole run: the event finds its packet by binary search over the packet offsets, then its window inside
// the packet by k_render_hist's rule, and adds +-1 to the plane of its global frame.
__global__ __launch_bounds__(256) void k_run_hist(RunArgs r)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n_rows) return;
    const int p = count_le<long long>(r.off, r.P + 1, i) - 1;
    if (p < 0 || p >= r.P) return;
    const long long li = i - r.off[p], n = r.off[p + 1] - r.off[p];
    if (li >= n - 1) return; // the packet's last event is never accumulated (renderer.py:303-306)
    const float4 e = r.ev[i];
    const double fi = ((double)e.z - r.y_lo) * r.delta_y;
    const double fj = ((double)e.y - r.x_lo) * r.delta_x;
    if (!(fi >= 0.0 && fi < (double)r.bins_y && fj >= 0.0 && fj < (double)r.bins_x)) return;
    const int bin = (int)fi * r.bins_x + (int)fj;
    const int v = e.w == 1.0f ? 1 : -1;
    const int f0 = r.pkt_f0[p], m = r.pkt_f0[p + 1] - f0; // complete frames of this packet
    long long k0 = 0, k1 = -1;
    if (r.mode == MODE_DURATION) {
        const double *b = r.bounds + f0 + p;
        const double t = (double)e.x;
        k0 = count_le<double>(b, m + 1, t) - 1;
        if (k0 >= 1 && b[k0] == t) k1 = k0 - 1;
    } else if (r.mode == MODE_COUNT) {
        k0 = li / r.count_per_frame;
    } else if (r.mode == MODE_AREA_COUNT) {
        k0 = count_le<int>(r.seg_end + f0, m, (int)li);
    }
    const size_t npx = (size_t)r.bins_y * r.bins_x;
    const bool open_kept = p == r.P - 1 && r.open_plane >= 0;
    if (k0 >= 0 && k0 < m) { if (r.complete_base >= 0) atomicAdd(&r.diff[(size_t)(r.complete_base + f0 + k0) * npx + bin], v); }
    else if (k0 == m && open_kept) atomicAdd(&r.diff[(size_t)r.open_plane * npx + bin], v);
    if (k1 >= 0 && k1 < m && r.complete_base >= 0) atomicAdd(&r.diff[(size_t)(r.complete_base + f0 + k1) * npx + bin], v);
}

// planes 0 .. n_complete-1: (clip(diff) + fs) / (2 fs) as float64, or the bytes (img * 255).astype(uint8) the reference hands its
// AVI writer (renderer.py:339); plane n_complete (if cur): clip(diff), the frame the run ends in
template <bool U8>
__global__ __launch_bounds__(256) void k_run_finish(const int *__restrict__ diff, long long total, long long n_complete_px,
                                                   double *__restrict__ frames, unsigned char *__restrict__ frames_u8,
                                                   double *__restrict__ cur, double fs)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    double v = (double)diff[i];
    v = v < -fs ? -fs : (v > fs ? fs : v);
    if (i < n_complete_px) {
        const double img = (v + fs) / (fs * 2);
        if (U8) frames_u8[i] = (unsigned char)(img * 255.0);
        else frames[i] = img;
    } else if (cur) cur[i - n_complete_px] = v;
}

} // namespace

extern "C" {

int v2e_render_area_segments(const float *events, int64_t n, int32_t *area_counts, int nw, int nh, double area_dimension, int area_count,
                             int32_t *seg_end, int64_t cap, int32_t *out2, void *stream)
{
    V2E_REQUIRE(events && area_counts && seg_end && out2 && n > 0 && nw > 0 && nh > 0 && area_count >= 2 && area_dimension > 0, "bad args");
    V2E_REQUIRE((size_t)nw * nh * sizeof(int) <= 64 * 1024, "too many area cells for the LDS counter table (64 KB)");
    k_area_segments<<<1, 64, (size_t)nw * nh * sizeof(int), (hipStream_t)stream>>>((const float4 *)events, n, area_counts, nw, nh,
                                                                                (float)area_dimension, area_count, seg_end, cap, out2);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_render_packet(const float *events, int64_t n_used, int mode, const double *bounds, int n_bounds, int64_t count_per_frame,
                      const int32_t *seg_end, int n_seg, int n_complete, int has_open, int32_t *diff, double *frames_out,
                      double *cur_out, int bins_y, int bins_x, double y_lo, double y_hi, double x_lo, double x_hi, double full_scale,
                      void *stream)
{
    V2E_REQUIRE(diff && bins_y > 0 && bins_x > 0 && n_complete >= 0 && (events || n_used == 0) && full_scale > 0, "bad args");
    V2E_REQUIRE(mode >= MODE_DURATION && mode <= MODE_SOURCE, "bad exposure mode");
    V2E_REQUIRE(mode != MODE_DURATION || (bounds && n_bounds >= 1), "DURATION needs the frame boundaries");
    V2E_REQUIRE(mode != MODE_COUNT || count_per_frame >= 1, "COUNT needs a positive event count");
    V2E_REQUIRE(mode != MODE_AREA_COUNT || seg_end || n_seg == 0, "AREA_COUNT needs the segment ends");
    V2E_REQUIRE(n_complete == 0 || frames_out, "null frames_out");
    const int n_frames = n_complete + (has_open ? 1 : 0);
    if (n_frames == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long npx = (long long)bins_y * bins_x, total = npx * n_frames;
    k_zero_i32<<<v2e_cdiv(total, 256), 256, 0, s>>>(diff, total);
    if (n_used > 0) {
        RenderArgs r;
        r.ev = (const float4 *)events; r.n_used = n_used; r.mode = mode; r.bounds = bounds; r.n_bounds = n_bounds;
        r.count_per_frame = count_per_frame; r.seg_end = seg_end; r.n_seg = n_seg; r.n_frames = n_frames; r.diff = diff;
        r.bins_y = bins_y; r.bins_x = bins_x; r.y_lo = y_lo; r.x_lo = x_lo;
        r.delta_y = 1 / ((y_hi - y_lo) / bins_y); r.delta_x = 1 / ((x_hi - x_lo) / bins_x); // v2e_utils.py:478
        k_render_hist<<<v2e_cdiv(n_used, 256), 256, 0, s>>>(r);
    }
    k_render_finish<<<v2e_cdiv(total, 256), 256, 0, s>>>(diff, total, npx, n_complete, frames_out, has_open ? cur_out : nullptr, full_scale);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_render_run_windows(const float *events, const int64_t *pkt_off, int n_packets, double interval, int f32_time, double *time_state,
                           int commit, int32_t *pkt_frame0, double *bounds, int64_t cap_bounds, double *frame_times, int64_t cap_times,
                           int64_t max_frames, int32_t *out2, void *stream)
{
    V2E_REQUIRE(events && pkt_off && n_packets > 0 && time_state && pkt_frame0 && out2 && max_frames > 0, "bad args");
    V2E_REQUIRE((bounds || cap_bounds == 0) && (frame_times || cap_times == 0) && cap_bounds >= 0 && cap_times >= 0, "bad tables");
    k_run_windows_duration<<<1, 64, 0, (hipStream_t)stream>>>((const float4 *)events, (const long long *)pkt_off, n_packets, interval,
                                                             f32_time, time_state, commit, pkt_frame0, bounds, cap_bounds, frame_times,
                                                             cap_times, max_frames, out2);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_render_run_area_segments(const float *events, const int64_t *pkt_off, int n_packets, int32_t *area_counts, int nw, int nh,
                                 double area_dimension, int area_count, int32_t *seg_end, int64_t cap, int32_t *pkt_frame0,
                                 int32_t *out2, void *stream)
{
    V2E_REQUIRE(events && pkt_off && n_packets > 0 && area_counts && seg_end && pkt_frame0 && out2 && nw > 0 && nh > 0 &&
                area_count >= 2 && area_dimension > 0, "bad args");
    V2E_REQUIRE((size_t)nw * nh * sizeof(int) <= 64 * 1024, "too many area cells for the LDS counter table (64 KB)");
    k_run_area_segments<<<1, 64, (size_t)nw * nh * sizeof(int), (hipStream_t)stream>>>((const float4 *)events, (const long long *)pkt_off,
                                                                                    n_packets, area_counts, nw, nh, (float)area_dimension,
                                                                                    area_count, seg_end, cap, pkt_frame0, out2);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_render_run_frame_times(const float *events, const int64_t *pkt_off, int n_packets, int mode, int64_t count_per_frame,
                               const int32_t *seg_end, const int32_t *pkt_frame0, int n_frames, double *frame_times, void *stream)
{
    V2E_REQUIRE(events && pkt_off && n_packets > 0 && pkt_frame0 && n_frames >= 0 && (frame_times || n_frames == 0), "bad args");
    V2E_REQUIRE(mode == MODE_COUNT || mode == MODE_AREA_COUNT || mode == MODE_SOURCE, "DURATION frame times come from v2e_render_run_windows");
    V2E_REQUIRE(mode != MODE_COUNT || count_per_frame >= 1, "COUNT needs a positive event count");
    V2E_REQUIRE(mode != MODE_AREA_COUNT || seg_end || n_frames == 0, "AREA_COUNT needs the segment ends");
    if (n_frames == 0) return 0;
    k_run_frame_times<<<v2e_cdiv(n_frames, 256), 256, 0, (hipStream_t)stream>>>((const float4 *)events, (const long long *)pkt_off, n_packets,
                                                                               mode, count_per_frame, seg_end, pkt_frame0, n_frames,
                                                                               frame_times);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_render_run(const float *events, int64_t n_rows, const int64_t *pkt_off, int n_packets, int mode, const double *bounds,
                   int64_t count_per_frame, const int32_t *seg_end, const int32_t *pkt_frame0, int n_complete, int has_open,
                   int want_frames, int32_t *diff, double *frames_out, uint8_t *frames_u8_out, double *cur_out, int bins_y, int bins_x,
                   double y_lo, double y_hi, double x_lo, double x_hi, double full_scale, void *stream)
{
    V2E_REQUIRE(events && n_rows > 0 && pkt_off && n_packets > 0 && pkt_frame0 && diff && bins_y > 0 && bins_x > 0 && n_complete >= 0 &&
                full_scale > 0, "bad args");
    V2E_REQUIRE(mode >= MODE_DURATION && mode <= MODE_SOURCE, "bad exposure mode");
    V2E_REQUIRE(mode != MODE_DURATION || bounds, "DURATION needs the frame boundaries");
    V2E_REQUIRE(mode != MODE_COUNT || count_per_frame >= 1, "COUNT needs a positive event count");
    V2E_REQUIRE(mode != MODE_AREA_COUNT || seg_end || n_complete == 0, "AREA_COUNT needs the segment ends");
    V2E_REQUIRE(!want_frames || n_complete == 0 || ((frames_out != nullptr) != (frames_u8_out != nullptr)), "one of the two frame outputs");
    V2E_REQUIRE(!has_open || cur_out, "null cur_out");
    const int planes_complete = want_frames ? n_complete : 0;
    const int planes = planes_complete + (has_open ? 1 : 0);
    if (planes == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long npx = (long long)bins_y * bins_x, total = npx * planes;
    k_zero_i32<<<v2e_cdiv(total, 256), 256, 0, s>>>(diff, total);
    RunArgs r;
    r.ev = (const float4 *)events; r.n_rows = n_rows; r.off = (const long long *)pkt_off; r.P = n_packets; r.mode = mode;
    r.bounds = bounds; r.count_per_frame = count_per_frame; r.seg_end = seg_end; r.pkt_f0 = pkt_frame0;
    r.complete_base = want_frames ? 0 : -1; r.open_plane = has_open ? planes_complete : -1; r.diff = diff;
    r.bins_y = bins_y; r.bins_x = bins_x; r.y_lo = y_lo; r.x_lo = x_lo;
    r.delta_y = 1 / ((y_hi - y_lo) / bins_y); r.delta_x = 1 / ((x_hi - x_lo) / bins_x); // v2e_utils.py:478
    k_run_hist<<<v2e_cdiv(n_rows, 256), 256, 0, s>>>(r);
    if (frames_u8_out)
        k_run_finish<true><<<v2e_cdiv(total, 256), 256, 0, s>>>(diff, total, npx * planes_complete, nullptr, frames_u8_out,
                                                                has_open ? cur_out : nullptr, full_scale);
    else
        k_run_finish<false><<<v2e_cdiv(total, 256), 256, 0, s>>>(diff, total, npx * planes_complete, frames_out, nullptr,
                                                                 has_open ? cur_out : nullptr, full_scale);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
