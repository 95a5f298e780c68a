// dwindow.hip -- the double-window filter (DWF of the DND21 denoising benchmark, jAER's DoubleWindowFilter) scored for every
// (L, sigma, k) of three tables over the rows of a device-resident run (host side: v2e_amd/dwindow.py, DoubleWindowSweep).
//
// A setting owns two windows, R ("real") and N ("noise"), of at most L rows each, both empty at first.  A valid row at (x, y)
// passes iff c = #{w in R u N : |x - w.x| + |y - w.y| <= sigma} >= k (L1 distance; a row at the same pixel counts); a passing row
// is appended to R, a failing one to N, and a window that now holds L + 1 rows drops its oldest.  The verdict feeds back into the
// windows, so one setting is a serial chain over the rows -- but the settings of a sweep are independent chains.
//
// One wavefront per setting.  A pass's valid rows are compacted by window.hip's kernels (v2e_window_compact with lmax = 1: the
// words x | y << 16 in order behind one unused word, and each word's row index); k_dwindow_labels puts each compacted row's label
// beside its word and adds the pass's signal / noise totals.  k_dwindow_sweep then runs F = NK * S * NL workgroups of one wave:
// wave f holds the 2 L words of setting f on chip, takes the pass's words 64 at a time (lane i loads word base + i and its label;
// the next chunk's loads are issued before this chunk is walked), and inside a chunk goes row by row with wave-uniform control
// flow: the row's word is broadcast, every lane compares its share of the window words, one ballot + population count per 64
// words gives c, the walk stops at c >= k, the verdict goes into a uniform 64-bit mask and the word into its window.  No wave
// waits for another, so F may exceed what is resident.  One wave owns a setting's counters and every sum is an integer: the
// result depends on the row order only.
//
// State between passes, in device memory: rings (uint32 [F][2][lmax]; window R of setting f is a ring of L slots at
// rings[f][0][0 .. L), N at rings[f][1][0 .. L), XY_NONE in a slot that holds no row yet and in the slots from L on) and pos
// (int32 [F][2]: the slot the next row of that window goes to, which is also its oldest).  A ring fills from slot 0, so the fill
// needs no counter of its own: the empty slots are pos .. L - 1 while any slot is empty.
#include "common.h"
#include "block_ops.h"
#include "rowkeys.h"

namespace {

constexpr int MAX_LENGTHS = 64, MAX_LENGTH = 512, MAX_SIGMAS = 8, MAX_SUPPORT = 4;
constexpr unsigned int XY_NONE = 0xffffffffu;               // (x, y) = (65535, 65535): no sensor has that pixel (H, W <= 65535)
constexpr int LDS_READS = 4;                                // window words per lane read from LDS before the first is used

// lab[r] = the label of the pass's r-th valid row (1 signal, 0 noise); totals[label] += the pass's valid rows of that label
__global__ __launch_bounds__(256) void k_dwindow_labels(const int *__restrict__ idx, int n, const int *__restrict__ n_valid,
                                                        const unsigned char *__restrict__ labels, const long long *__restrict__ lbounds,
                                                        int n_lbounds, long long row0, unsigned char *__restrict__ lab,
                                                        unsigned long long *__restrict__ totals)
{
    __shared__ int s[4];
    const int nv = n_valid[0] < n ? n_valid[0] : n;            // no read past the pass's words, whatever n_valid holds
    const int r = blockIdx.x * 256 + threadIdx.x;
    const bool active = r < nv;
    int label = 1;
    if (active) {
        const int i = idx[r];
        label = row_label(labels, lbounds, n_lbounds, row0, i);
        lab[r] = (unsigned char)label;
    }
    const int c1 = block_count(active && label == 1, s, 4);
    const int c0 = block_count(active && label == 0, s, 4);
    if (threadIdx.x == 0) {
        if (c0) atomicAdd(&totals[0], (unsigned long long)c0);
        if (c1) atomicAdd(&totals[1], (unsigned long long)c1);
    }
}

struct SweepArgs {
    const unsigned int *xy;      // [1 + n]: one unused word, then the pass's valid rows
    const int *idx;              // [n]: the row of the pass behind each compacted word
    const unsigned char *lab;    // [n]: the label of each compacted word
    int n;                       // rows of this pass
    const int *n_valid;          // [1]
    int NL, S, lmax;
    int length[MAX_LENGTHS], sigma[MAX_SIGMAS], support[MAX_SUPPORT];
    unsigned int *rings;         // [F][2][lmax]
    int *pos;                    // [F][2]
    unsigned long long *passed;  // [F][2]
    unsigned char *keep;         // [n] or null
    int keep_f;                  // the setting whose verdicts keep gets
};

// The number of lanes whose window word w lies within sigma of the row's word; called by the whole wave.  v_sad_u16 is
// |lo - lo| + |hi - hi| of the packed halves in one step; two ballots of plain compares and a scalar AND cost less than one
// ballot of their conjunction, which goes through a register.
__device__ __forceinline__ int count_near(unsigned int w, unsigned int row, unsigned int sigma)
{
    const unsigned long long near = __builtin_amdgcn_ballot_w64(__builtin_amdgcn_sad_u16(w, row, 0u) <= sigma);
    return (int)__popcll(near & __builtin_amdgcn_ballot_w64(w != XY_NONE));
}

// slot i of a setting's 2 L window words (R, then N) in the carried rings
__device__ __forceinline__ unsigned int *ring_slot(unsigned int *rings, int f, int lmax, int L, int i)
{
    return rings + (size_t)(2 * f + (i < L ? 0 : 1)) * lmax + (i < L ? i : i - L);
}

// The two windows in LDS: 2 L words, XY_NONE up to the next multiple of 64 * LDS_READS.  One lane writes a new word; the wave's
// LDS operations keep their order, so the next row's reads see it.  Measured against 2 L / 64 registers per lane with a
// wave-uniform switch for the insertion and a test of c after every 64 words (profiles/r28_double_window_sweep.txt): the
// registers took 1.46 times as long at Lmax = 512 and 1.29 times at Lmax = 64, and are gone.
struct LdsWindows {
    unsigned int *s;
    __device__ __forceinline__ void load(unsigned int *rings, int f, int lmax, int L, int lane)
    {
        extern __shared__ unsigned int s_win[];
        s = s_win;
        const int cap = (2 * L + 64 * LDS_READS - 1) / (64 * LDS_READS) * (64 * LDS_READS);
        for (int i = lane; i < cap; i += 64) s[i] = i < 2 * L ? *ring_slot(rings, f, lmax, L, i) : XY_NONE;
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void store(unsigned int *rings, int f, int lmax, int L, int lane) const
    {
        for (int i = lane; i < 2 * L; i += 64) *ring_slot(rings, f, lmax, L, i) = s[i];
    }
    // c, or a partial count that has reached k: the walk over the 2 L words stops behind the group of reads that brings it there
    __device__ __forceinline__ int count(unsigned int row, unsigned int sigma, int k, int L, int lane) const
    {
        int c = 0;
        for (int t = 0; t < 2 * L; t += 64 * LDS_READS) {
            unsigned int w[LDS_READS];
#pragma unroll
            for (int u = 0; u < LDS_READS; ++u) w[u] = s[t + 64 * u + lane];
#pragma unroll
            for (int u = 0; u < LDS_READS; ++u) c += count_near(w[u], row, sigma);
            if (c >= k) break; // (once per group of reads: a test per word would have each read wait for the one before)
        }
        return c;
    }
    __device__ __forceinline__ void insert(int slot, unsigned int row, int lane)
    {
        if (lane == 0) s[slot] = row;
        __builtin_amdgcn_wave_barrier();
    }
};

// One workgroup of one wave per setting f = (ki * S + s) * NL + li.
__global__ __launch_bounds__(64) void k_dwindow_sweep(SweepArgs r)
{
    const int lane = threadIdx.x, f = blockIdx.x;
    const int li = f % r.NL, si = (f / r.NL) % r.S, ki = f / (r.NL * r.S);
    const int L = r.length[li], k = r.support[ki];
    const unsigned int sigma = (unsigned int)r.sigma[si];
    const int nv_dev = __builtin_amdgcn_readfirstlane(r.n_valid[0]);
    const int nv = nv_dev < r.n ? nv_dev : r.n;                // no read past the pass's words, whatever n_valid holds
    if (nv <= 0) return;
    const unsigned int *words = r.xy + 1;
    const bool keeps = r.keep && f == r.keep_f;
    LdsWindows win;
    win.load(r.rings, f, r.lmax, L, lane);
    int pos_r = __builtin_amdgcn_readfirstlane(r.pos[2 * f]), pos_n = __builtin_amdgcn_readfirstlane(r.pos[2 * f + 1]);
    if ((unsigned int)pos_r >= (unsigned int)L) pos_r = 0;     // no slot outside the window, whatever pos holds
    if ((unsigned int)pos_n >= (unsigned int)L) pos_n = 0;
    unsigned long long passed_signal = 0, passed_noise = 0;
    unsigned int cur_w = lane < nv ? words[lane] : XY_NONE;
    unsigned int cur_l = lane < nv ? r.lab[lane] : 0u;

    for (int base = 0; base < nv; base += 64) {
        const int nxt = base + 64 + lane;                      // the next chunk's loads, in flight while this chunk is walked
        const unsigned int nxt_w = nxt < nv ? words[nxt] : XY_NONE;
        const unsigned int nxt_l = nxt < nv ? r.lab[nxt] : 0u;
        const int cnt = nv - base < 64 ? nv - base : 64;
        unsigned long long mask = 0;
        for (int j = 0; j < cnt; ++j) {
            const unsigned int row = (unsigned int)__builtin_amdgcn_readlane((int)cur_w, j);
            const bool pass = win.count(row, sigma, k, L, lane) >= k;
            if (pass) {
                mask |= 1ull << j;
                win.insert(pos_r, row, lane);
                pos_r = pos_r + 1 == L ? 0 : pos_r + 1;
            } else {
                win.insert(L + pos_n, row, lane);
                pos_n = pos_n + 1 == L ? 0 : pos_n + 1;
            }
        }
        const unsigned long long signal = __ballot(cur_l != 0u);   // (a lane behind the pass's last row holds label 0 and verdict 0)
        passed_signal += (unsigned long long)__popcll(mask & signal);
        passed_noise += (unsigned long long)__popcll(mask & ~signal);
        if (keeps && lane < cnt) r.keep[r.idx[base + lane]] = (unsigned char)((mask >> lane) & 1ull);
        cur_w = nxt_w;
        cur_l = nxt_l;
    }
    win.store(r.rings, f, r.lmax, L, lane);
    if (lane == 0) {
        r.pos[2 * f] = pos_r;
        r.pos[2 * f + 1] = pos_n;
        r.passed[2 * f] += passed_noise;
        r.passed[2 * f + 1] += passed_signal;
    }
}

} // namespace

extern "C" {

int v2e_dwindow_labels(const int32_t *idx, int64_t n, const int32_t *n_valid, const uint8_t *labels, const int64_t *label_bounds,
                       int n_label_bounds, int64_t row0, uint8_t *lab, uint64_t *totals, void *stream)
{
    V2E_REQUIRE(n >= 1 && n <= (1 << 30) && idx && n_valid && lab && totals && row0 >= 0, "bad args");
    V2E_REQUIRE_LABELS(labels, label_bounds, n_label_bounds);
    V2E_REQUIRE(((uintptr_t)totals & 7u) == 0 && ((uintptr_t)idx & 3u) == 0 && ((uintptr_t)n_valid & 3u) == 0, "counters and indices must be aligned");
    k_dwindow_labels<<<v2e_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(idx, (int)n, n_valid, labels, (const long long *)label_bounds,
                                                                         label_bounds ? n_label_bounds : 0, row0, lab,
                                                                         (unsigned long long *)totals);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_dwindow_sweep(const uint32_t *xy, const int32_t *idx, const uint8_t *lab, int64_t n, const int32_t *n_valid, const int32_t *lengths,
                      int n_lengths, const int32_t *sigmas, int n_sigmas, const int32_t *supports, int n_supports, uint32_t *rings,
                      int32_t *pos, uint64_t *passed, uint8_t *keep, int keep_length, int keep_sigma, int keep_support, void *stream)
{
    V2E_REQUIRE(n >= 1 && n <= (1 << 30) && xy && idx && lab && n_valid && lengths && sigmas && supports && rings && pos && passed, "bad args");
    V2E_REQUIRE(n_lengths >= 1 && n_lengths <= MAX_LENGTHS && n_sigmas >= 1 && n_sigmas <= MAX_SIGMAS && n_supports >= 1 &&
                n_supports <= MAX_SUPPORT, "1 to 64 lengths, 1 to 8 sigmas, 1 to 4 supports");
    V2E_REQUIRE(((uintptr_t)xy & 3u) == 0 && ((uintptr_t)idx & 3u) == 0 && ((uintptr_t)n_valid & 3u) == 0 && ((uintptr_t)rings & 3u) == 0 &&
                ((uintptr_t)pos & 3u) == 0 && ((uintptr_t)passed & 7u) == 0, "words, indices and counters must be aligned");
    SweepArgs r;
    r.xy = xy; r.idx = idx; r.lab = lab; r.n = (int)n; r.n_valid = n_valid; r.NL = n_lengths; r.S = n_sigmas;
    for (int i = 0; i < n_lengths; ++i) {
        V2E_REQUIRE(lengths[i] >= 1 && lengths[i] <= MAX_LENGTH && (i == 0 || lengths[i] > lengths[i - 1]), "lengths: 1 .. 512, strictly ascending");
        r.length[i] = lengths[i];
    }
    for (int i = 0; i < n_sigmas; ++i) {
        V2E_REQUIRE(sigmas[i] >= 0 && sigmas[i] <= 65535 && (i == 0 || sigmas[i] > sigmas[i - 1]), "sigmas: 0 .. 65535, strictly ascending");
        r.sigma[i] = sigmas[i];
    }
    for (int i = 0; i < n_supports; ++i) {
        V2E_REQUIRE(supports[i] >= 1 && supports[i] <= MAX_SUPPORT && (i == 0 || supports[i] > supports[i - 1]), "supports: 1 .. 4, strictly ascending");
        r.support[i] = supports[i];
    }
    r.lmax = lengths[n_lengths - 1];
    r.rings = rings; r.pos = pos; r.passed = (unsigned long long *)passed; r.keep = keep; r.keep_f = -1;
    if (keep) {
        V2E_REQUIRE(keep_length >= 0 && keep_length < n_lengths && keep_sigma >= 0 && keep_sigma < n_sigmas && keep_support >= 0 &&
                    keep_support < n_supports, "keep: the indices of its L, sigma and k in the three tables");
        r.keep_f = (keep_support * n_sigmas + keep_sigma) * n_lengths + keep_length;
    }
    const int F = n_supports * n_sigmas * n_lengths;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)((2 * r.lmax + 64 * LDS_READS - 1) / (64 * LDS_READS) * (64 * LDS_READS)) * 4;
    k_dwindow_sweep<<<F, 64, lds, s>>>(r);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
