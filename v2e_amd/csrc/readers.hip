// readers.hip -- event files read back into device rows: the inverse of sinks.hip.
//   AEDAT-2.0  v2ecore/output/aedat2_output.py:155-173 inverted (jAER: big-endian int32 address, int32 timestamp in us)
//   text       v2ecore/output/ae_text_output.py:86-101 inverted (`t x y p[ label]` lines; text_parse.h)
// A recording holds records that are not rows (APS / IMU samples, special events, comment and malformed lines), so both decoders
// are an ordered compaction over blocks of V2E_READER_BLOCK items: the kept items counted per block, an exclusive scan of the
// block counts by one workgroup, and a write pass in which an item's place is its block's base plus the kept items before it in
// the block (block_ops.h: block_sum, block_bases, block_rank).  The text decoder runs that twice: over the bytes for the
// line starts, then over the lines -- parsed one per lane from LDS where a block's lines fit -- for the rows.  Counters are
// integer block sums added with integer atomics: every result is the same from run to run.
#include "common.h"
#include "block_ops.h"
#include "text_parse.h"

namespace {

constexpr int RB = V2E_READER_BLOCK;
constexpr int RB_WAVES = RB / 64;
constexpr int NL_BYTES = 16;                  // bytes per lane of the newline passes
constexpr int NL_BLOCK_BYTES = RB * NL_BYTES; // 16 KiB per workgroup
constexpr int LINE_BLOCK = 256;               // lines per workgroup of the parse pass
constexpr int STAGE_BYTES = 16384;            // LDS for a workgroup's lines (64 bytes per line; longer ones are read from HBM)

typedef unsigned long long u64;

__device__ __forceinline__ void add_counter(int64_t *c, long long v)
{
    if (v) atomicAdd((u64 *)c, (u64)v);
}

// exclusive scan of blk[0 .. nblk) in place by one workgroup, the total to *total
__global__ __launch_bounds__(1024) void k_rd_scan(long long *__restrict__ blk, int nblk, long long *__restrict__ total)
{
    __shared__ long long s_part[1024];
    const long long t = block_bases(blk, nblk, s_part);
    if (threadIdx.x == 1023) *total = t;
}

// ------------------------------------------------------------------------------------------------------------- AEDAT-2.0
struct A2Layout { int sizex, sizey, xshift, yshift, pshift, flipx, flipy, special_mode; }; // special_mode 2: bit 10 is data

enum { A2_ROW = 0, A2_APS = 1, A2_SPECIAL = 2 };

__device__ __forceinline__ int a2_class(uint32_t addr, int special_mode)
{
    if (addr >> 31) return A2_APS;
    if (((addr >> 10) & 1u) && !special_mode) return A2_SPECIAL;
    return A2_ROW;
}

__host__ __device__ __forceinline__ uint32_t coord_mask(int size) // the bits that hold 0 .. size - 1
{
    uint32_t m = 1;
    while ((int)m < size) m <<= 1;
    return m - 1;
}

__global__ __launch_bounds__(RB) void k_a2_count(const uint2 *__restrict__ rec, int64_t n, A2Layout L, long long *__restrict__ blk,
                                                 int64_t *__restrict__ counters)
{
    __shared__ int s[RB_WAVES];
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    int cls = -1, outside = 0;
    if (i < n) {
        const uint32_t a = __builtin_bswap32(rec[i].x);
        cls = a2_class(a, L.special_mode);
        if (cls == A2_ROW) {
            int x = (int)((a >> L.xshift) & coord_mask(L.sizex)), y = (int)((a >> L.yshift) & coord_mask(L.sizey));
            outside = x >= L.sizex || y >= L.sizey; // (the flips map the range onto itself)
        }
    }
    const int kept = block_sum(cls == A2_ROW, s), aps = block_sum(cls == A2_APS, s), spec = block_sum(cls == A2_SPECIAL, s),
              out = block_sum(outside, s);
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = kept;
        add_counter(counters + V2E_A2C_APS, aps);
        add_counter(counters + V2E_A2C_SPECIAL, spec);
        add_counter(counters + V2E_A2C_OUTSIDE, out);
    }
}

__global__ __launch_bounds__(RB) void k_a2_write(const uint2 *__restrict__ rec, int64_t n, A2Layout L, const long long *__restrict__ blk_base,
                                                 float4 *__restrict__ rows, uint8_t *__restrict__ labels, int64_t *__restrict__ t_us,
                                                 int32_t *__restrict__ ts_kept)
{
    __shared__ int s[RB_WAVES];
    const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
    uint32_t a = 0;
    int32_t ts = 0;
    bool keep = false;
    if (i < n) {
        const uint2 r = rec[i];
        a = __builtin_bswap32(r.x);
        ts = (int32_t)__builtin_bswap32(r.y);
        keep = a2_class(a, L.special_mode) == A2_ROW;
    }
    const int before = block_rank(keep, s);
    if (!keep) return;
    const int64_t o = blk_base[blockIdx.x] + before; // < the number of kept records <= n
    int x = (int)((a >> L.xshift) & coord_mask(L.sizex)), y = (int)((a >> L.yshift) & coord_mask(L.sizey));
    if (L.flipx) x = (L.sizex - 1) - x;
    if (L.flipy) y = (L.sizey - 1) - y;
    const double t = (double)ts * 1e-6; // one float64 product, one rounding to float32
    rows[o] = make_float4((float)t, (float)x, (float)y, ((a >> L.pshift) & 1u) ? 1.0f : -1.0f);
    if (labels) labels[o] = ((a >> 10) & 1u) ? 0 : 1; // the special-event bit marks noise (label_signal_noise)
    if (t_us) t_us[o] = (int64_t)ts;
    ts_kept[o] = ts;
}

// kept records whose time stamp is below the one before them; the first one looks at the last record of the call before
__global__ __launch_bounds__(RB) void k_a2_order(const int32_t *__restrict__ ts_kept, const long long *__restrict__ n_kept,
                                                 int64_t *__restrict__ counters)
{
    __shared__ int s[RB_WAVES];
    const int64_t n = *n_kept, i = (int64_t)blockIdx.x * RB + threadIdx.x;
    int back = 0;
    if (i < n) {
        if (i > 0) back = ts_kept[i] < ts_kept[i - 1];
        else if (counters[V2E_A2C_HAVE_LAST]) back = (int64_t)ts_kept[0] < counters[V2E_A2C_LAST_TS];
    }
    const int t = block_sum(back, s);
    if (threadIdx.x == 0) add_counter(counters + V2E_A2C_NONMONOTONIC, t);
}

// after k_a2_order has read the carried time stamp: the call's totals and the time stamp the next call carries
__global__ void k_a2_finish(const int32_t *__restrict__ ts_kept, const long long *__restrict__ n_kept, int64_t *__restrict__ counters)
{
    const int64_t n = *n_kept;
    counters[V2E_A2C_ROWS] += n;
    counters[V2E_A2C_CALL_ROWS] = n;
    if (n > 0) { counters[V2E_A2C_LAST_TS] = ts_kept[n - 1]; counters[V2E_A2C_HAVE_LAST] = 1; }
}

// ------------------------------------------------------------------------------------------------------------------ text
// the 16 bytes of lane j of the newline passes as a mask of its '\n' (bit k: byte 16 j + k); bytes past n_bytes are not read
__device__ __forceinline__ uint32_t newline_mask(const char *__restrict__ bytes, int64_t n_bytes, int64_t j)
{
    const int64_t b0 = j * NL_BYTES;
    uint32_t m = 0;
    if (b0 + NL_BYTES <= n_bytes) {
        const uint4 v = *(const uint4 *)(bytes + b0); // bytes is 16-byte aligned
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int q = 0; q < 4; ++q)
            for (int k = 0; k < 4; ++k)
                if (((w[q] >> (8 * k)) & 0xFFu) == (uint32_t)'\n') m |= 1u << (4 * q + k);
    } else {
        for (int k = 0; b0 + k < n_bytes; ++k)
            if (bytes[b0 + k] == '\n') m |= 1u << k;
    }
    return m;
}

__global__ __launch_bounds__(RB) void k_txt_count_newlines(const char *__restrict__ bytes, int64_t n_bytes, long long *__restrict__ blk)
{
    __shared__ int s[RB_WAVES];
    const int64_t j = (int64_t)blockIdx.x * RB + threadIdx.x;
    const int c = j * NL_BYTES < n_bytes ? __popc(newline_mask(bytes, n_bytes, j)) : 0;
    const int t = block_sum(c, s);
    if (threadIdx.x == 0) blk[blockIdx.x] = t;
}

// line_start[0] = 0, line_start[1 + r] = the byte after the r-th '\n' (for the last byte of the text: n_bytes, the end mark);
// nothing is written when the text has more than cap_lines lines
__global__ __launch_bounds__(RB) void k_txt_line_starts(const char *__restrict__ bytes, int64_t n_bytes, const long long *__restrict__ blk_base,
                                                        const long long *__restrict__ n_newlines, int64_t cap_lines,
                                                        int64_t *__restrict__ line_start)
{
    __shared__ int s_cnt[RB];
    const int64_t nl = *n_newlines;
    if (nl > cap_lines) return; // line_start holds cap_lines + 1 entries: 0 .. nl
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * RB + tid;
    const uint32_t m = j * NL_BYTES < n_bytes ? newline_mask(bytes, n_bytes, j) : 0u;
    const int c = __popc(m);
    s_cnt[tid] = c;
    block_scan<RB>(s_cnt); // inclusive scan of the lanes' counts
    int64_t r = blk_base[blockIdx.x] + (s_cnt[tid] - c);
    if (j == 0) line_start[0] = 0;
    for (uint32_t mm = m; mm; mm &= mm - 1) {
        const int k = __ffs(mm) - 1;
        line_start[1 + r] = j * NL_BYTES + k + 1; // 1 + r <= nl <= cap_lines
        ++r;
    }
}

// the number of lines of the text: one per '\n', and a last one without
__device__ __forceinline__ int64_t text_lines(const char *bytes, int64_t n_bytes, int64_t nl)
{
    return nl + (n_bytes > 0 && bytes[n_bytes - 1] != '\n' ? 1 : 0);
}

// one line per lane: its class and row to status / tmp_rows, the kept lines of the workgroup to blk
__global__ __launch_bounds__(LINE_BLOCK) void k_txt_parse(const char *__restrict__ bytes, int64_t n_bytes, int want_labels,
                                                          const int64_t *__restrict__ line_start, const long long *__restrict__ n_newlines,
                                                          int64_t cap_lines, float4 *__restrict__ tmp_rows, uint8_t *__restrict__ status,
                                                          long long *__restrict__ blk, int64_t *__restrict__ counters)
{
    __shared__ int s[LINE_BLOCK / 64];
    __shared__ __attribute__((aligned(16))) char s_text[STAGE_BYTES];
    const int64_t nl = *n_newlines, nlines = text_lines(bytes, n_bytes, nl);
    if (nlines > cap_lines) { // nothing is decoded: the caller makes room for nlines lines and calls again
        if (threadIdx.x == 0) blk[blockIdx.x] = 0;
        return;
    }
    const int tid = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * LINE_BLOCK, k = k0 + tid;
    if (k0 >= nlines) { if (tid == 0) blk[blockIdx.x] = 0; return; }
    // line k is bytes [line_start[k], end): end = the '\n' before the next line's start, or the text's end for a last line without
    const int64_t k1 = k0 + LINE_BLOCK < nlines ? k0 + LINE_BLOCK : nlines;
    const int64_t a = line_start[k0], b = k1 <= nl ? line_start[k1] : n_bytes;
    const int64_t a16 = a & ~(int64_t)15;
    const bool staged = b - a16 <= STAGE_BYTES;
    if (staged) {
        const int nvec = (int)((b - a16 + 15) >> 4);
        for (int v = tid; v < nvec; v += LINE_BLOCK) {
            const int64_t g = a16 + 16 * (int64_t)v;
            if (g + 16 <= n_bytes) *(uint4 *)(s_text + 16 * v) = *(const uint4 *)(bytes + g);
            else for (int q = 0; g + q < n_bytes; ++q) s_text[16 * v + q] = bytes[g + q];
        }
    }
    __syncthreads();
    int cls = -1;
    if (k < nlines) {
        const int64_t ls = line_start[k], le = k < nl ? line_start[k + 1] - 1 : n_bytes;
        v2e_tp::Row row;
        row.t = row.x = row.y = row.p = 0.f;
        row.label = -1;
        cls = v2e_tp::parse_line(staged ? s_text + (ls - a16) : bytes + ls, le - ls, want_labels, row);
        status[k] = (uint8_t)(cls | (row.label > 0 ? 4 : 0));
        if (cls == v2e_tp::LINE_ROW || cls == v2e_tp::LINE_ROW_FLAGGED) tmp_rows[k] = make_float4(row.t, row.x, row.y, row.p);
    }
    const int kept = block_sum(cls == v2e_tp::LINE_ROW || cls == v2e_tp::LINE_ROW_FLAGGED, s),
              skipped = block_sum(cls == v2e_tp::LINE_SKIP, s), bad = block_sum(cls == v2e_tp::LINE_BAD, s);
    if (tid == 0) {
        blk[blockIdx.x] = kept;
        add_counter(counters + V2E_TXC_COMMENT, skipped);
        add_counter(counters + V2E_TXC_BAD, bad);
    }
}

__global__ __launch_bounds__(LINE_BLOCK) void k_txt_rows(const char *__restrict__ bytes, int64_t n_bytes, const int64_t *__restrict__ line_start,
                                                         const long long *__restrict__ n_newlines, int64_t cap_lines,
                                                         const float4 *__restrict__ tmp_rows, const uint8_t *__restrict__ status,
                                                         const long long *__restrict__ blk_base, float4 *__restrict__ rows,
                                                         uint8_t *__restrict__ labels, int64_t *__restrict__ flagged, int64_t cap_flagged,
                                                         int64_t *__restrict__ counters)
{
    __shared__ int s[LINE_BLOCK / 64];
    const int64_t nlines = text_lines(bytes, n_bytes, *n_newlines);
    if (nlines > cap_lines) return;
    const int64_t k = (int64_t)blockIdx.x * LINE_BLOCK + threadIdx.x;
    int st = 0;
    if (k < nlines) st = status[k];
    const int cls = st & 3;
    const bool keep = k < nlines && (cls == v2e_tp::LINE_ROW || cls == v2e_tp::LINE_ROW_FLAGGED);
    const int before = block_rank(keep, s);
    if (!keep) return;
    const int64_t o = blk_base[blockIdx.x] + before; // < kept lines <= nlines <= cap_lines
    rows[o] = tmp_rows[k];
    if (labels) labels[o] = (uint8_t)(st >> 2);
    if (cls == v2e_tp::LINE_ROW_FLAGGED) { // (the order of this list does not matter: each entry names its line and row)
        const int64_t slot = (int64_t)atomicAdd((u64 *)(counters + V2E_TXC_CALL_FLAGGED), 1ull);
        if (slot < cap_flagged) { flagged[2 * slot] = line_start[k]; flagged[2 * slot + 1] = o; }
    }
}

__global__ void k_txt_begin(int64_t *__restrict__ counters)
{
    counters[V2E_TXC_CALL_ROWS] = -1;
    counters[V2E_TXC_CALL_LINES] = 0;
    counters[V2E_TXC_CALL_FLAGGED] = 0;
}

__global__ void k_txt_finish(const char *__restrict__ bytes, int64_t n_bytes, const long long *__restrict__ n_newlines, int64_t cap_lines,
                             const long long *__restrict__ n_rows, int64_t *__restrict__ counters)
{
    const int64_t nlines = text_lines(bytes, n_bytes, *n_newlines);
    counters[V2E_TXC_CALL_LINES] = nlines;
    if (nlines > cap_lines) return; // CALL_ROWS stays -1, CALL_LINES says how many lines there are
    counters[V2E_TXC_ROWS] += *n_rows;
    counters[V2E_TXC_LINES] += nlines;
    counters[V2E_TXC_FLAGGED] += counters[V2E_TXC_CALL_FLAGGED];
    counters[V2E_TXC_CALL_ROWS] = *n_rows;
}

// scratch of v2e_events_parse_text, in 16-byte units so that every part is aligned
struct TextScratch {
    int64_t nl_blocks, line_blocks;
    int64_t o_total, o_nlblk, o_lnblk, o_starts, o_tmp, o_status, bytes;
    TextScratch(int64_t n_bytes, int64_t cap_lines)
    {
        auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
        nl_blocks = (n_bytes + NL_BLOCK_BYTES - 1) / NL_BLOCK_BYTES;
        line_blocks = (cap_lines + LINE_BLOCK - 1) / LINE_BLOCK;
        o_total = 0;                                    // [0] newlines, [1] rows
        o_nlblk = 16;
        o_lnblk = o_nlblk + up(8 * nl_blocks);
        o_starts = o_lnblk + up(8 * line_blocks);
        o_tmp = o_starts + up(8 * (cap_lines + 1));
        o_status = o_tmp + 16 * cap_lines;
        bytes = o_status + up(cap_lines);
    }
};

} // namespace

extern "C" {

int64_t v2e_events_unpack_aedat2_scratch_bytes(int64_t n_records)
{
    const int64_t nblk = (n_records + RB - 1) / RB;
    return 16 + 8 * nblk + 4 * n_records; // the kept total, the block counts, the kept time stamps
}

int v2e_events_unpack_aedat2(const void *bytes, int64_t n_records, int sizex, int sizey, int xshift, int yshift, int pshift, int flipx,
                             int flipy, int special_mode, float *rows, uint8_t *labels, int64_t *t_us, int64_t *counters, void *scratch,
                             void *stream)
{
    V2E_REQUIRE(counters && scratch && n_records >= 0 && (n_records == 0 || (bytes && rows)), "null");
    V2E_REQUIRE(((uintptr_t)bytes & 7) == 0 && ((uintptr_t)rows & 15) == 0 && ((uintptr_t)scratch & 15) == 0, "unaligned buffer");
    V2E_REQUIRE(sizex > 0 && sizey > 0 && sizex <= (1 << 15) && sizey <= (1 << 15), "bad sensor size");
    V2E_REQUIRE(xshift >= 0 && xshift < 31 && yshift >= 0 && yshift < 31 && pshift >= 0 && pshift < 31, "bad address layout");
    V2E_REQUIRE((special_mode == 0 || special_mode == 1) && (n_records + RB - 1) / RB <= ((int64_t)1 << 30), "bad args");
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (int)((n_records + RB - 1) / RB);
    long long *total = (long long *)scratch, *blk = total + 2;
    int32_t *ts_kept = (int32_t *)(blk + nblk);
    // the 640x480 layout keeps x in bits 1 .. 10: there bit 10 is a coordinate bit and no record is a special event
    const uint32_t fields = (coord_mask(sizex) << xshift) | (coord_mask(sizey) << yshift) | (1u << pshift);
    const bool bit10_is_data = (fields >> 10) & 1u;
    V2E_REQUIRE(!(bit10_is_data && special_mode), "the special-event bit lies inside a field of this layout: it cannot carry labels");
    const A2Layout L = {sizex, sizey, xshift, yshift, pshift, flipx ? 1 : 0, flipy ? 1 : 0, bit10_is_data ? 2 : special_mode};
    V2E_HIP(hipMemsetAsync(total, 0, 16, s));
    if (n_records > 0) {
        k_a2_count<<<nblk, RB, 0, s>>>((const uint2 *)bytes, n_records, L, blk, counters);
        k_rd_scan<<<1, 1024, 0, s>>>(blk, nblk, total);
        k_a2_write<<<nblk, RB, 0, s>>>((const uint2 *)bytes, n_records, L, blk, (float4 *)rows, labels, t_us, ts_kept);
        k_a2_order<<<nblk, RB, 0, s>>>(ts_kept, total, counters);
    }
    k_a2_finish<<<1, 1, 0, s>>>(ts_kept, total, counters);
    V2E_HIP(hipGetLastError());
    return 0;
}

int64_t v2e_events_parse_text_scratch_bytes(int64_t n_bytes, int64_t cap_rows)
{
    return n_bytes < 0 || cap_rows < 0 ? -1 : TextScratch(n_bytes, cap_rows).bytes;
}

int v2e_events_parse_text(const char *bytes, int64_t n_bytes, int want_labels, float *rows, uint8_t *labels, int64_t cap_rows,
                          int64_t *counters, int64_t *flagged, int64_t cap_flagged, void *scratch, void *stream)
{
    V2E_REQUIRE(counters && scratch && n_bytes >= 0 && cap_rows >= 0 && cap_flagged >= 0, "bad args");
    V2E_REQUIRE(n_bytes == 0 || (bytes && (rows || cap_rows == 0)), "null");
    V2E_REQUIRE((flagged || cap_flagged == 0) && (labels || !want_labels || cap_rows == 0), "null flagged list or labels");
    V2E_REQUIRE(((uintptr_t)bytes & 15) == 0 && ((uintptr_t)rows & 15) == 0 && ((uintptr_t)scratch & 15) == 0, "unaligned buffer");
    const TextScratch ts(n_bytes, cap_rows);
    V2E_REQUIRE(ts.nl_blocks <= ((int64_t)1 << 30) && ts.line_blocks <= ((int64_t)1 << 30), "too large");
    hipStream_t s = (hipStream_t)stream;
    char *sc = (char *)scratch;
    long long *total = (long long *)(sc + ts.o_total), *nlblk = (long long *)(sc + ts.o_nlblk), *lnblk = (long long *)(sc + ts.o_lnblk);
    int64_t *starts = (int64_t *)(sc + ts.o_starts);
    float4 *tmp = (float4 *)(sc + ts.o_tmp);
    uint8_t *status = (uint8_t *)(sc + ts.o_status);
    V2E_HIP(hipMemsetAsync(total, 0, 16, s));
    k_txt_begin<<<1, 1, 0, s>>>(counters);
    if (n_bytes > 0) {
        const int nb = (int)ts.nl_blocks, lb = (int)ts.line_blocks;
        k_txt_count_newlines<<<nb, RB, 0, s>>>(bytes, n_bytes, nlblk);
        k_rd_scan<<<1, 1024, 0, s>>>(nlblk, nb, total);
        k_txt_line_starts<<<nb, RB, 0, s>>>(bytes, n_bytes, nlblk, total, cap_rows, starts);
        if (lb > 0) {
            k_txt_parse<<<lb, LINE_BLOCK, 0, s>>>(bytes, n_bytes, want_labels ? 1 : 0, starts, total, cap_rows, tmp, status, lnblk, counters);
            k_rd_scan<<<1, 1024, 0, s>>>(lnblk, lb, total + 1);
            k_txt_rows<<<lb, LINE_BLOCK, 0, s>>>(bytes, n_bytes, starts, total, cap_rows, tmp, status, lnblk, (float4 *)rows,
                                                 want_labels ? labels : nullptr, flagged, cap_flagged, counters);
        }
    }
    k_txt_finish<<<1, 1, 0, s>>>(bytes, n_bytes, total, cap_rows, total + 1, counters);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_events_parse_text_host(const char *bytes, int64_t n_bytes, int want_labels, float *rows, uint8_t *labels, int64_t cap_rows,
                               int64_t *counters, int64_t *flagged, int64_t cap_flagged)
{
    V2E_REQUIRE(counters && n_bytes >= 0 && cap_rows >= 0 && cap_flagged >= 0 && (n_bytes == 0 || bytes), "bad args");
    V2E_REQUIRE((rows || cap_rows == 0) && (flagged || cap_flagged == 0), "null");
    int64_t nlines = 0;
    for (int64_t i = 0; i < n_bytes; ++i) nlines += bytes[i] == '\n';
    nlines += n_bytes > 0 && bytes[n_bytes - 1] != '\n';
    counters[V2E_TXC_CALL_ROWS] = -1;
    counters[V2E_TXC_CALL_LINES] = nlines;
    counters[V2E_TXC_CALL_FLAGGED] = 0;
    if (nlines > cap_rows) return 0;
    int64_t n_rows = 0, ls = 0;
    while (ls < n_bytes) {
        int64_t le = ls;
        while (le < n_bytes && bytes[le] != '\n') ++le;
        v2e_tp::Row row;
        const int cls = v2e_tp::parse_line(bytes + ls, le - ls, want_labels ? 1 : 0, row);
        if (cls == v2e_tp::LINE_SKIP) ++counters[V2E_TXC_COMMENT];
        else if (cls == v2e_tp::LINE_BAD) ++counters[V2E_TXC_BAD];
        else {
            float *r = rows + 4 * n_rows;
            r[0] = row.t; r[1] = row.x; r[2] = row.y; r[3] = row.p;
            if (labels && want_labels) labels[n_rows] = (uint8_t)(row.label > 0);
            if (cls == v2e_tp::LINE_ROW_FLAGGED) {
                const int64_t slot = counters[V2E_TXC_CALL_FLAGGED]++;
                if (slot < cap_flagged) { flagged[2 * slot] = ls; flagged[2 * slot + 1] = n_rows; }
            }
            ++n_rows;
        }
        ls = le + 1;
    }
    counters[V2E_TXC_ROWS] += n_rows;
    counters[V2E_TXC_LINES] += nlines;
    counters[V2E_TXC_FLAGGED] += counters[V2E_TXC_CALL_FLAGGED];
    counters[V2E_TXC_CALL_ROWS] = n_rows;
    return 0;
}

} // extern "C"
