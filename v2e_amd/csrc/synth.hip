// synth.hip -- the reference's synthetic input sources (v2e.py --synthetic_input=scripts.<name>) rendered straight into HBM:
// a block of n consecutive frames [n][H][W] per launch, for v2e_amd/synthetic.py.
//
//   v2e_synth_dots        scripts/moving_dot.py:26-54, 156-183 (fill_dot on a bg frame, uint8) and
//                         scripts/particles.py:187-197, 213-241 (fill_dot on a bg frame, float32)
//   v2e_synth_gradients   scripts/gradients.py:117-138 (im_function)
//   v2e_synth_barberpole  scripts/barberpole.py:85-95, 139-140, 155-163 (pole mask, bb_func)
//
// All arithmetic is float64 in the reference's order of operations (numpy's is; the library is built with -ffp-contract=off, so no
// product is fused into a sum).  What is per frame and tiny -- dot centres and their rounded boxes, the bump position p, the frame
// time -- the host computes in the reference's own expressions and hands over as small device tables; the kernels restate the
// per-pixel part.  exp / sin / tanh are the device library's float64 functions: they may differ from the recording host's in the
// last bit, which moves a stored value only where the exact one sits on a decision boundary (tests/golden/make_golden_synth.py
// measures the distance of every fixture value from the nearest one).
//
// Kernel form: one lane per four consecutive pixels of one frame; the four are one aligned 4-element store (a 32-bit word of
// uint8, a float4) wherever the whole group lies inside the frame, single stores for the frame's ragged head and tail (a frame
// of an odd size does not start on a 4-element boundary of the buffer).  Nothing outside [out, out + n * H * W) is written: every
// store is guarded by 0 <= pixel < H * W of its own frame.
#include "common.h"

#include <cstdint>

namespace {

constexpr int BLOCK = 256;
constexpr int DOT_CHUNK = 1024; // dot boxes per LDS chunk (8 KiB); longer lists are walked chunk by chunk from the back

template <typename T> __device__ __forceinline__ T to_out(double v);
// numpy storing a double into a uint8 array: the C conversion (truncation toward zero; the values are inside 0..255 here)
template <> __device__ __forceinline__ uint8_t to_out<uint8_t>(double v) { return (uint8_t)(int)v; }
template <> __device__ __forceinline__ float to_out<float>(double v) { return (float)v; } // round to nearest even, as numpy
template <> __device__ __forceinline__ double to_out<double>(double v) { return v; }

__device__ __forceinline__ void store_vec(uint8_t *p, const uint8_t (&v)[4])
{
    *reinterpret_cast<uint32_t *>(p) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}
__device__ __forceinline__ void store_vec(float *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store_vec(double *p, const double (&v)[4])
{
    reinterpret_cast<double2 *>(p)[0] = make_double2(v[0], v[1]);
    reinterpret_cast<double2 *>(p)[1] = make_double2(v[2], v[3]);
}

// The lane's group of four pixels in frame `f`: groups are cut at the 4-element boundaries of the buffer's ADDRESS, so that a full
// group is an aligned vector store whatever H * W is; p0 (the group's first pixel within the frame) is negative in the frame's
// first group when the frame does not start on such a boundary.
template <typename T> struct Group {
    T *frame;
    long long p0;
    __device__ __forceinline__ Group(T *out, int f, int npx, int groups_per_frame_blocks)
    {
        frame = out + (size_t)f * npx;
        const int a = (int)((reinterpret_cast<uintptr_t>(frame) / sizeof(T)) & 3);
        const long long g = (long long)(blockIdx.x % groups_per_frame_blocks) * BLOCK + threadIdx.x;
        p0 = 4 * g - a;
    }
    __device__ __forceinline__ bool valid(int j, int npx) const { return p0 + j >= 0 && p0 + j < npx; }
    __device__ __forceinline__ void store(const T (&v)[4], int npx) const
    {
        if (p0 >= 0 && p0 + 4 <= npx) {
            store_vec(frame + p0, v);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (valid(j, npx)) frame[p0 + j] = v[j];
        }
    }
};

// moving_dot.py:39-54 / particles.py:228-241 as a gather: the pixel takes the value of the LAST dot of its frame's list whose box
// [x0 - d, x0 + d) x [y0 - d, y0 + d) covers it (the reference draws the dots in list order, each overwriting the one before), or
// bg.  No two dots ever write one pixel, so the result does not depend on scheduling.  A box that leaves the frame is clipped by
// construction (particles.py:232; the host refuses such a moving_dot table).
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_dots(const double *__restrict__ centres, const int32_t *__restrict__ boxes,
                                               const int32_t *__restrict__ offs, T *__restrict__ out, int W, int npx, int gpb, double bg,
                                               double fg, double sigma, int d, double peak, double low_cut, int clip)
{
    __shared__ int2 sbox[DOT_CHUNK];
    const int f = blockIdx.x / gpb;
    const Group<T> grp(out, f, npx, gpb);
    int px[4], py[4], hit[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = grp.valid(j, npx) ? (int)(grp.p0 + j) : 0;
        py[j] = p / W;
        px[j] = p - py[j] * W;
        hit[j] = -1;
    }
    const int first = offs[f], cnt = offs[f + 1] - first;
    for (int hi = cnt; hi > 0; hi -= DOT_CHUNK) { // (cnt is the same in every lane of the workgroup: the barriers are uniform)
        const int lo = hi > DOT_CHUNK ? hi - DOT_CHUNK : 0;
        __syncthreads();
        for (int i = threadIdx.x; i < hi - lo; i += BLOCK) sbox[i] = reinterpret_cast<const int2 *>(boxes)[first + lo + i];
        __syncthreads();
        for (int i = hi - lo - 1; i >= 0; --i) {
            const int2 b = sbox[i];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (hit[j] < 0 && px[j] >= b.x - d && px[j] < b.x + d && py[j] >= b.y - d && py[j] < b.y + d) hit[j] = lo + i;
        }
    }
    T v4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double pv = bg;
        if (hit[j] >= 0) {
            const double x = centres[2 * (size_t)(first + hit[j])], y = centres[2 * (size_t)(first + hit[j]) + 1];
            const double ddx = (double)px[j] - x, ddy = (double)py[j] - y; // distances of this pixel to the float dot location
            const double dist2 = ddx * ddx + ddy * ddy;
            double v = peak * exp(-dist2 / (sigma * sigma));
            if (v > 1) v = 1; // a disk, not a gaussian blob
            else if (v < low_cut) v = 0;
            pv = bg + (fg - bg) * v;
            if (clip) {
                if (pv > 255) pv = 255;
                else if (pv < 0) pv = 0;
            }
        }
        v4[j] = to_out<T>(pv);
    }
    grp.store(v4, npx);
}

// gradients.py:121-140; x is the pixel column, the rows are equal
__global__ __launch_bounds__(BLOCK) void k_gradients(const double *__restrict__ pf, uint8_t *__restrict__ out, int W, int npx, int gpb,
                                                    double low, double high, double slope, double w2)
{
    const int f = blockIdx.x / gpb;
    const Group<uint8_t> grp(out, f, npx, gpb);
    const double p = pf[f];      // centre of bump location
    const double p2 = p + w2 * 2; // centre of sharp edges
    uint8_t v4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pi = grp.valid(j, npx) ? (int)(grp.p0 + j) : 0;
        const double x = (double)(pi % W);
        double g = low;
        if (x > p - w2 && x < p) g = high + slope * (p - x);   // left side of bump
        if (x <= p + w2 && x >= p) g = high + slope * (x - p); // right side of bump
        if (x > p2 && x <= p2 + 10) g = high;                  // square wave
        v4[j] = to_out<uint8_t>(g);
    }
    grp.store(v4, npx);
}

// barberpole.py:155-163 inside the pole (barberpole.py:94-97: strict inequalities), bg outside (barberpole.py:140)
__global__ __launch_bounds__(BLOCK) void k_barberpole(const double *__restrict__ tf, uint8_t *__restrict__ out, int W, int npx, int gpb,
                                                     double low, double diff, double tan_a, double speed, double two_pi,
                                                     double wavelength, int minx, int maxx, int miny, int maxy, int bg)
{
    const int f = blockIdx.x / gpb;
    const Group<uint8_t> grp(out, f, npx, gpb);
    const double ts = tf[f] * speed;
    uint8_t v4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pi = grp.valid(j, npx) ? (int)(grp.p0 + j) : 0;
        const int y = pi / W, x = pi - y * W;
        uint8_t o = (uint8_t)bg;
        if (x > minx && x < maxx && y > miny && y < maxy) {
            const double ph = two_pi * ((double)y - tan_a * (double)x - ts) / wavelength;
            o = to_out<uint8_t>(floor(low + diff * 0.5 * (1 + tanh(10 * sin(ph)))));
        }
        v4[j] = o;
    }
    grp.store(v4, npx);
}

// groups per frame (one more than H * W / 4 rounded up can be needed: the frame's ragged head) in workgroups, and the grid
inline bool plan_grid(int n, int H, int W, int *gpb, unsigned *grid)
{
    const long long npx = (long long)H * W;
    if (npx > 0x7fffffffLL - 8) return false;
    const long long groups = (npx + 3 + 3) / 4;
    *gpb = (int)((groups + BLOCK - 1) / BLOCK);
    const long long g = (long long)*gpb * n;
    if (g > 0x7fffffffLL) return false;
    *grid = (unsigned)g;
    return true;
}

} // namespace

extern "C" {

int v2e_synth_dots(const double *centres, const int32_t *boxes, const int32_t *offs, int n, int H, int W, void *out, int out_dtype,
                   double bg, double fg, double sigma, int d, double peak, double low_cut, int clip, void *stream)
{
    V2E_REQUIRE(offs && out && n > 0 && H > 0 && W > 0, "bad synth_dots args");
    V2E_REQUIRE(d > 0 && d < (1 << 20) && sigma == sigma && sigma != 0, "bad dot size");
    V2E_REQUIRE(out_dtype == V2E_DT_U8 || out_dtype == V2E_DT_F32 || out_dtype == V2E_DT_F64, "bad output type");
    int gpb;
    unsigned grid;
    V2E_REQUIRE(plan_grid(n, H, W, &gpb, &grid), "block too large");
    const size_t es = out_dtype == V2E_DT_U8 ? 1 : (out_dtype == V2E_DT_F32 ? 4 : 8);
    V2E_REQUIRE(reinterpret_cast<uintptr_t>(out) % es == 0, "output buffer is not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    const int npx = H * W;
    if (out_dtype == V2E_DT_U8)
        k_dots<uint8_t><<<grid, BLOCK, 0, s>>>(centres, boxes, offs, (uint8_t *)out, W, npx, gpb, bg, fg, sigma, d, peak, low_cut, clip);
    else if (out_dtype == V2E_DT_F32)
        k_dots<float><<<grid, BLOCK, 0, s>>>(centres, boxes, offs, (float *)out, W, npx, gpb, bg, fg, sigma, d, peak, low_cut, clip);
    else
        k_dots<double><<<grid, BLOCK, 0, s>>>(centres, boxes, offs, (double *)out, W, npx, gpb, bg, fg, sigma, d, peak, low_cut, clip);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_synth_gradients(const double *p, int n, int H, int W, uint8_t *out, double low, double high, double slope, double w2,
                        void *stream)
{
    V2E_REQUIRE(p && out && n > 0 && H > 0 && W > 0, "bad synth_gradients args");
    int gpb;
    unsigned grid;
    V2E_REQUIRE(plan_grid(n, H, W, &gpb, &grid), "block too large");
    k_gradients<<<grid, BLOCK, 0, (hipStream_t)stream>>>(p, out, W, H * W, gpb, low, high, slope, w2);
    V2E_HIP(hipGetLastError());
    return 0;
}

int v2e_synth_barberpole(const double *t, int n, int H, int W, uint8_t *out, double low, double diff, double tan_a, double speed,
                         double two_pi, double wavelength, int minx, int maxx, int miny, int maxy, int bg, void *stream)
{
    V2E_REQUIRE(t && out && n > 0 && H > 0 && W > 0, "bad synth_barberpole args");
    V2E_REQUIRE(bg >= 0 && bg <= 255, "bg is a uint8 grey level");
    int gpb;
    unsigned grid;
    V2E_REQUIRE(plan_grid(n, H, W, &gpb, &grid), "block too large");
    k_barberpole<<<grid, BLOCK, 0, (hipStream_t)stream>>>(t, out, W, H * W, gpb, low, diff, tan_a, speed, two_pi, wavelength, minx,
                                                         maxx, miny, maxy, bg);
    V2E_HIP(hipGetLastError());
    return 0;
}

} // extern "C"
