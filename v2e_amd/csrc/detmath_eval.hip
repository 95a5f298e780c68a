// detmath_eval.hip -- diagnostics: include/v2e_detmath.h evaluated on the device, an array at a time (v2e_detmath_eval).
//
// The header is compiled verbatim into the kernels and into the CPU oracle, and every Philox-mode fixture rests on the two giving the
// same bits.  This entry point lets a test put that to the device directly, on whole domains (all 2^24 arguments of the logarithm)
// rather than on the arguments a fixture happens to form: tests/test_detmath_gpu.py compares it with the oracle's loops over the same
// functions.  Built with the library's flags like every other translation unit; nothing in the product path calls it.
//
// One thread per element, grid-stride.  Every value travels as a 32-bit word (a float as its bit pattern, so NaN and -0 compare)
// through plain loads and stores.  The kernel calls the header's functions and nothing else.
#include "common.h"
#include "../../include/v2e_detmath.h"

namespace {

constexpr int MAX_BLOCKS = 1 << 16;

__global__ __launch_bounds__(256) void k_detmath_eval(int fn, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                      uint32_t *__restrict__ out0, uint32_t *__restrict__ out1, long long n)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        switch (fn) {
        case V2E_DM_PHILOX: {
            uint32_t o[4];
            v2e_philox4x32(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3], b[0], b[1], o);
            for (int k = 0; k < 4; ++k) out0[4 * i + k] = o[k];
            break;
        }
        case V2E_DM_PHILOX_KS: {
            v2e_philox_keys ks;
            uint32_t o[4];
            v2e_philox_key_schedule(b[0], b[1], &ks);
            v2e_philox4x32_ks(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3], &ks, o);
            for (int k = 0; k < 4; ++k) out0[4 * i + k] = o[k];
            break;
        }
        case V2E_DM_LOGF: out0[i] = v2e_f2u(v2e_det_logf(v2e_u2f(a[i]))); break;
        case V2E_DM_EXPF: out0[i] = v2e_f2u(v2e_det_expf(v2e_u2f(a[i]))); break;
        case V2E_DM_SINCOS2PI: {
            float s, c;
            v2e_det_sincos2pi(v2e_u2f(a[i]), &s, &c);
            out0[i] = v2e_f2u(s);
            out1[i] = v2e_f2u(c);
            break;
        }
        case V2E_DM_NORMAL2: {
            float nc, ns;
            v2e_normal2(a[i], b[i], &nc, &ns);
            out0[i] = v2e_f2u(nc);
            out1[i] = v2e_f2u(ns);
            break;
        }
        case V2E_DM_SLEEF_SINHF: out0[i] = v2e_f2u(v2e_sleef_sinhf(v2e_u2f(a[i]))); break;
        case V2E_DM_PERM_APPLY:
        case V2E_DM_PERM_INVERT: {
            v2e_perm_t pm;
            v2e_perm_init(&pm, (uint64_t)b[1] | (uint64_t)b[2] << 32, b[3], b[4], b[5], b[0]);
            out0[i] = fn == V2E_DM_PERM_APPLY ? v2e_perm_apply(&pm, a[i]) : v2e_perm_invert(&pm, a[i]);
            break;
        }
        case V2E_DM_NTH_SET_BIT_256: {
            const uint32_t *m = a + 8 * i;
            out0[i] = v2e_nth_set_bit_256((uint64_t)m[0] | (uint64_t)m[1] << 32, (uint64_t)m[2] | (uint64_t)m[3] << 32,
                                          (uint64_t)m[4] | (uint64_t)m[5] << 32, (uint64_t)m[6] | (uint64_t)m[7] << 32, b[i]);
            break;
        }
        case V2E_DM_TS_FORMULA:
            out0[i] = v2e_f2u(v2e_ts_formula(a[4 * i], a[4 * i + 1], v2e_u2f(a[4 * i + 2]), v2e_u2f(a[4 * i + 3]), v2e_u2f(b[i])));
            break;
        case V2E_DM_DRAW_PAIR:
        case V2E_DM_DRAW_PAIR_KS: {
            const uint64_t seed = (uint64_t)b[0] | (uint64_t)b[1] << 32;
            float r_odd, u_odd, r_even, u_even;
            if (fn == V2E_DM_DRAW_PAIR) {
                v2e_draw_pair(seed, b[2], b[3], a[i], (int)b[4], &r_odd, &u_odd, &r_even, &u_even);
            } else {
                v2e_philox_keys ks;
                v2e_philox_key_schedule((uint32_t)seed, (uint32_t)(seed >> 32), &ks);
                v2e_draw_pair_ks(&ks, b[2], b[3], a[i], (int)b[4], &r_odd, &u_odd, &r_even, &u_even);
            }
            out0[4 * i] = v2e_f2u(r_odd);
            out0[4 * i + 1] = v2e_f2u(u_odd);
            out0[4 * i + 2] = v2e_f2u(r_even);
            out0[4 * i + 3] = v2e_f2u(u_even);
            break;
        }
        case V2E_DM_DRAW_FRAME: {
            float r, u;
            v2e_draw_frame((uint64_t)b[0] | (uint64_t)b[1] << 32, b[2], b[3], a[i], &r, &u);
            out0[i] = v2e_f2u(r);
            out1[i] = v2e_f2u(u);
            break;
        }
        case V2E_DM_DRAW_PNOISE: out0[i] = v2e_f2u(v2e_draw_pnoise((uint64_t)b[0] | (uint64_t)b[1] << 32, b[2], b[3], a[i])); break;
        case V2E_DM_DRAW_INIT: {
            const uint64_t seed = (uint64_t)b[0] | (uint64_t)b[1] << 32;
            float n_pos, n_neg, n_rate;
            v2e_draw_init(seed, b[2], a[i], &n_pos, &n_neg, &n_rate);
            out0[4 * i] = v2e_f2u(n_pos);
            out0[4 * i + 1] = v2e_f2u(n_neg);
            out0[4 * i + 2] = v2e_f2u(n_rate);
            out0[4 * i + 3] = v2e_f2u(v2e_draw_scidvs(seed, b[2], a[i]));
            break;
        }
        default: break;
        }
    }
}

} // namespace

int v2e_detmath_eval(int fn, const uint32_t *a, const uint32_t *b, uint32_t *out0, uint32_t *out1, int64_t n, void *stream)
{
    V2E_REQUIRE(fn >= 0 && fn < V2E_DM_COUNT, "fn");
    V2E_REQUIRE(n >= 0 && n <= (int64_t)1 << 26, "n");
    if (n == 0) return 0;
    const bool needs_b = fn != V2E_DM_LOGF && fn != V2E_DM_EXPF && fn != V2E_DM_SINCOS2PI && fn != V2E_DM_SLEEF_SINHF;
    const bool needs_out1 = fn == V2E_DM_SINCOS2PI || fn == V2E_DM_NORMAL2 || fn == V2E_DM_DRAW_FRAME;
    V2E_REQUIRE(a && out0 && (b || !needs_b) && (out1 || !needs_out1), "null");
    const int blocks = v2e_cdiv(n, 256) < MAX_BLOCKS ? v2e_cdiv(n, 256) : MAX_BLOCKS;
    k_detmath_eval<<<blocks, 256, 0, (hipStream_t)stream>>>(fn, a, b, out0, out1, (long long)n);
    V2E_HIP(hipGetLastError());
    return 0;
}
