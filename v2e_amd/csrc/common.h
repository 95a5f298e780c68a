// common.h -- error plumbing shared by the gfx950 translation units of libv2e_amd.so
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

#include "../../include/v2e_amd.h"

void v2e_set_error(const char *fmt, ...);

#define V2E_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            v2e_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return V2E_EHIP;                                                               \
        }                                                                                  \
    } while (0)

#define V2E_REQUIRE(cond, msg)                                       \
    do {                                                             \
        if (!(cond)) {                                               \
            v2e_set_error("%s:%d %s", __FILE__, __LINE__, msg);      \
            return V2E_EINVAL;                                       \
        }                                                            \
    } while (0)

// the label arguments of a labelled entry point: a byte per row, or a table of at least one bound, or neither
#define V2E_REQUIRE_LABELS(labels, label_bounds, n_label_bounds) \
    V2E_REQUIRE(!((labels) && (label_bounds)) && (!(label_bounds) || (n_label_bounds) >= 1), \
                "labels: a byte per row or a table of bounds, not both")

static inline int v2e_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// csdvs.hip: one frame's surround (diffuser) update enqueued on `s` without a host step (emu.hip's per-frame run loop)
int v2e_csdvs_enqueue_frame(const void *p_plane, void *h_plane, void *h_scratch, int H, int W, int f64, double alpha_p, double alpha_h,
                            int num_steps, double thr, unsigned long long *slots, int *steps_taken_dev, hipStream_t s);

// probe.hip: the probed pixels of a run (v2e_emu_set_probes; row * W + col, one clip), passed to the kernels by value, and the three
// launches emu.hip's per-frame run loop adds for them.  out_f: the frame's block out[f][P][V2E_PROBE_FIELDS]; cnt: uint32
// [n_frames][P][2] and ticket: one uint32, both zero on entry.
struct V2EProbeSet { int n; int32_t pix[V2E_PROBE_MAX]; };
int v2e_probe_tap_count(const V2EProbeSet &ps, const void *frame, int dtype, const double *lognew, const double *diff, double *out_f,
                        hipStream_t s);
int v2e_probe_tap_emit(const V2EProbeSet &ps, const void *lp, const void *base, int f64_state, const float *pos, const float *neg,
                       int scalar_thres, double pos_scalar, double neg_scalar, double *out_f, hipStream_t s);
int v2e_probe_count_rows(const V2EProbeSet &ps, const float *events, uint64_t cap, const v2e_frame_rec *recs, int n_frames, int W,
                         unsigned int *cnt, unsigned int *ticket, double *out, int n_cu, hipStream_t s);
