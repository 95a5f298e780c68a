// dev tool: what does a "the kernel before me has finished" hand-over to another stream cost the stream that hands over?
//   variant 0: nothing between the two kernels of stream A (the floor)
//   variant 1: hipLaunchKernel + hipEventRecord(e, A) between them; stream B: hipStreamWaitEvent(B, e) + a stamp kernel
//   variant 2: the first kernel through hipExtLaunchKernel(..., nullptr, e, 0) -- e is its stop event, no record; stream B the same
// Stream A holds a gate kernel (200 us, bounded by the clock) in front, so that every packet of a repetition is in its queue before
// the first short kernel runs: the gaps are the GPU's, not the host's enqueue time.  Events are hipEventDisableTiming, re-used by
// every repetition.  Build: hipcc -O2 --offload-arch=gfx950 scripts/ubench_stop_event.hip -o scripts/ubench_stop_event
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("ERR %s line %d: %s\n", #x, __LINE__, hipGetErrorString(e_)); return 1; } } while (0)

// t[0] = start, t[1] = end, after `ticks` of the 100 MHz clock (the spin is bounded by the clock itself)
__global__ void k_stamp(unsigned long long *t, unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(2);
    t[0] = t0;
    t[1] = wall_clock64();
}

constexpr unsigned long long GATE = 20000ull, SHORT = 500ull; // 200 us, 5 us

struct Ctx {
    hipStream_t A, B;
    hipEvent_t e;
    unsigned long long *t; // pinned host memory: [gate 0,1][k1 2,3][k2 4,5][B 6,7]
};

static hipError_t launch(hipStream_t s, unsigned long long *t, unsigned long long ticks, hipEvent_t stop)
{
    void *args[] = {(void *)&t, (void *)&ticks};
    if (stop) return hipExtLaunchKernel((const void *)k_stamp, dim3(1), dim3(64), args, 0, s, nullptr, stop, 0);
    return hipLaunchKernel((const void *)k_stamp, dim3(1), dim3(64), args, 0, s);
}

// one repetition; a2a = k1's end to k2's start, a2b = k1's end to B's start (ticks; a2b only for variants 1, 2)
static int rep(Ctx &c, int variant, long long *a2a, long long *a2b)
{
    memset(c.t, 0, 8 * sizeof(unsigned long long));
    CK(launch(c.A, c.t + 0, GATE, nullptr));
    CK(launch(c.A, c.t + 2, SHORT, variant == 2 ? c.e : nullptr));
    if (variant == 1) CK(hipEventRecord(c.e, c.A));
    CK(launch(c.A, c.t + 4, SHORT, nullptr));
    if (variant != 0) {
        CK(hipStreamWaitEvent(c.B, c.e, 0));
        CK(launch(c.B, c.t + 6, SHORT, nullptr));
    }
    CK(hipStreamSynchronize(c.A));
    CK(hipStreamSynchronize(c.B));
    *a2a = (long long)(c.t[4] - c.t[3]);
    *a2b = variant != 0 ? (long long)(c.t[6] - c.t[3]) : 0;
    return 0;
}

static double pct(std::vector<long long> v, double q)
{
    std::sort(v.begin(), v.end());
    return v[std::min(v.size() - 1, (size_t)(q * v.size()))] / 100.0; // us
}

// hipEventQuery / hipEventSynchronize on e, while the gate still runs and after: as recorded (variant 1) or as a stop event (2)
static int check_host_side(Ctx &c, int variant, const char *what)
{
    for (int round = 0; round < 2; ++round) { // round 1: the event re-used by a second launch
        memset(c.t, 0, 8 * sizeof(unsigned long long));
        CK(launch(c.A, c.t + 0, GATE, nullptr));
        CK(launch(c.A, c.t + 2, SHORT, variant == 2 ? c.e : nullptr));
        if (variant == 1) CK(hipEventRecord(c.e, c.A));
        const hipError_t q0 = hipEventQuery(c.e); // the gate runs for 200 us: not ready
        CK(hipEventSynchronize(c.e));
        const unsigned long long end_seen = c.t[3]; // the kernel's end stamp is visible to the host once the event has completed
        const hipError_t q1 = hipEventQuery(c.e);
        CK(hipStreamSynchronize(c.A));
        printf("%s, %s: query while pending = %s, k1's end stamp visible after synchronize = %s, query after = %s\n", what,
               round ? "event re-used" : "first use", q0 == hipErrorNotReady ? "hipErrorNotReady" : hipGetErrorString(q0),
               end_seen ? "yes" : "NO", q1 == hipSuccess ? "hipSuccess" : hipGetErrorString(q1));
    }
    return 0;
}

int main()
{
    Ctx c;
    CK(hipStreamCreateWithFlags(&c.A, hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&c.B, hipStreamNonBlocking));
    CK(hipEventCreateWithFlags(&c.e, hipEventDisableTiming));
    CK(hipHostMalloc(&c.t, 8 * sizeof(unsigned long long), hipHostMallocDefault));
    long long x, y;
    // do A and B have hardware queues of their own?  (B's stamp beside A's gate, not behind it)
    memset(c.t, 0, 8 * sizeof(unsigned long long));
    CK(launch(c.A, c.t + 0, GATE, nullptr));
    CK(launch(c.B, c.t + 6, SHORT, nullptr));
    CK(hipStreamSynchronize(c.A));
    CK(hipStreamSynchronize(c.B));
    printf("streams A and B: %s\n", c.t[6] < c.t[1] ? "separate hardware queues" : "ONE hardware queue (B waited for A's gate)");
    for (int w = 0; w < 10; ++w)
        for (int v = 0; v < 3; ++v) if (rep(c, v, &x, &y)) return 1;
    const int REPS = 200;
    std::vector<long long> a2a[3], a2b[3];
    int early[3] = {0, 0, 0};
    for (int r = 0; r < REPS; ++r)
        for (int v = 0; v < 3; ++v) { // interleaved
            if (rep(c, v, &x, &y)) return 1;
            a2a[v].push_back(x);
            a2b[v].push_back(y);
            if (v && y < 0) ++early[v]; // B ran before k1 had ended: the wait did not hold
        }
    const char *name[3] = {"0 nothing between      ", "1 launch + event record", "2 stop event, no record"};
    printf("%d repetitions per variant, interleaved; us (100 MHz wall clock)\n", REPS);
    printf("variant                    A-to-A p50   p90   min | A-to-B p50   p90   min | B before k1's end\n");
    for (int v = 0; v < 3; ++v)
        printf("%s   %9.2f %6.2f %5.2f | %9.2f %6.2f %5.2f | %d\n", name[v], pct(a2a[v], 0.5), pct(a2a[v], 0.9), pct(a2a[v], 0.0),
               pct(a2b[v], 0.5), pct(a2b[v], 0.9), pct(a2b[v], 0.0), early[v]);
    const double d = pct(a2a[1], 0.5) - pct(a2a[2], 0.5);
    const double s1 = pct(a2a[1], 0.9) - pct(a2a[1], 0.5), s2 = pct(a2a[2], 0.9) - pct(a2a[2], 0.5);
    printf("A-to-A median: variant 1 - variant 2 = %.2f us; p90 - p50 spread: variant 1 %.2f, variant 2 %.2f -> %s\n", d, s1, s2,
           d > s1 && d > s2 ? "PROCEED" : "STOP");
    if (check_host_side(c, 1, "recorded event")) return 1;
    if (check_host_side(c, 2, "stop event    ")) return 1;
    return 0;
}
