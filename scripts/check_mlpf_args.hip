// check_mlpf_args.hip -- v2e_patches_mlp_scores refuses bad arguments with V2E_EINVAL before anything is launched: a stand-alone
// host program (no GPU needed: every call here returns from the argument checks), meant to be built with the host sanitizers.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         scripts/check_mlpf_args.hip -o check_mlpf_args && ./check_mlpf_args
#include <cstdarg>
#include <cstdio>

#include "../v2e_amd/csrc/mlpf.hip"

static char g_msg[512];
void v2e_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}

int main()
{
    // addresses that are never dereferenced on the host: the checks look at null-ness and alignment only
    alignas(16) static float rows[8], w[4], out[4];
    static int64_t keys[2];
    static int32_t seg[2];
    static int8_t lp[1];
    static uint8_t valid[2], mask[2];
    struct Case { const char *what; const float *ev; int64_t n; int H, W; const int64_t *keys; const int32_t *seg; const float *lt;
                  const int8_t *lp; int radius; double tau; const float *w1, *b1; int hidden; const float *w2, *b2; float *scores;
                  uint8_t *valid; double thr; uint8_t *mask; };
    const Case good = {"", rows, 1, 1, 1, keys, seg, w, lp, 3, 0.1, w, w, 20, w, w, out, valid, 0.0, mask};
    Case c[24];
    int m = 0;
#define BAD(name, stmt) do { c[m] = good; c[m].what = name; { Case &k = c[m]; stmt; } ++m; } while (0)
    BAD("null rows", k.ev = nullptr);
    BAD("null sorted keys", k.keys = nullptr);
    BAD("null seg", k.seg = nullptr);
    BAD("null last_t", k.lt = nullptr);
    BAD("null last_p", k.lp = nullptr);
    BAD("null scores", k.scores = nullptr);
    BAD("null valid", k.valid = nullptr);
    BAD("null w1", k.w1 = nullptr);
    BAD("null b1", k.b1 = nullptr);
    BAD("null w2", k.w2 = nullptr);
    BAD("null b2", k.b2 = nullptr);
    BAD("null seg with n = 0", (k.n = 0, k.seg = nullptr));
    BAD("radius 0", k.radius = 0);
    BAD("radius 4", k.radius = 4);
    BAD("hidden 0", k.hidden = 0);
    BAD("hidden 65", k.hidden = 65);
    BAD("tau 0", k.tau = 0.0);
    BAD("tau negative", k.tau = -1.0);
    BAD("tau infinite", k.tau = __builtin_inf());
    BAD("tau NaN", k.tau = __builtin_nan(""));
    BAD("misaligned rows", k.ev = rows + 1);
    BAD("negative n", k.n = -1);
    BAD("H = 0", k.H = 0);
    BAD("NaN threshold with a mask", k.thr = __builtin_nan(""));
    int failed = 0;
    for (int i = 0; i < m; ++i) {
        const Case &k = c[i];
        g_msg[0] = 0;
        const int rc = v2e_patches_mlp_scores(k.ev, k.n, k.H, k.W, k.keys, k.seg, k.lt, k.lp, k.radius, k.tau, k.w1, k.b1, k.hidden, k.w2,
                                              k.b2, k.scores, k.valid, k.thr, k.mask, nullptr);
        const bool ok = rc == V2E_EINVAL && g_msg[0];
        printf("%-28s rc = %d (%s) %s\n", k.what, rc, g_msg, ok ? "ok" : "FAILED");
        failed += !ok;
    }
    // n = 0 with good arguments: nothing to do, no launch
    const int rc0 = v2e_patches_mlp_scores(nullptr, 0, 1, 1, nullptr, seg, w, lp, 3, 0.1, w, w, 20, w, w, nullptr, nullptr, 0.0, nullptr, nullptr);
    printf("%-28s rc = %d %s\n", "n = 0", rc0, rc0 == 0 ? "ok" : "FAILED");
    failed += rc0 != 0;
    printf("%d cases, %d failed\n", m + 1, failed);
    return failed ? 1 : 0;
}
