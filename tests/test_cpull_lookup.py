"""k_cpull's bucketed group lookup (v2e_amd/csrc/pull_index.h) against the whole-row binary search it replaced, on the CPU.

The header is compiled by the host compiler into a small shim that stages a prefix row exactly as k_cpull<false> does (four entries
per thread plus the entry after them, padding 0xFFFFFFFF up to p2) and then, for EVERY canonical index cp < T, compares the group
and its base from pull_index_find with those of the log2(p2)-step search over the row.  Rows: random, empty groups, one hot group,
full groups, padding entries (nwaves < nwp), tiny and large totals, at the p2 of 346x260 (352 groups -> 512) and of 1280x720
(3 600 groups -> 4 096, the single-level search forced)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "v2e_amd", "csrc")

SHIM = r"""
#include <stdint.h>
#include <stdlib.h>
#include "pull_index.h"

/* 0: every cp < T agrees with the whole-row search; -1 - cp: the first cp that does not; -100000000 - b: index entry b unwritten */
int pull_check(const uint32_t *row, int nwp, int P2, uint32_t T)
{
    uint32_t *tab = (uint32_t *)malloc(sizeof(uint32_t) * P2);
    uint16_t *idx = (uint16_t *)malloc(sizeof(uint16_t) * P2);
    int rc = 0;
    for (int k = 0; k < P2; ++k) idx[k] = 0xFFFFu;
    const uint32_t sh = pull_bucket_shift(T, (uint32_t)P2);
    for (int kk = 0; kk < P2; kk += 4) {
        uint32_t v[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, nx = 0xFFFFFFFFu;
        if (kk < nwp) for (int j = 0; j < 4; ++j) v[j] = row[kk + j];
        if (kk + 4 < nwp) nx = row[kk + 4];
        for (int j = 0; j < 4; ++j) {
            tab[kk + j] = v[j];
            pull_index_group(idx, (uint32_t)(kk + j), v[j], j < 3 ? v[j + 1] : nx, T, sh);
        }
    }
    if (T > 0u && ((T - 1u) >> sh) + 1u >= (uint32_t)P2) rc = -200000000;
    for (uint32_t cp = 0; cp < T && rc == 0; ++cp) {
        uint32_t g = 0, gbase = 0;
        for (int st = P2 >> 1; st >= 1; st >>= 1) {
            const uint32_t v = tab[g + st];
            if (v <= cp) { g += st; gbase = v; }
        }
        const uint32_t b = cp >> sh;
        if (idx[b] == 0xFFFFu) { rc = -100000000 - (int)b; break; }
        if (idx[b + 1] == 0xFFFFu) { rc = -100000000 - (int)(b + 1); break; }
        uint32_t gb2 = 0;
        const uint32_t g2 = pull_index_find(tab, idx, sh, cp, &gb2);
        if (g2 != g || gb2 != gbase) rc = -1 - (int)cp;
    }
    free(tab);
    free(idx);
    return rc;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler")
    d = tmp_path_factory.mktemp("pull_index")
    src, so = d / "shim.c", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call([cc, "-O2", "-std=c99", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.pull_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32]
    lib.pull_check.restype = C.c_int
    return lib


def p2_of(nwaves):  # emu_chain_host.h launch_emission, single level
    p2 = 64
    while p2 < nwaves:
        p2 *= 2
    return p2


def check(lib, counts, nwp=None):
    counts = np.asarray(counts, np.int64)
    nwaves = counts.size
    nwp = nwp or (nwaves + 15) // 16 * 16
    T = int(counts.sum())
    row = np.full(nwp, T, np.uint32)                    # entries nwaves .. nwp - 1 hold the key's total
    row[:nwaves] = np.cumsum(counts) - counts
    rc = lib.pull_check(row.ctypes.data_as(C.c_void_p), nwp, p2_of(nwaves), T)
    assert rc == 0, "nwaves %d T %d: rc %d" % (nwaves, T, rc)


@pytest.mark.parametrize("nwaves", [352, 351, 337, 3600, 64, 1])
def test_random_rows(shim, nwaves):
    rng = np.random.default_rng(nwaves)
    for trial in range(12):
        dens = [0.02, 0.1, 0.3, 0.6, 0.9, 1.0][trial % 6]
        counts = rng.binomial(256, dens, nwaves)
        counts[rng.random(nwaves) < (0.5 if trial >= 6 else 0.0)] = 0  # runs of empty groups
        check(shim, counts)


@pytest.mark.parametrize("nwaves", [352, 3600])
def test_adversarial_rows(shim, nwaves):
    z = np.zeros(nwaves, np.int64)
    for g in [0, 1, nwaves // 2, nwaves - 2, nwaves - 1]:
        for c in [1, 2, 37, 255, 256]:
            one = z.copy()
            one[g] = c                                 # one hot group, all others empty
            check(shim, one)
    check(shim, np.full(nwaves, 256))                  # every group full
    check(shim, np.full(nwaves, 1))                    # one event per group: as many groups per bucket as the shift allows
    alt = np.zeros(nwaves, np.int64)
    alt[::2] = 256
    check(shim, alt)
    alt = np.zeros(nwaves, np.int64)
    alt[1::7] = 3
    alt[-1] = 256
    check(shim, alt)
    ramp = np.arange(nwaves) % 257
    check(shim, ramp)
    check(shim, ramp[::-1].copy())


def test_padding_and_totals(shim):
    rng = np.random.default_rng(5)
    for nwaves in [337, 350, 352]:
        counts = rng.binomial(256, 0.1, nwaves)
        check(shim, counts, nwp=(nwaves + 15) // 16 * 16)
        check(shim, counts, nwp=512)                   # padding up to p2 itself
    for T in [1, 2, 3, 510, 511, 512, 1023, 1024, 1025, 4097]:
        counts = np.zeros(352, np.int64)
        idx = rng.choice(352, size=min(352, max(1, T // 200 + 1)), replace=False)
        left = T
        for k, g in enumerate(idx):
            c = min(256, left if k == len(idx) - 1 else left // (len(idx) - k))
            counts[g] = c
            left -= c
        if left:
            continue
        check(shim, counts)



@pytest.mark.parametrize("W,H", [(346, 260), (1280, 720), (64, 96), (4095, 4095)])
def test_row_pixel_division(W, H):
    """k_cpull's y = p / W with one multiply: the float32 quotient estimate, then one correction by the sign / size of the
    remainder, for every pixel of the frame (npx < 2^24: float32 holds p exactly)."""
    p = np.arange(W * H, dtype=np.uint32)
    rcpW = np.float32(1.0) / np.float32(W)
    qy = (p.astype(np.float32) * rcpW).astype(np.uint32)
    r = p.astype(np.int64) - qy.astype(np.int64) * W
    assert np.all(np.abs(r) < 2 * W)                                # the estimate is the true quotient or one off
    lo, hi = r < 0, r >= W
    qy = qy - lo + hi
    r = r + W * lo - W * hi
    assert np.array_equal(qy, p // W) and np.array_equal(r, p % W)
