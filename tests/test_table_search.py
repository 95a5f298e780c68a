"""The table searches of the event-row kernels (v2e_amd/csrc/table_search.h) on the CPU: the header is compiled by the host C++
compiler into a small shim, count_le / count_lt are compared with numpy.searchsorted ('right' / 'left'), frame_of_row and
row_is_signal with a direct loop over the records.  Tables of length 0, 1, 2, 3, 1023, 1024 and 1025, with and without runs of equal
entries (frames without rows share an ev_offset: the last of them wins); probes below the first entry, equal to every entry and
above the last; every lower bound `from` up to the result."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "v2e_amd", "csrc")

SHIM = r"""
#include "table_search.h"

extern "C" {
void le_i64(const int64_t *a, int n, const int64_t *v, int nv, int from, int *out)
{
    for (int j = 0; j < nv; ++j) out[j] = count_le<int64_t>(a, n, v[j], from);
}
void lt_i64(const int64_t *a, int n, const int64_t *v, int nv, int from, int *out)
{
    for (int j = 0; j < nv; ++j) out[j] = count_lt<int64_t>(a, n, v[j], from);
}
void le_f64(const double *a, int n, const double *v, int nv, int from, int *out)
{
    for (int j = 0; j < nv; ++j) out[j] = count_le<double>(a, n, v[j], from);
}
void lt_f64(const double *a, int n, const double *v, int nv, int from, int *out)
{
    for (int j = 0; j < nv; ++j) out[j] = count_lt<double>(a, n, v[j], from);
}
/* records from their ev_offset / n_signal columns; out[2 j] = frame_of_row, out[2 j + 1] = row_is_signal of row v[j] */
void frames(const uint64_t *ev_offset, const uint32_t *n_signal, int nrec, const int64_t *v, int nv, int *out)
{
    v2e_frame_rec *recs = new v2e_frame_rec[nrec]();
    for (int f = 0; f < nrec; ++f) { recs[f].ev_offset = ev_offset[f]; recs[f].n_signal = n_signal[f]; }
    for (int j = 0; j < nv; ++j) {
        out[2 * j] = frame_of_row(recs, nrec, v[j]);
        out[2 * j + 1] = row_is_signal(v[j], recs, nrec, 0);
    }
    delete[] recs;
}
int one_frame(int64_t i, int64_t n_signal0) { return row_is_signal(i, nullptr, 0, n_signal0); }
}
"""

LENGTHS = [0, 1, 2, 3, 1023, 1024, 1025]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("table_search")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    return C.CDLL(str(so))


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def tables(n, seed):
    """Ascending int64 tables of length n: strictly ascending, and with runs of equal entries."""
    rng = np.random.default_rng(seed)
    yield np.cumsum(rng.integers(1, 5, n)).astype(np.int64) + 10
    yield np.cumsum(rng.integers(0, 2, n) * rng.integers(0, 4, n)).astype(np.int64) + 10
    yield np.full(n, 7, np.int64)


def probes(t):
    """Below the first entry, every entry and its neighbours, above the last."""
    return np.unique(np.concatenate([t - 1, t, t + 1, [0, 1 << 40]])).astype(np.int64)


@pytest.mark.parametrize("n", LENGTHS)
def test_counts_against_searchsorted(shim, n):
    for t in tables(n, n):
        v = probes(t)
        right, left = np.searchsorted(t, v, "right"), np.searchsorted(t, v, "left")
        for dtype, le, lt in ((np.int64, shim.le_i64, shim.lt_i64), (np.float64, shim.le_f64, shim.lt_f64)):
            scale = 1 if dtype is np.int64 else 0.25              # (exact in float64: the order of the entries stays)
            td, vd = np.ascontiguousarray(t * scale, dtype), np.ascontiguousarray(v * scale, dtype)
            for fn, want in ((le, right), (lt, left)):
                out = np.full(len(v), -1, np.int32)
                fn(p(td), n, p(vd), len(v), 0, p(out))
                assert np.array_equal(out, want), (n, dtype, fn)
                # a nonzero start index: any lower bound of the result gives the same result
                for from_ in sorted({1, 2, n // 2, n - 1, n} & set(range(n + 1))):
                    sel = np.flatnonzero(want >= from_)
                    out = np.full(len(sel), -1, np.int32)
                    fn(p(td), n, p(np.ascontiguousarray(vd[sel])), len(sel), from_, p(out))
                    assert np.array_equal(out, want[sel]), (n, dtype, fn, from_)


@pytest.mark.parametrize("n", LENGTHS[1:])
def test_frames_against_a_direct_loop(shim, n):
    rng = np.random.default_rng(100 + n)
    for t in tables(n, 50 + n):
        off = (t - t[0]).astype(np.uint64)                    # a run's first record starts at row 0
        counts = np.diff(np.concatenate([off, [off[-1] + 5]])).astype(np.int64)
        n_signal = np.minimum(rng.integers(0, 4, n), counts).astype(np.uint32)
        rows = np.unique(np.concatenate([off.astype(np.int64) - 1, off.astype(np.int64), off.astype(np.int64) + 1,
                                         [0, int(off[-1]) + 4]]))
        rows = np.ascontiguousarray(rows[rows >= 0], np.int64)
        f = np.zeros(len(rows), np.int64)
        for g in range(n):                                    # the last record whose ev_offset is <= the row
            f[off[g].astype(np.int64) <= rows] = g
        want = np.stack([f, rows - off[f].astype(np.int64) < n_signal[f]], 1).astype(np.int32)
        out = np.full((len(rows), 2), -1, np.int32)
        shim.frames(p(off), p(n_signal), n, p(rows), len(rows), p(out))
        assert np.array_equal(out, want), n


def test_one_frame_without_records(shim):
    shim.one_frame.argtypes = [C.c_int64, C.c_int64]
    assert [shim.one_frame(i, 3) for i in range(5)] == [1, 1, 1, 0, 0] and shim.one_frame(0, 0) == 0
