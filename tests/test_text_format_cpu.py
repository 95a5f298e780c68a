"""CPU: the text sink's time stamp formatter (v2e_amd/csrc/text_format.h) through its host entry point
v2e_events_format_text_host -- the same __host__ __device__ code the GPU kernels run -- against Python's own formatting of
the float64 value of a float32 time stamp, '{}'.format(np.float64(t)) as ae_text_output.py:86-101 writes it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_text(ev, labels=False, n_signal=0, ev_offset=None, frame_n_signal=None):
    from v2e_amd import _capi
    from v2e_amd.sinks import _frame_recs
    lib = _capi.lib()
    ev = np.ascontiguousarray(ev, dtype=np.float32)
    recs, nrec = None, 0
    if ev_offset is not None:
        rec = _frame_recs(ev_offset, frame_n_signal)
        recs, nrec = rec.ctypes.data, len(rec)
    total = C.c_int64()
    rc = lib.v2e_events_format_text_host(ev.ctypes.data, len(ev), recs, nrec, n_signal, int(labels), None, 0, C.byref(total))
    assert rc == (0 if total.value == 0 else -75)  # V2E_EOVERFLOW: a buffer of 0 bytes is too small, nothing written
    buf = np.empty(max(total.value, 1), np.uint8)
    assert lib.v2e_events_format_text_host(ev.ctypes.data, len(ev), recs, nrec, n_signal, int(labels), buf.ctypes.data,
                                           total.value, C.byref(total)) == 0
    return buf[:total.value].tobytes()


def time_rows(t):
    ev = np.zeros((len(t), 4), np.float32)
    ev[:, 0] = t
    ev[:, 3] = -1.0
    return ev


def check_times(t):
    """Every value's line `t 0 0 0` against Python's repr of float64(t) (repr(float) and '{}'.format(np.float64) agree; the
    latter is checked on a sample, the former on all)."""
    got = host_text(time_rows(t))
    want = "".join("%s 0 0 0\n" % r for r in map(repr, t.astype(np.float64).tolist())).encode()
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [(i, g[i], w[i]) for i in range(min(len(g), len(w))) if g[i] != w[i]]
        raise AssertionError("%d of %d lines differ, first: %r" % (len(bad), len(t), bad[:5]))
    sample = t[:: max(1, len(t) // 2000)]
    assert [l.split(b" ")[0].decode() for l in host_text(time_rows(sample)).splitlines()] == \
        ['{}'.format(np.float64(v)) for v in sample]


def test_pow5_table_is_the_generator_output():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "v2e_amd", "csrc", "gen_pow5.py")])
    assert out == open(os.path.join(ROOT, "v2e_amd", "csrc", "pow5_table.h"), "rb").read()


def test_every_float32_of_the_binade_holding_1_over_300():
    lo, hi = np.float32(2.0 ** -9).view(np.uint32), np.float32(2.0 ** -8).view(np.uint32)
    assert lo <= np.float32(1 / 300).view(np.uint32) < hi
    bits = np.arange(lo, hi, dtype=np.uint32)
    assert len(bits) == 1 << 23
    check_times(bits.view(np.float32))


def test_random_finite_bit_patterns_across_all_exponents():
    rng = np.random.default_rng(20261016)
    bits = rng.integers(0, 1 << 32, 2_100_000, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7F800000) != 0x7F800000][:2_000_000]
    assert len(bits) == 2_000_000 and len(np.unique(bits >> 23 & 0xFF)) == 255  # every finite exponent, subnormals included
    check_times(bits.view(np.float32))


def test_edge_values():
    f32 = np.float32
    vals = [0.0, -0.0, np.float32(1e-45), -np.float32(1e-45), np.finfo(f32).max, -np.finfo(f32).max, np.finfo(f32).tiny,
            np.nextafter(np.finfo(f32).tiny, f32(0)), 1.0, -1.0, 0.5, 2.0, 3.0, 10.0, 100.0, 1 / 300, 2 / 300, 0.1, 0.2, 0.3,
            16777216.0, 16777217.0, 123456789.0, 1e15, 9999999583119360.0, 1e16, 1e17, 1e18, 1e19, 1e20, 3e16]
    vals += [2.0 ** k for k in range(-149, 128)]
    for edge in (f32(1e-4), f32(1e16), f32(1e-5), f32(1e-3)):  # both sides of the notation switches
        vals += [np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(np.inf))]
    vals += [f32(k) / f32(300) for k in range(1, 400)] + [f32(k) for k in range(0, 2000, 7)]
    t = np.array(vals, dtype=np.float32)
    t = np.concatenate([t, -t])
    check_times(t)
    lens = [len(repr(float(v))) for v in t]
    assert max(lens) <= 24 and any(len(repr(float(v)).replace("-", "").replace("0.", "").split("e")[0]) >= 17 for v in t)
    # nan, inf: as numpy prints them
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, np.float32(np.nan) * 0], dtype=np.float32)
    assert host_text(time_rows(special)).decode().split("\n")[:-1] == \
        ['{} 0 0 0'.format(np.float64(v)) for v in special]


def test_whole_lines_with_labels_across_frame_boundaries():
    """Line layout of ae_text_output.py:86-101 with and without the label column; the label per frame of a run (its first
    n_signal rows signal), frames with no rows in between, and the one-frame form (n_signal only)."""
    rng = np.random.default_rng(3)
    n = 3000
    ev = np.stack([np.sort(rng.uniform(0, 2, n)).astype(np.float32), rng.integers(0, 346, n), rng.integers(0, 260, n),
                   rng.choice([-1.0, 1.0], n)], axis=1).astype(np.float32)
    t = ev[:, 0].astype(float)
    x, y = ev[:, 1].astype(np.int32), ev[:, 2].astype(np.int32)
    p = ((ev[:, 3] + 1) / 2).astype(np.int32)
    plain = "".join('{} {} {} {}\n'.format(t[i], x[i], y[i], p[i]) for i in range(n)).encode()
    assert host_text(ev) == plain
    off = np.array([0, 700, 700, 1500, 2999])
    nsig = np.array([650, 5, 800, 0, 1])
    lab = np.zeros(n, bool)
    for o, k in zip(off, nsig):
        lab[o:o + k] = True
    want = "".join('{} {} {} {} {}\n'.format(t[i], x[i], y[i], p[i], int(lab[i])) for i in range(n)).encode()
    assert host_text(ev, labels=True, ev_offset=off, frame_n_signal=nsig) == want
    one = "".join('{} {} {} {} {}\n'.format(t[i], x[i], y[i], p[i], int(i < 1234)) for i in range(n)).encode()
    assert host_text(ev, labels=True, n_signal=1234) == one
    from v2e_amd.sinks import frames_from_labels
    assert host_text(ev, labels=True, ev_offset=frames_from_labels(lab)[0], frame_n_signal=frames_from_labels(lab)[1]) == want


def test_zero_rows_and_a_buffer_too_small():
    from v2e_amd import _capi
    lib = _capi.lib()
    total = C.c_int64(-1)
    assert lib.v2e_events_format_text_host(None, 0, None, 0, 0, 0, None, 0, C.byref(total)) == 0 and total.value == 0
    ev = time_rows(np.array([1 / 300, 2 / 300], np.float32))
    buf = np.full(64, 7, np.uint8)
    assert lib.v2e_events_format_text_host(ev.ctypes.data, 2, None, 0, 0, 0, buf.ctypes.data, 40, C.byref(total)) == -75
    assert total.value == len(b"0.0033333334140479565 0 0 0\n0.006666666828095913 0 0 0\n") and (buf == 7).all()
