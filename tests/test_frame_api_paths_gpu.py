"""Where v2e_emu_frame puts a frame's rows: every branch of the function's tail against the oracle, bit for bit.

The call copies the rows a frame is EXPECTED to have (at least 1 024, at most the buffer's capacity) with the frame's
last kernel, and what happens after the one synchronisation depends on how many rows there were: nothing more, the rest
of the rows, a larger buffer first, the handle's buffer instead of the caller's, or the hand-over to the step-wise entry
points (rc 1: tests/test_emulator_gpu.py::test_many_iterations_grow_scratch; rc 2: here).  Each case asserts the row
count that puts it on its branch.  33 x 37 uint8 frames, Philox mode, sigma_thres = 0: a 0 -> 255 step makes
floor(log(255) / threshold) ON events at every pixel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 33, 37
EST_FLOOR = 1024       # v2e_emu_frame's estimate never goes below this
OWN_ROWS = 1 << 16     # the smallest pinned buffer of the handle's own, and generate_events' smallest device buffer
DT = 0.01


def _kw(thres):
    return dict(pos_thres=thres, neg_thres=thres, sigma_thres=0.0, cutoff_hz=0, leak_rate_hz=0, shot_noise_rate_hz=0,
                refractory_period_s=0)


def _grey(v):
    return np.full((H, W), v, np.uint8)


def _same_rows(a, b):
    if b is None:
        b = np.zeros((0, 4), np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class _Direct:
    """v2e_emu_frame called as a C caller would, on the handle of an EventEmulator that has seen its first frame."""

    def __init__(self, oracle_lib, thres, max_iters, seed=5):
        from v2e_amd import EventEmulator
        self.emu = EventEmulator(device="cuda", rng_mode="philox", seed=seed, max_iters=max_iters, **_kw(thres))
        self.ora = oracle_lib.OracleEmulator(rng_mode="philox", seed=seed, **_kw(thres))
        assert self.emu.generate_events(_grey(0), 0.0) is None and self.ora.generate_events(_grey(0), 0.0) is None
        self.eng = self.emu._engine
        self.ev = torch.empty((1, 1 << 18, 4), dtype=torch.float32, device="cuda")
        self.t, self.fidx = 0.0, 1

    def frame(self, grey, user=None, user_cap=0):
        """(rows, where) of the next frame; `where`: the address the library returned the rows at (None: no rows)."""
        from v2e_amd._capi import check
        eng, f = self.eng, _grey(grey)
        t = self.t + DT
        if user is not None:
            check(eng.lib.v2e_emu_frame_host_rows(eng._h, C.c_void_p(user.data_ptr()), user_cap), "v2e_emu_frame_host_rows")
        out8 = (C.c_uint32 * 8)()
        rows = C.POINTER(C.c_float)()
        rc = eng.lib.v2e_emu_frame(eng._h, C.byref(self.emu._params()), C.c_void_p(f.ctypes.data), 1, 0, self.t, t, self.fidx,
                                   C.c_void_p(self.ev.data_ptr()), int(self.ev.shape[1]), out8, C.byref(rows), eng.stream)
        assert rc == 0, (rc, eng.lib.v2e_last_error())
        n = int(out8[0])
        got = np.empty((n, 4), np.float32)
        where = C.cast(rows, C.c_void_p).value
        if n:
            C.memmove(got.ctypes.data, rows, 16 * n)
        else:
            assert where is None
        ref = self.ora.generate_events(f, t)
        assert _same_rows(got, ref), "frame %d: %d rows, the oracle has %d" % (self.fidx, n, 0 if ref is None else len(ref))
        self.t, self.fidx = t, self.fidx + 1
        return got, where


@pytest.mark.parametrize("thres,grows", [(0.2, False), (0.04, True)])
def test_short_estimate_own_rows(oracle_lib, thres, grows):
    """A quiet frame leaves the estimate at its floor; the step frame has more rows than that, so the rest of them follow
    in a second copy -- into the handle's buffer as it is (thres 0.2: fewer rows than the buffer holds) or into a larger
    one that has to keep the rows of the first copy (thres 0.04)."""
    d = _Direct(oracle_lib, thres, max_iters=256)
    assert len(d.frame(0)[0]) == 0
    n = len(d.frame(255)[0])
    assert n == H * W * d.ora.last["M"] and d.ora.last["M"] <= 256
    assert (n > OWN_ROWS) if grows else (EST_FLOOR < n <= OWN_ROWS)
    assert 0 < len(d.frame(128)[0]) < n


def test_callers_buffer_short_estimate(oracle_lib):
    """The caller's pinned buffer holds the frame, the estimate does not: the second copy goes to the caller's buffer too."""
    d = _Direct(oracle_lib, 0.2, max_iters=64)
    user = torch.zeros((OWN_ROWS, 4), dtype=torch.float32).pin_memory()
    assert len(d.frame(0)[0]) == 0
    rows, where = d.frame(255, user, OWN_ROWS)
    assert EST_FLOOR < len(rows) <= OWN_ROWS
    assert where == user.data_ptr()
    assert _same_rows(user[:len(rows)].numpy(), rows)


def test_callers_buffer_too_small(oracle_lib):
    """16 rows of caller's buffer for a frame of thousands: all rows arrive in the handle's buffer (which this call is the
    first to allocate), and the caller's buffer is not used for the frame after it."""
    d = _Direct(oracle_lib, 0.2, max_iters=64)
    user = torch.zeros((16, 4), dtype=torch.float32).pin_memory()
    assert len(d.frame(0, user, 16)[0]) == 0
    rows, where = d.frame(255, user, 16)
    assert len(rows) > EST_FLOOR
    assert where is not None and where != user.data_ptr()
    rows, where = d.frame(128)
    assert len(rows) > 16 and where != user.data_ptr()


def test_more_rows_than_the_event_buffer(oracle_lib):
    """rc 2: the step frame has more rows than generate_events' device buffer holds and no more iterations than the scratch:
    v2e_emu_frame counts it, hands it to the ring, and the step-wise entry points finish it."""
    from v2e_amd import EventEmulator
    kw = _kw(0.08)
    hip = EventEmulator(device="cuda", rng_mode="philox", seed=9, max_iters=128, **kw)
    ora = oracle_lib.OracleEmulator(rng_mode="philox", seed=9, **kw)
    rcs = []
    for i, g in enumerate((0, 0, 255, 128)):
        a = hip.generate_events(_grey(g), DT * i)
        if i == 0:
            eng_frame = hip._engine.frame
            hip._engine.frame = lambda *args: rcs.append(eng_frame(*args)) or rcs[-1]
        b = ora.generate_events(_grey(g), DT * i)
        assert _same_rows(np.zeros((0, 4), np.float32) if a is None else a, b)
        if g == 255:
            assert len(b) > OWN_ROWS and ora.last["M"] <= 128
    assert [rc for rc, _, _ in rcs] == [0, 2, 0]


def test_more_rows_than_the_event_buffer_with_a_text_file_open(oracle_lib, tmp_path):
    """rc 2 with an event file open: the step-wise entry points finish the frame and its rows reach the file once, through the
    same frame tail as the one-call frame's.  8 x 70 pixels stepping 0 -> 255 -> 128 with thresholds 0.02: more rows than
    generate_events' device buffer holds, no more iterations than the scratch.  The twin's device buffer is grown beforehand, so
    every frame of its is the one-call frame (rc 0): the same rows (the oracle's), counters and file."""
    from v2e_amd import EventEmulator
    frames = [np.full((8, 70), g, np.uint8) for g in (0, 0, 255, 128)]
    ora = oracle_lib.OracleEmulator(rng_mode="philox", seed=3, **_kw(0.02))
    ref = [ora.generate_events(f, DT * i) for i, f in enumerate(frames)]
    assert len(ref[2]) > OWN_ROWS > len(ref[3]) > 0 and len(ref[2]) <= 8 * 70 * 512  # (every pixel makes the same events)

    def run(name, grow_first):
        emu = EventEmulator(device="cuda", rng_mode="philox", seed=3, max_iters=512, output_folder=str(tmp_path), dvs_text=name,
                            **_kw(0.02))
        rcs, rows = [], []
        for i, f in enumerate(frames):
            rows.append(emu.generate_events(f, DT * i))
            if i == 0:
                if grow_first:
                    emu._engine.event_buffer(1 << 18)
                eng_frame = emu._engine.frame
                emu._engine.frame = lambda *args: rcs.append(eng_frame(*args)) or rcs[-1]
        state = (emu.num_events_total, emu.num_events_on, emu.num_events_off, emu.t_previous, emu.frame_counter)
        emu.cleanup()
        lines = open(str(tmp_path / (name + ".txt")), "rb").read().split(b"\n")
        return rows, [rc for rc, _, _ in rcs], state, [l for l in lines if not l.startswith(b"#")]

    rows, rcs, state, lines = run("grown", False)
    twin_rows, twin_rcs, twin_state, twin_lines = run("twin", True)
    assert rcs == [0, 2, 0] and twin_rcs == [0, 0, 0]
    for a, b, c in zip(rows, twin_rows, ref):
        assert (a is None) == (b is None) == (c is None) and (a is None or (_same_rows(a, c) and _same_rows(b, c)))
    assert state == twin_state == (len(ref[2]) + len(ref[3]), len(ref[2]), len(ref[3]), DT * 3, 4)
    assert lines == twin_lines and len(lines) == state[0] + 1
