"""GPU: the text lines made by v2e_events_format_text equal the host entry point's (the same __host__ __device__ code, checked
against Python in tests/test_text_format_cpu.py) over a sweep of 2^26 float32 bit patterns, and Python's formatting of
whole lines with and without labels; the AEDAT-2.0 noise bit per frame of a run."""
import os

import numpy as np
import pytest

from test_text_format_cpu import host_text, time_rows
from fixtures import GOLDEN


@pytest.mark.gpu
def test_device_lines_equal_host_entry_over_2_to_26_values():
    import torch
    from v2e_amd.sinks import format_text
    step = 1 << 6  # every 64th bit pattern of all 2^32: every exponent and sign, nan and inf included
    chunk = 1 << 24
    out = None
    for c0 in range(0, 1 << 32, chunk * step):
        bits = np.arange(c0, c0 + chunk * step, step, dtype=np.uint64).astype(np.uint32) + np.uint32((c0 // (chunk * step)) * 7)
        ev = time_rows(bits.view(np.float32))
        ev[:, 1] = (bits & 0x1FF).astype(np.float32)
        ev[:, 2] = (bits >> 9 & 0xFF).astype(np.float32)
        ev[:, 3] = np.where(bits & 1, 1.0, -1.0)
        want = np.frombuffer(host_text(ev), np.uint8)
        if out is None or out.numel() < len(want):
            out = torch.empty(len(want) + (1 << 20), dtype=torch.uint8, device="cuda")
        got, total = format_text(torch.from_numpy(ev).cuda(), out=out)
        assert total == len(want)
        assert np.array_equal(got[:total].cpu().numpy(), want)


@pytest.mark.gpu
def test_device_lines_equal_python_with_and_without_labels():
    import torch
    from v2e_amd.sinks import format_text
    rng = np.random.default_rng(5)
    n = 20000
    ev = np.stack([np.sort(rng.uniform(0, 30, n)).astype(np.float32), rng.integers(0, 1280, n), rng.integers(0, 720, n),
                   rng.choice([-1.0, 1.0], n)], axis=1).astype(np.float32)
    ev[:50, 0] = rng.uniform(0, 1e-4, 50).astype(np.float32)  # a few exponent-notation stamps
    dev = torch.from_numpy(ev).cuda()
    t = ev[:, 0].astype(float)
    x, y = ev[:, 1].astype(np.int32), ev[:, 2].astype(np.int32)
    p = ((ev[:, 3] + 1) / 2).astype(np.int32)
    got, total = format_text(dev)
    assert got[:total].cpu().numpy().tobytes() == "".join('{} {} {} {}\n'.format(t[i], x[i], y[i], p[i]) for i in range(n)).encode()
    off = np.array([0, 256, 256, 257, 5000, 5000, 12345, 19999])  # frame boundaries inside workgroups, empty frames
    nsig = np.array([200, 0, 7, 3000, 1, 7000, 6000, 1])
    lab = np.zeros(n, bool)
    for o, k in zip(off, nsig):
        lab[o:o + k] = True
    got, total = format_text(dev, labels=True, frames=(off, nsig))
    want = "".join('{} {} {} {} {}\n'.format(t[i], x[i], y[i], p[i], int(lab[i])) for i in range(n)).encode()
    assert got[:total].cpu().numpy().tobytes() == want
    got, total = format_text(dev, labels=True, n_signal=777)
    want = "".join('{} {} {} {} {}\n'.format(t[i], x[i], y[i], p[i], int(i < 777)) for i in range(n)).encode()
    assert got[:total].cpu().numpy().tobytes() == want


@pytest.mark.gpu
def test_zero_rows_and_a_buffer_too_small():
    import torch
    from v2e_amd import _capi
    from v2e_amd.sinks import format_text
    got, total = format_text(torch.empty((0, 4), dtype=torch.float32, device="cuda"))
    assert total == 0
    ev = torch.from_numpy(time_rows(np.array([1 / 300] * 1000, np.float32))).cuda()
    out = torch.full((1000,), 7, dtype=torch.uint8, device="cuda")
    with pytest.raises(_capi.V2EAmdError, match="needs 28000 bytes"):
        format_text(ev, out=out)
    assert bool((out == 7).all())


@pytest.mark.gpu
def test_aedat2_noise_bit_per_frame_of_a_run():
    """v2e_events_pack_aedat2_run: the bytes of packing each frame with its own noise_from (the per-frame path, golden-pinned
    by tests/test_sinks.py), concatenated."""
    import torch
    from v2e_amd import _capi
    from v2e_amd._capi import ptr as _ptr
    from v2e_amd.sinks import _frame_recs, _AEDAT2_LAYOUT, pack_aedat2
    import ctypes as C
    z = np.load(os.path.join(GOLDEN, "sinks.npz"))
    ev = torch.from_numpy(z["ev_346x260"]).cuda()
    n = int(ev.shape[0])
    off = np.array([0, 1000, 1000, 2500, 4999])
    nsig = np.array([900, 3, 1400, 2000, 0])
    ends = list(off[1:]) + [n]
    want = np.concatenate([pack_aedat2(ev[o:e], 346, 260, noise_from=k).cpu().numpy() for o, e, k in zip(off, ends, nsig)])
    rec = torch.from_numpy(_frame_recs(off, nsig).view(np.uint8)).cuda()
    out = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
    xs, ys, ps, fx, fy = _AEDAT2_LAYOUT[(346, 260)]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.lib().v2e_events_pack_aedat2_run(_ptr(ev), _ptr(out), n, 346, 260, xs, ys, ps, fx, fy, _ptr(rec), len(off), s),
                "v2e_events_pack_aedat2_run")
    assert np.array_equal(out.cpu().numpy(), want)
    _capi.check(_capi.lib().v2e_events_pack_aedat2_run(_ptr(ev), _ptr(out), n, 346, 260, xs, ys, ps, fx, fy, None, 0, s), "run")
    assert np.array_equal(out.cpu().numpy(), pack_aedat2(ev, 346, 260).cpu().numpy())
