"""VideoToEvents(auto_upsample=True) on the MI355X: the segmented max-speed reduction and the ragged prep / fuse / truncation
kernels against the per-batch kernels, and the whole pipeline against the drop-in SuperSloMo(auto_upsample=True) writing PNGs
followed by a per-frame emulator."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(pos_thres=0.15, neg_thres=0.15, sigma_thres=0.03, cutoff_hz=200, leak_rate_hz=0.1, shot_noise_rate_hz=2.0,
          refractory_period_s=0.001)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("b,seg,h,w", [(21, 8, 32, 64), (7, 3, 40, 72), (20, 8, 256, 320), (5, 1, 16, 16)])
def test_segmented_max_speed_equals_the_per_batch_kernel(b, seg, h, w):
    from v2e_amd import _capi
    from v2e_amd._capi import check
    lib = _capi.lib()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(b * 1000 + seg)
    nseg = (b + seg - 1) // seg
    flow = torch.randn((b, 4, h, w), generator=g)
    for j in range(nseg):  # batches of different magnitudes
        flow[j * seg:(j + 1) * seg] *= float(1 + 3 * j)
    zero_batch, nan_batch = (1, nseg - 1) if nseg > 2 else (0, nseg - 1)
    flow[zero_batch * seg:(zero_batch + 1) * seg] = 0.0
    flow[min(nan_batch * seg + 1, b - 1), 3, h // 2, w // 3] = float("nan")
    flow = flow.to(dev).contiguous()
    seg_bits = torch.full((nseg + 1,), 0x1234, dtype=torch.int32, device=dev)  # one slot past the end: must stay untouched
    check(lib.v2e_slomo_max_speed2_seg(_p(flow), b, seg, h, w, _p(seg_bits), _stream()), "v2e_slomo_max_speed2_seg")
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    expect = []
    for j in range(nseg):
        part = flow[j * seg:min((j + 1) * seg, b)].contiguous()
        check(lib.v2e_slomo_max_speed2(_p(part), int(part.shape[0]), h, w, _p(one), _stream()), "v2e_slomo_max_speed2")
        expect.append(int(one.item()))
    got = seg_bits.cpu().tolist()
    assert got[:nseg] == expect and got[nseg] == 0x1234
    assert got[zero_batch] == 0
    assert got[nan_batch] == -1 and sum(1 for v in got[:nseg] if v == -1) == 1  # 0xffffffff: that batch only


def _engine(conv_math, flow_seed=401, interp_seed=402, head=1.0):
    from v2e_amd.slomo import SloMoEngine
    from v2e_amd.synth import portable_unet_state_dict
    sd_f, sd_i = portable_unet_state_dict(2, 4, flow_seed), portable_unet_state_dict(12, 5, interp_seed)
    sd_f["conv3.weight"] = sd_f["conv3.weight"] * np.float32(head)
    sd_f["conv3.bias"] = sd_f["conv3.bias"] * np.float32(head)
    return SloMoEngine({k: torch.from_numpy(v) for k, v in sd_f.items()}, {k: torch.from_numpy(v) for k, v in sd_i.items()},
                       "cuda", conv_math=conv_math)


@pytest.mark.parametrize("cap", [0, 10, 27])
def test_ragged_prep_fuse_trunc_equal_the_per_batch_kernels(cap):
    """Batches with U_b = 2, 5, 3 of 3, 3 and 2 pairs packed into interpolation calls of `cap` samples (0: the whole chunk in one),
    against SloMoEngine.interpolate per batch followed by v2e_f32_to_u8_trunc (time order): bit for bit under the per-sample
    independent conv math."""
    from v2e_amd import _capi
    from v2e_amd._capi import check
    from v2e_amd.pipeline import auto_sample_table
    from v2e_amd.slomo import time_coefficients
    lib = _capi.lib()
    eng = _engine("bf16x3")
    dev = eng.device
    g = torch.Generator().manual_seed(5)
    P, bs, us, h, w, mean = 8, 3, [2, 5, 3], 32, 64, 0.428
    x = (torch.rand((P + 1, 1, h, w), generator=g) - mean).to(dev)
    I0, I1 = x[:P].contiguous(), x[1:].contiguous()
    flow = eng.flow(I0, I1)
    ref_f, ref_q = [], []
    for j, u in enumerate(us):
        b0, b1 = j * bs, min((j + 1) * bs, P)
        ts = [(k + 0.5) / u for k in range(u)]
        Ft = eng.interpolate(I0[b0:b1], I1[b0:b1], ts, flow=flow[b0:b1].contiguous())  # [U,B,1,h,w]
        q = torch.empty(((b1 - b0) * u, h, w), dtype=torch.uint8, device=dev)
        check(lib.v2e_f32_to_u8_trunc(_p(Ft), _p(q), u, b1 - b0, h * w, mean, 1, _stream()), "v2e_f32_to_u8_trunc")
        ref_f.append(Ft[:, :, 0].permute(1, 0, 2, 3).reshape(-1, h, w))  # time order b * U + k
        ref_q.append(q)
    ref_f, ref_q = torch.cat(ref_f), torch.cat(ref_q)
    ts, tab, _ = auto_sample_table(us, P, bs)
    n = len(tab)
    coef = torch.from_numpy(time_coefficients(ts)).to(dev)
    tab_dev = torch.tensor(tab, dtype=torch.int32, device=dev)
    q = torch.full((n, h, w), 7, dtype=torch.uint8, device=dev)
    fr = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    step = cap or n
    for a in range(0, n, step):
        m = min(step, n - a)
        out = eng.interpolate_table(I0, I1, flow, coef, tab_dev, a, m)
        fr[a:a + m] = out[:, 0]
        check(lib.v2e_f32_to_u8_trunc_tab(_p(out), _p(q), _p(tab_dev[a:a + m]), m, h * w, mean, _stream()), "v2e_f32_to_u8_trunc_tab")
    assert torch.equal(fr.view(torch.int32), ref_f.view(torch.int32))
    assert torch.equal(q, ref_q)


def _scaled_ckpt(tmp_path):
    from v2e_amd.synth import portable_unet_state_dict
    sd_f, sd_i = portable_unet_state_dict(2, 4, 401), portable_unet_state_dict(12, 5, 402)
    sd_f["conv3.weight"] = sd_f["conv3.weight"] * np.float32(25.0)  # the fixture of test_auto_upsample_follows_the_flow_magnitude
    sd_f["conv3.bias"] = sd_f["conv3.bias"] * np.float32(25.0)
    ckpt = tmp_path / "ckpt.pt"
    torch.save({"state_dictFC": {k: torch.from_numpy(v) for k, v in sd_f.items()},
                "state_dictAT": {k: torch.from_numpy(v) for k, v in sd_i.items()}}, str(ckpt))
    return ckpt


def _factors_from_times(times, n_pairs, bs):
    """The per-batch factors the drop-in used, read off its interpTimes (batch b starts at time b0, steps 1 / U_b)."""
    out, i = [], 0
    for b0 in range(0, n_pairs, bs):
        nb = min(bs, n_pairs - b0)
        u = int(round(1.0 / (times[i + 1] - times[i])))
        out.append(u)
        i += u * nb
    assert i == len(times)
    return out


def _against_drop_in(tmp_path, monkeypatch, conv_math, n, bs, Ufloor, seed):
    from PIL import Image
    from v2e_amd import EventEmulator, SuperSloMo
    from v2e_amd.pipeline import VideoToEvents
    from v2e_amd.synth import int_gradient_frames
    if conv_math is not None:
        monkeypatch.setenv("V2E_AMD_CONV_MATH", conv_math)
    Hs, Ws = 40, 70
    fr = int_gradient_frames(n, Hs, Ws, seed=seed, noise=10, as_array=True)
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir(); dst.mkdir()
    for i, f in enumerate(fr):
        np.save(str(src / ("%08d.npy" % i)), f)
    sm = SuperSloMo(model=str(_scaled_ckpt(tmp_path)), auto_upsample=True, upsampling_factor=Ufloor, batch_size=bs)
    times, avg = sm.interpolate(str(src), str(dst), (Ws, Hs))
    assert sm.batch_size == bs
    factors = _factors_from_times(times, n - 1, bs)
    assert max(factors) > Ufloor, "the scaled flow head must make some batch exceed the requested factor"
    nout = len(times)
    pngs = np.stack([np.asarray(Image.open(str(dst / ("%d.png" % i)))) for i in range(nout)])
    dt_src = 1 / 30.0
    vt = ((n - 1) * dt_src / (np.max(times) - np.min(times))) * times  # v2e.py:786-797
    ref_emu = EventEmulator(device="cuda", seed=5, rng_mode="philox", **KW)
    ref_ev = [ref_emu.generate_events(p.astype(np.float32), float(t)) for p, t in zip(pngs, vt)]
    ref_counts = np.array([0 if e is None else len(e) for e in ref_ev])
    ref_ev = np.concatenate([e for e in ref_ev if e is not None])
    pipe = VideoToEvents(sm.engine, EventEmulator(device="cuda", seed=5, rng_mode="philox", **KW), Ufloor, batch_size=bs,
                         auto_upsample=True)
    frames_dev = torch.from_numpy(fr).cuda()
    up = pipe.upsample(frames_dev).cpu().numpy()
    assert pipe.upsampling_factors == factors and pipe.avg_upsampling_factor == avg
    assert np.array_equal(pipe.interpTimes, times) and up.shape == pngs.shape
    ev, counts, nfr = pipe.run(frames_dev, dt_src)
    assert nfr == nout and len(counts) == nout and pipe.upsampling_factors == factors
    return pipe, up, pngs, ev, counts, ref_ev, ref_counts


def _check(conv_math, pipe, up, pngs, ev, counts, ref_ev, ref_counts):
    diff = np.abs(up.astype(np.int16) - pngs.astype(np.int16))
    frac = float((diff > 0).mean())
    rel = abs(int(counts.sum()) - len(ref_ev)) / max(1, len(ref_ev))
    print("auto_upsample vs drop-in (%s): factors %s, %d frames, host syncs %d, max grey diff %d on %.4f %% of pixels, "
          "events %d vs %d (%.4f %%)" % (conv_math or "default", pipe.upsampling_factors, len(up), pipe.host_syncs, int(diff.max()),
                                         100 * frac, int(counts.sum()), len(ref_ev), 100 * rel))
    if conv_math == "bf16x3":
        assert np.array_equal(up, pngs), "device frames differ from the PNG frames"
        assert np.array_equal(counts, ref_counts) and np.array_equal(ev, ref_ev)
    else:  # packed calls share one activation scale: the bounds of the config-3 comparison
        assert diff.max() <= 1 and frac < 1e-3
        assert rel <= 2e-3


@pytest.mark.parametrize("conv_math", ["bf16x3", None])
def test_auto_pipeline_equals_the_drop_in(tmp_path, monkeypatch, conv_math):
    """The fixture of test_auto_upsample_follows_the_flow_magnitude: 7 frames of 40 x 70, batches of 2, minimum factor 3."""
    r = _against_drop_in(tmp_path, monkeypatch, conv_math, 7, 2, 3, 19)
    assert r[0].host_syncs == 1
    _check(conv_math, *r)


@pytest.mark.parametrize("conv_math", ["bf16x3", None])
def test_auto_pipeline_over_several_flow_chunks(tmp_path, monkeypatch, conv_math):
    """150 source frames in batches of 8: three flow chunks (64, 64, 21 pairs; a short last batch), one factor read-back each,
    the next chunk's flow UNet queued ahead of it."""
    r = _against_drop_in(tmp_path, monkeypatch, conv_math, 150, 8, 3, 23)
    assert r[0].host_syncs == 3 and len(r[0].upsampling_factors) == 19
    _check(conv_math, *r)
