"""CPU-only: the C-ABI library loads and exports every symbol include/v2e_amd.h declares
(no compute calls), and the host logic of the drop-in classes behaves like the reference's."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "v2e_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(v2e_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from v2e_amd import _capi
    syms = _declared_symbols()
    assert len(syms) >= 20
    assert sorted(_capi.SIGNATURES) == syms, "ctypes table and header disagree"
    lib = _capi.lib()  # raises if the .so or a symbol is missing
    for s in syms:
        assert hasattr(lib, s)
    assert lib.v2e_version() >= 100
    assert lib.v2e_emu_npx_pad(260, 346) == 90112


def test_struct_layouts_match_header():
    import ctypes as C
    from v2e_amd._capi import ConvDesc, EmuParams, FrameRec
    assert C.sizeof(FrameRec) == 32
    assert C.sizeof(EmuParams) == 16 + 12 * 8 + 8 + 8 + 8 + 8  # ... + log_input, photoreceptor_noise, vrms
    assert C.sizeof(ConvDesc) == 40 and ConvDesc.weight_s3.offset == 32  # two pointers, 3 ints + pad, split-bf16 weights


def test_run_flags_match_header():
    from v2e_amd import _capi
    src = open(os.path.join(ROOT, "include", "v2e_amd.h")).read()
    header = {k: int(v) for k, v in re.findall(r"^#define V2E_(RUN_[A-Z_]+) (\d+)\b", src, flags=re.M)}
    python = {k: v for k, v in vars(_capi).items() if k.startswith("RUN_")}
    assert len(header) == 7 and header == python
    assert (header["RUN_GRAPH"], header["RUN_PROFILE"], header["RUN_PIPELINED"]) == (1, 2, 1024)  # bench.py passes these values


def test_emulator_constructor_surface():
    import inspect
    from v2e_amd import EventEmulator
    ref_args = ["pos_thres", "neg_thres", "sigma_thres", "cutoff_hz", "leak_rate_hz", "refractory_period_s",
                "shot_noise_rate_hz", "photoreceptor_noise", "leak_jitter_fraction", "noise_rate_cov_decades", "seed",
                "output_folder", "dvs_h5", "dvs_aedat2", "dvs_aedat4", "dvs_text", "show_dvs_model_state",
                "save_dvs_model_state", "output_width", "output_height", "device", "cs_lambda_pixels", "cs_tau_p_ms",
                "hdr", "scidvs", "record_single_pixel_states", "label_signal_noise"]  # emulator.py:86-117
    params = list(inspect.signature(EventEmulator.__init__).parameters)[1:]
    assert params[:len(ref_args)] == ref_args
    e = EventEmulator()
    assert (e.pos_thres, e.neg_thres, e.sigma_thres, e.leak_rate_hz, e.cutoff_hz) == (0.2, 0.2, 0.03, 0.1, 0.0)
    assert e.num_events_total == 0 and e.t_previous == 0
    assert "lp_log_frame" in EventEmulator.MODEL_STATES and EventEmulator.SINGLE_PIXEL_STATES_FILENAME
    e.set_dvs_params("noisy")  # emulator.py:525-535
    assert (e.sigma_thres, e.cutoff_hz, e.leak_rate_hz, e.shot_noise_rate_hz, e.refractory_period_s) == (0.05, 30, 0.1, 5.0, 0)
    assert e.pos_thres_nominal == 0.2
    e.set_dvs_params("clean")
    assert (e.sigma_thres, e.cutoff_hz, e.leak_rate_hz, e.shot_noise_rate_hz) == (0.02, 0, 0, 0)


def test_emulator_errors_like_reference(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from v2e_amd import EventEmulator
    e = EventEmulator()
    e.t_previous = 1.0
    with pytest.raises(ValueError):  # emulator.py:650-653
        e.generate_events(np.zeros((4, 4), np.uint8), 0.5)
    EventEmulator(cs_lambda_pixels=2.0, cs_tau_p_ms=2.0)  # CSDVS: built (tests/test_csdvs.py)
    EventEmulator(scidvs=True)  # SCIDVS with float32 state (no cutoff): built (torch's float32 sinh restated, v2e_detmath.h)
    # research tooling: accepted as host pass-throughs (emulator.py:279-300, 365-368), validated as the reference does
    e2 = EventEmulator(show_dvs_model_state=["all"], record_single_pixel_states=(1, 2), rng_mode="philox")
    assert list(e2.show_dvs_model_state) == list(EventEmulator.MODEL_STATES) and e2.single_pixel_states["time"].shape == (10000,)
    e2.record_single_pixel_states = None  # nothing recorded: no pickle file from cleanup()
    for bad in ([1, 2], (1, 2, 3), (1.0, 2)):
        with pytest.raises(ValueError):
            EventEmulator(record_single_pixel_states=bad)
    with pytest.raises(SystemExit):  # emulator.py:196-204: v2e_quit when the rate or the cutoff is zero
        EventEmulator(photoreceptor_noise=True, shot_noise_rate_hz=0.0, cutoff_hz=10)
    e = EventEmulator(photoreceptor_noise=True, shot_noise_rate_hz=1.0, cutoff_hz=10, rng_mode="tape")
    with pytest.raises(ValueError):  # device-resident clips need the Philox streams (tape mode needs the host per frame)
        e.generate_events_batch(np.zeros((2, 4, 4), np.uint8), [0.0, 0.1])
    with pytest.raises(ValueError):
        EventEmulator(rng_mode="bogus")


def test_no_cpu_fallback():
    import torch
    from v2e_amd import EventEmulator, V2EAmdError
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    e = EventEmulator(device="cuda")
    with pytest.raises(V2EAmdError):
        e.generate_events(np.zeros((8, 8), np.uint8), 0.0)


def test_slomo_constructor_surface():
    import inspect
    from v2e_amd import SuperSloMo
    params = list(inspect.signature(SuperSloMo.__init__).parameters)[1:]
    assert params == ["model", "auto_upsample", "upsampling_factor", "batch_size", "video_path", "vid_orig",
                      "vid_slomo", "preview", "avi_frame_rate"]  # slomo.py:44-54
    with pytest.raises(ValueError):  # slomo.py:91-94
        SuperSloMo("x.ckpt", auto_upsample=False, upsampling_factor=1)
    s = SuperSloMo("x.ckpt", auto_upsample=False, upsampling_factor=4)
    ts = s.get_interpolated_timestamps(np.array([0.0, 1.0, 2.0]))  # slomo.py:540-564
    assert np.allclose(ts, [0.125, 0.375, 0.625, 0.875, 1.125, 1.375, 1.625, 1.875])
    with pytest.raises(ValueError):
        s.interpolate("/nonexistent", None, (64, 32))


def test_synthetic_generators_are_reproducible():
    from v2e_amd.synth import int_gradient_frames, portable_unet_state_dict, unet_layer_shapes
    import hashlib
    a = int_gradient_frames(3, 20, 30, seed=1, noise=6, as_array=True)
    assert hashlib.sha256(a.tobytes()).hexdigest()[:16] == hashlib.sha256(
        int_gradient_frames(3, 20, 30, seed=1, noise=6, as_array=True).tobytes()).hexdigest()[:16]
    assert a.dtype == np.uint8 and a.std() > 5
    shapes = unet_layer_shapes(12, 5)
    assert len(shapes) == 23 and shapes[13] == ("up1.conv2", 512, 1024, 3)
    sd = portable_unet_state_dict(2, 4, 1)
    n = sum(v.size for v in sd.values())
    assert n == 19_786_660 or abs(n - 19.79e6) < 0.02e6  # 19.79 M params


def test_time_coefficients_are_python_doubles_first():
    from v2e_amd.slomo import time_coefficients
    c = time_coefficients([0.05])
    t = 0.05
    assert c[0, 0] == np.float32(-t * (1 - t)) and c[0, 2] == np.float32((1 - t) * (1 - t)) and c[0, 4] == np.float32(1 - t)


def test_photoreceptor_noise_amplitude_port():
    """The noise-amplitude estimate (emulator_utils.py:177-290 restated; unseeded draws like the reference) lands where
    the reference's does for the v2e defaults: 0.0615 +- 0.001 measured with the reference function itself."""
    from v2e_amd.emulator import photoreceptor_noise_vrms
    v = [photoreceptor_noise_vrms(1.0, 300.0, 3000.0, 0.2, 0.2, 0.03) for _ in range(4)]
    assert 0.055 < np.mean(v) < 0.068
    # lower rate per Hz of bandwidth -> less noise needed; higher threshold -> more
    assert photoreceptor_noise_vrms(0.01, 300.0, 3000.0, 0.2, 0.2, 0.03) < np.mean(v)
    assert photoreceptor_noise_vrms(1.0, 300.0, 3000.0, 0.4, 0.4, 0.03) > np.mean(v)


@pytest.mark.parametrize("has_refr", [0, 1])
@pytest.mark.parametrize("fused", [0, 1])
def test_chain_launch_schedule_invariants(has_refr, fused):
    """v2e_emu_chain_plan, the schedule v2e_emu_run enqueues (no GPU needed): every frame is advanced exactly once and in
    order; with a refractory period every launch validates exactly its predecessor's frames and a tail launch validates the
    last ones; an emission batch is launched once, in order, and only when all its frames are final (validated, or -- without
    a refractory period -- advanced); a ring slot is not overwritten before the emission batch that reads it was waited for;
    k_ahead batches are produced before the launch that needs them and never more than the ring holds."""
    import ctypes as C
    from v2e_amd import _capi
    lib = _capi.lib()
    for K, m in ((1, 1), (1, 8), (1, 32), (2, 1), (3, 2), (5, 6), (8, 1), (8, 4), (11, 2), (16, 2), (32, 1), (32, 2)):
        E = K * m
        for nD in (3, 5):
            D = nD * E
            for F in list(range(1, 2 * D + 5, max(1, D // 7))) + [300]:
                n = lib.v2e_emu_chain_plan(F, K, E, nD, has_refr, fused, None, 0)
                buf = (C.c_int32 * (8 * n))()
                assert lib.v2e_emu_chain_plan(F, K, E, nD, has_refr, fused, buf, n) == n
                plan = np.frombuffer(buf, dtype=np.int32).reshape(n, 8)
                nb = (F + E - 1) // E
                advanced, final, emitted, waited, ahead = 0, 0, [], set(), {0, 1} if not fused else set()
                for L, (f0, nf, pf0, pnf, wj, wa, an, eb) in enumerate(plan):
                    if wj >= 0:
                        assert wj in emitted, "waits for an emission batch that was never launched"
                        waited.add(wj)
                    if wa >= 0:
                        assert not fused and wa in ahead, "needs records no k_ahead launch produced"
                    assert f0 == advanced and 0 <= nf <= K, "frames must be advanced once, in order"
                    for f in range(f0, f0 + nf):  # the slot of frame f was last used by frame f - D
                        assert f < D or (f - D) // E in waited, "ring slot reused before its emission batch was waited for"
                    if has_refr:
                        assert (pnf == 0) == (L == 0)
                        if L > 0:
                            assert (pf0, pnf) == (plan[L - 1][0], plan[L - 1][1]), "validates something else than its predecessor"
                            final = pf0 + pnf
                    else:
                        assert pnf == 0
                    advanced += nf
                    if not has_refr:
                        final = advanced
                    if an >= 0:
                        assert not fused and an not in ahead and an < nb
                        # its records overwrite those of batch an - nD, whose frames (and their redo) must be behind the chain
                        assert an < nD or (an - nD + 1) * E <= f0 + nf
                        ahead.add(an)
                    if eb >= 0:
                        assert eb == len(emitted), "emission batches in order, once"
                        assert min((eb + 1) * E, F) <= final, "batch launched before its frames are final"
                        emitted.append(eb)
                assert advanced == F and final == F and emitted == list(range(nb))
                assert (plan[-1][1] == 0) == bool(has_refr), "a tail launch iff there is something left to validate"
                if not fused:
                    assert ahead >= set(range(nb))
