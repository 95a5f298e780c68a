"""The headline configuration (bench.py: 346x260, CLI-default DVS, 300 frames per step) keeps 32 frames per chain launch with the
redo rendezvous.  k_chain decodes a sub-pass's records into registers, so its register count sets how many of its workgroups a CU
holds; if the 352 workgroups no longer passed the plan-time co-residency check, the run would fall back to one frame per launch
without any result changing.  This test is what notices."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_headline_runs_32_frame_launches_with_rendezvous():
    import bench
    from v2e_amd import EventEmulator
    from v2e_amd.benchutil import run_steps
    dev = torch.device("cuda", 0)
    F = bench.FRAMES_PER_STEP
    frames = bench.gen_frames_device(2 * F + 1, 1, dev)
    emu = EventEmulator(device=dev, seed=1, rng_mode="philox", **bench.DEFAULT_KW)
    emu.generate_events(frames[0], 0.0)
    run_steps(emu, frames, F, bench.DT, 1, 1, None, None, dev)
    eng = emu._engine
    kind, fpl, fpb = eng.last_pipeline()
    assert kind == "k_chain", kind  # records from k_ahead: the small-grid path the benchmark times
    assert fpl == 32, "frames per chain launch %d: the co-residency check failed and the chain lost its rendezvous" % fpl
    # the schedule those launches follow: every launch after the first validates the one before it (a redo pass and its
    # rendezvous can happen there), with a refractory period and k_ahead's records
    n = eng.lib.v2e_emu_chain_plan(F, fpl, fpb, 3, 1, 0, None, 0)
    assert n > 0
    plan = np.zeros((n, 8), dtype=np.int32)
    assert eng.lib.v2e_emu_chain_plan(F, fpl, fpb, 3, 1, 0, plan.ctypes.data, n) == n
    nf, pnf = plan[:, 1], plan[:, 3]
    assert nf.max() == 32 and (pnf[1:] > 0).all() and pnf[0] == 0
    del emu, eng
