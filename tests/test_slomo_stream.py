"""CPU: what tests/test_slomo_stream_gpu.py leans on.  The fixture tests/golden/slomo_stream_edges.npz (the reference's backWarp,
blend and fusion at edge shapes; tests/golden/make_golden_slomo_stream.py) holds every class of sampling position it was planted
with, the oracle reproduces it within the suite's bound, and the oracle's avg_pool2d / bilinear x2 agree with the torch operators
the reference calls at every shape the GPU file uses."""
import os

import numpy as np
import pytest

import slomo_stream_cases as sc
from fixtures import GOLDEN


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(GOLDEN, sc.EDGE_FIXTURE))


@pytest.mark.parametrize("case", sc.EDGE_CASES, ids=sc.case_name)
def test_fixture_holds_every_class_of_sampling_position(edges, case):
    """Recomputed in float64 from the fixture's own flows (prep) and from its interpolation override and x12 channels (fuse):
    per warp direction, at least 8 positions exactly on an interior integer, on -1, on the last and on the first outside column
    and row, half a pixel across each border, in each corner with one neighbour inside, and 3e4 px outside (at least 4 on
    either side)."""
    d = sc.load_case(edges, case)
    h, w, b, n_t = case
    assert 0.5 in d["ts"] and len(d["ts"]) == n_t
    assert d["flow"].shape == (b, 4, h, w) and d["intrp"].shape == (n_t, b, 5, h, w)
    assert d["x12_tail"].shape == (n_t, b, 6, h, w) and d["Ft"].shape == (n_t, b, 1, h, w)
    assert np.isfinite(d["x12_tail"]).all() and np.isfinite(d["Ft"]).all()
    for what, pos in (("prep", sc.prep_positions(d, case)), ("fuse", sc.fuse_positions(d, case))):
        cen = sc.census(pos, case)
        assert set(cen) == {0, 1} and all(set(c) == set(sc.CLASSES) for c in cen.values())
        assert not sc.census_short(cen), (what, sc.census_short(cen))
    logits = d["intrp"][:, :, 4].reshape(n_t * b, -1)
    for v in sc.LOGITS:   # every sample carries every saturating visibility logit
        assert (logits == np.float32(v)).any(axis=1).all(), v
    if b * h * w >= 512:  # where the planted pixels leave room, the other flows fill +-(max(h, w) + 3) px
        R = max(h, w) + 3
        inner = np.abs(d["flow"]) <= R
        assert inner.mean() > 0.3 and np.abs(d["flow"][inner]).max() > 0.9 * R


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, sc.EDGE_FIXTURE)) < 500 * 1000


@pytest.mark.parametrize("case", sc.EDGE_CASES, ids=sc.case_name)
def test_oracle_prep_and_fuse_equal_the_fixture(edges, case, oracle_lib):
    """oracle.slomo_prep / slomo_fuse against the reference's numbers within TOL: on these inputs the reference's own arithmetic
    (x / W in float32, torch's grid_sample, torch.sigmoid) stays inside the bound the GPU kernels are held to."""
    d = sc.load_case(edges, case)
    h, w, b, n_t = case
    x12 = oracle_lib.slomo_prep(d["I0"], d["I1"], d["flow"], d["ts"]).reshape(n_t, b, 12, h, w)
    e_prep = sc.relerr(x12[:, :, 6:12], d["x12_tail"])
    Ft = oracle_lib.slomo_fuse(d["I0"], d["I1"], x12.reshape(n_t * b, 12, h, w), d["intrp"].reshape(n_t * b, 5, h, w), d["ts"])
    e_fuse = sc.relerr(Ft, d["Ft"])
    print("%s: prep %.2e fuse %.2e" % (sc.case_name(case), e_prep, e_fuse))
    assert e_prep <= sc.TOL and e_fuse <= sc.TOL
    # channels 6-9 are the float32 blend itself: the same two products and one sum in the reference
    assert np.array_equal(sc.bits(x12[:, :, 6:10]), sc.bits(d["x12_tail"][:, :, 0:4]))


@pytest.mark.parametrize("shape", sc.POOL_SHAPES, ids=str)
def test_oracle_avgpool2_equals_torch(shape, oracle_lib):
    import torch
    x = sc.pool_input(shape)
    ref = torch.nn.functional.avg_pool2d(torch.from_numpy(x), 2).numpy()
    assert ref.shape == (1,) + tuple(shape)
    assert sc.relerr(oracle_lib.avgpool2(x), ref) <= sc.TOL


@pytest.mark.parametrize("shape", sc.UP_SHAPES, ids=str)
def test_oracle_upsample2_equals_torch(shape, oracle_lib):
    import torch
    x = sc.up_input(shape)
    ref = torch.nn.functional.interpolate(torch.from_numpy(x), scale_factor=2, mode="bilinear", align_corners=False).numpy()
    assert ref.shape == (1,) + tuple(shape)
    assert sc.relerr(oracle_lib.upsample2(x), ref) <= sc.TOL


def test_reference_values_of_the_reductions():
    """the numpy references of the GPU file on inputs whose answer is known by hand"""
    f = np.zeros((2, 4, 1, 3), np.float32)
    assert sc.speed2_ref(f) == 0
    f[1, 2, 0, 1], f[1, 3, 0, 1] = 3.0, -4.0
    assert sc.speed2_ref(f) == int(np.float32(25.0).view(np.uint32))
    f[0, 0, 0, 0] = 1e20
    assert sc.speed2_ref(f) == 0x7F800000
    f[0, 1, 0, 2] = np.nan
    assert sc.speed2_ref(f) == 0xFFFFFFFF
    assert sc.amax_positions(7) == [0, 3, 4, 5, 6] and sc.amax_positions(3) == [0, 1, 2] and sc.amax_positions(8) == [0, 7]
    big = sc.amax_positions(sc.AMAX_SIZES[-1])
    assert max(big) == sc.AMAX_SIZES[-1] - 1 and any(4194304 <= p < sc.AMAX_SIZES[-1] - 3 for p in big)
    assert sc.AMAX_SIZES[-1] // 4 > 4096 * 256 and sc.AMAX_SIZES[-1] % 4 == 2
    b, h, w = sc.SPEED_SHAPES[-1]
    assert b * h * w == 540672 and b * h * w > 2048 * 256
