"""CPU-only: the numpy statement of MLPFilter's definition (tests/mlp_filter_ref.py) against a float64 torch evaluation of the same
network and against single features, and the host side of v2e_amd/mlpf.py: argument checks (all raised before the library or a
device is touched), from_module, logit, the launch-shape constants and the ctypes table."""
import math
import os
import re

import numpy as np
import pytest
import torch

from denoise_ref import border_rows
from mlp_filter_ref import NAN_BITS, bits, mlp_filter_serial, mlp_scores, mlp_scores_parts, random_network
from patches_ref import patches_serial

H5, W7 = 5, 7
TAU = 2.0 ** -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sequential(w1, b1, w2, b2, sigmoid=False, dtype=torch.float32):
    nn = torch.nn
    hidden, K = w1.shape
    layers = [nn.Linear(K, hidden), nn.ReLU(), nn.Linear(hidden, 1)] + ([nn.Sigmoid()] if sigmoid else [])
    net = nn.Sequential(*layers)
    with torch.no_grad():
        net[0].weight.copy_(torch.from_numpy(w1))
        net[0].bias.copy_(torch.from_numpy(b1))
        net[2].weight.copy_(torch.from_numpy(w2).reshape(1, hidden))
        net[2].bias.copy_(torch.from_numpy(b2).reshape(1))
    return net.to(dtype)


@pytest.mark.parametrize("r,hidden", [(1, 1), (2, 20), (3, 20), (3, 64)])
def test_reference_against_float64_torch(r, hidden):
    """The same nn.Sequential in torch.float64 on the same features.  The bound is derived from the definition.  Layer 1: K
    float64 additions of exact products onto the bias, each with a relative error of at most 2^-53 on a partial sum that is at
    most the sum of the absolute terms: (K + 1) * 2^-53 * (|b1_j| + sum_k |w1_jk x_k|) on a_j, which ReLU (1-Lipschitz) passes on
    at most unchanged; rounding h_j to float32 adds 2^-24 |h_j|; both reach the score times |w2_j|.  Layer 2:
    (hidden + 1) * 2^-53 * (|b2| + sum_j |w2_j h_j|).  The reference's sum is compared before its own rounding to float32."""
    rows, _ = border_rows(H5, W7, 1500)
    feat, valid, _, _ = patches_serial(rows, H5, W7, r, "linear", TAU)
    K = feat[0].size
    w1, b1, w2, b2 = random_network(K, hidden, seed=10 * r + hidden)
    score, s, h = mlp_scores_parts(feat, valid, w1, b1, w2, b2)
    x = feat.reshape(len(feat), K).astype(np.float64)
    with torch.no_grad():
        want = sequential(w1, b1, w2, b2, dtype=torch.float64)(torch.from_numpy(x)).numpy().reshape(-1)
    u = 2.0 ** -53
    terms1 = np.abs(b1.astype(np.float64))[None, :] + np.abs(x) @ np.abs(w1.astype(np.float64)).T         # [n, hidden]
    aw2 = np.abs(w2.astype(np.float64)).reshape(-1)
    h64 = h.astype(np.float64)
    bound = ((K + 1) * u * terms1 + 2.0 ** -24 * np.abs(h64)) @ aw2 + (hidden + 1) * u * (abs(float(b2[0])) + np.abs(h64) @ aw2)
    err = np.abs(s - want)
    assert valid.sum() > 1400 and (err[valid] <= bound[valid]).all(), (err[valid] / bound[valid]).max()
    assert (bound[valid] < 1e-4 * (1 + np.abs(want[valid]))).all()          # and the bound itself says something
    assert np.array_equal(bits(score[valid]), bits(s[valid].astype(np.float32)))
    assert (bits(score[~valid]) == NAN_BITS).all() and (~valid).sum() > 20


@pytest.mark.parametrize("r", [1, 2, 3])
def test_reference_with_one_hot_networks_returns_single_features(r):
    rows, _ = border_rows(H5, W7, 1500)
    feat, valid, _, _ = patches_serial(rows, H5, W7, r, "linear", TAU)
    K = feat[0].size
    x = feat.reshape(len(feat), K)
    zero, one = np.zeros(1, np.float32), np.ones((1, 1), np.float32)
    seen_fraction = False
    for k in range(K):
        w1 = np.zeros((1, K), np.float32)
        w1[0, k] = 1
        got = mlp_scores(feat, valid, w1, zero, one, zero)
        want = np.where(x[:, k] > 0, x[:, k], np.float32(0))
        assert np.array_equal(bits(got[valid]), bits(want[valid]))
        seen_fraction |= bool(((want[valid] > 0) & (want[valid] < 1)).any())
    assert seen_fraction


def test_reference_mask_and_maps():
    rows, _ = border_rows(H5, W7, 1500)
    net = random_network(98, 20, seed=3)
    scores, valid, mask, last_t, last_p = mlp_filter_serial(rows, H5, W7, 3, TAU, *net, keep=0.25)
    feat, pvalid, pt, pp = patches_serial(rows, H5, W7, 3, "linear", TAU)
    assert np.array_equal(valid, pvalid) and np.array_equal(last_t, pt) and np.array_equal(last_p, pp)
    assert np.array_equal(mask, valid & (np.nan_to_num(scores.astype(np.float64), nan=-np.inf) >= 0.25)) and 0 < mask.sum() < valid.sum()
    assert not mask[~valid].any() and np.isnan(scores[~valid]).all()
    # cutting the rows changes nothing
    a = mlp_filter_serial(rows[:700], H5, W7, 3, TAU, *net, keep=0.25)
    b = mlp_filter_serial(rows[700:], H5, W7, 3, TAU, *net, keep=0.25, last_t=a[3], last_p=a[4])
    assert np.array_equal(bits(np.concatenate([a[0], b[0]])), bits(scores)) and np.array_equal(np.concatenate([a[2], b[2]]), mask)
    assert np.array_equal(b[3], last_t) and np.array_equal(b[4], last_p)


@pytest.fixture
def untouched(monkeypatch):
    from v2e_amd import MLPFilter, _capi

    def touched(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)
    monkeypatch.setattr(MLPFilter, "_dev", touched)
    return MLPFilter


def test_constructor_checks(untouched):
    MLPFilter = untouched
    w1, b1, w2, b2 = random_network(98, 20, seed=1)
    good = dict(height=4, width=6, w1=w1, b1=b1, w2=w2, b2=b2)
    flt = MLPFilter(**good)
    assert (flt.height, flt.width, flt.radius, flt.size, flt.n_inputs, flt.hidden, flt.tau, flt.passes) == (4, 6, 3, 7, 98, 20, 0.1, 0)
    assert flt.max_rows_per_pass == 1 << 25 and flt.thresholds is None
    # accepted layouts: w2 [hidden] or [1, hidden], b2 [1], 0-dim or a number that is a float32 value; tensors as well as arrays
    for kw in (dict(w2=w2.reshape(20)), dict(b2=b2.reshape(())), dict(b2=np.float32(0.5)), dict(b2=0.5), dict(b2=0),
               dict(w1=torch.from_numpy(w1), b1=torch.from_numpy(b1), w2=torch.from_numpy(w2), b2=torch.from_numpy(b2))):
        MLPFilter(**dict(good, **kw))
    for radius, K in ((1, 18), (2, 50)):
        n = random_network(K, 64, seed=2)
        assert MLPFilter(4, 6, *n, radius=radius).hidden == 64
    inf_w1, nan_b2 = w1.copy(), b2.copy()
    inf_w1[3, 5], nan_b2[0] = np.inf, np.nan
    bad = [dict(w1=w1.astype(np.float64)), dict(b1=b1.astype(np.float16)), dict(w2=w2.astype(np.float64)), dict(b2=b2.astype(np.float64)),
           dict(w1=torch.from_numpy(w1).double()), dict(w1=torch.from_numpy(w1).to(torch.bfloat16)), dict(w1=w1.tolist()), dict(b2=0.1),
           dict(b2=None), dict(b2=True),
           dict(w1=w1[:, :97]), dict(w1=w1.reshape(-1)), dict(radius=2), dict(radius=1), dict(b1=b1[:19]), dict(w2=w2[:, :19]),
           dict(w2=w2.reshape(20, 1)), dict(b2=np.zeros(2, np.float32)),
           dict(w1=inf_w1), dict(b2=nan_b2), dict(b1=np.full(20, -np.inf, np.float32)),
           dict(w1=np.zeros((0, 98), np.float32), b1=np.zeros(0, np.float32), w2=np.zeros((1, 0), np.float32)),
           dict(w1=np.zeros((65, 98), np.float32), b1=np.zeros(65, np.float32), w2=np.zeros((1, 65), np.float32)),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(tau="x"),
           dict(radius=0), dict(radius=4), dict(radius=1.5), dict(height=0), dict(width=0), dict(max_rows_per_pass=0),
           dict(max_rows_per_pass=(1 << 30) + 1),
           dict(thresholds=[]), dict(thresholds=[0.5, 0.5]), dict(thresholds=[1.0, 0.5]), dict(thresholds=[0.0, np.nan]),
           dict(thresholds=[0.0, np.inf])]
    for kw in bad:
        with pytest.raises(ValueError):
            MLPFilter(**dict(good, **kw))
    for radius, K in ((1, 18), (2, 50), (3, 98)):                  # a shape that does not match the radius: the message names K
        with pytest.raises(ValueError, match="= %d inputs at radius %d" % (K, radius)):
            MLPFilter(4, 6, np.zeros((20, K + 1), np.float32), b1, w2, b2, radius=radius)
    assert MLPFilter(**dict(good, thresholds=[-1.0, 0.0, 2.5])).thresholds.tolist() == [-1.0, 0.0, 2.5]


def test_add_run_checks(untouched):
    flt = untouched(4, 6, *random_network(98, 20, seed=1), thresholds=[0.0])
    for r in (torch.zeros((6, 4)), torch.zeros((6, 3)), torch.zeros((6, 4), dtype=torch.float64), np.zeros((6, 4), np.float32), [[0, 0, 0, 0]]):
        with pytest.raises(ValueError):  # host rows, wrong shape, wrong type
            flt.add_run(r)
    for kw in (dict(keep=float("nan")), dict(keep="x"), dict(keep=(1, 0.5)), dict(out=torch.zeros(3)), dict(n_signal=[0]),
               dict(counts=[2], n_signal=[3]), dict(counts=[2], n_signal=[1]), dict(counts=[0], n_signal=[0], labels=np.zeros(0, bool)),
               dict(labels=np.zeros(1, bool)), dict(labels=np.zeros(0, np.uint8))):
        with pytest.raises(ValueError):
            flt.add_run(None, **kw)
    with pytest.raises(ValueError):
        untouched(4, 6, *random_network(98, 20, seed=1)).result()  # no thresholds: no ROC


def test_from_module_equals_the_explicit_constructor():
    from v2e_amd import MLPFilter
    nn = torch.nn
    net = random_network(50, 20, seed=5)
    for sigmoid in (False, True):
        flt = MLPFilter.from_module(4, 6, sequential(*net, sigmoid=sigmoid), radius=2, tau=0.003, thresholds=[0.0, 1.0], max_rows_per_pass=77)
        ref = MLPFilter(4, 6, *net, radius=2, tau=0.003, thresholds=[0.0, 1.0], max_rows_per_pass=77)
        for name in ("w1", "b1", "w2", "b2"):
            a, b = getattr(flt, name), getattr(ref, name)
            assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(bits(a), bits(b))
        assert flt.w2.shape == (20,) and flt.b2.shape == (1,) and np.array_equal(flt.w1, net[0])
        assert (flt.radius, flt.tau, flt.hidden, flt.max_rows_per_pass) == (2, 0.003, 20, 77) and flt.thresholds.tolist() == [0.0, 1.0]
    lin = nn.Linear
    for module in (lin(50, 1), nn.Sequential(lin(50, 20), nn.Tanh(), lin(20, 1)), nn.Sequential(lin(50, 20), nn.ReLU()),
                   nn.Sequential(lin(50, 20), nn.ReLU(), lin(20, 2)), nn.Sequential(lin(50, 20), nn.ReLU(), lin(20, 1), nn.ReLU()),
                   nn.Sequential(lin(50, 20), nn.ReLU(), lin(20, 20), nn.ReLU(), lin(20, 1)),
                   nn.Sequential(lin(50, 20), nn.ReLU(), lin(20, 1), nn.Sigmoid(), nn.Sigmoid()),
                   nn.Sequential(lin(50, 20, bias=False), nn.ReLU(), lin(20, 1)), nn.Sequential(lin(50, 20), nn.ReLU(), lin(20, 1)).double(),
                   nn.Sequential(lin(98, 20), nn.ReLU(), lin(20, 1)), nn.Sequential(lin(50, 65), nn.ReLU(), lin(65, 1)), "net", None):
        with pytest.raises(ValueError):
            MLPFilter.from_module(4, 6, module, radius=2)


def test_logit():
    from v2e_amd import MLPFilter
    assert MLPFilter.logit(0.5) == 0.0 and MLPFilter.logit(0.75) == math.log(3.0) and MLPFilter.logit(0.25) == math.log(1.0 / 3.0)
    for p in (0.01, 0.3, 0.9, 0.999):
        assert abs(1.0 / (1.0 + math.exp(-MLPFilter.logit(p))) - p) < 1e-15
    for p in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            MLPFilter.logit(p)


def test_launch_shape_constants_and_the_ctypes_table():
    """The rows of a tile and the grid cap that tests/test_mlp_filter_gpu.py is sized for, read from the source, are those the
    module exports; and the entry point is declared, typed and exported."""
    from v2e_amd import _capi, mlpf
    src = open(os.path.join(ROOT, "v2e_amd", "csrc", "mlpf.hip")).read()
    const = {k: int(v) for k, v in re.findall(r"^constexpr int (MLP_\w+) = (\d+);", src, flags=re.M)}
    assert const == {"MLP_TILE_ROWS": 64, "MLP_MAX_BLOCKS": 2048, "MLP_MAX_HIDDEN": 64, "MLP_GROUPS": 4}
    assert (mlpf.ROWS_PER_WORKGROUP, mlpf.MAX_WORKGROUPS, mlpf.MAX_HIDDEN) == (64, 2048, 64)
    assert "const int blocks = (int)(want < MLP_MAX_BLOCKS ? want : MLP_MAX_BLOCKS);" in src
    assert "const int64_t want = (n + MLP_TILE_ROWS - 1) / MLP_TILE_ROWS;" in src
    header = open(os.path.join(ROOT, "include", "v2e_amd.h")).read()
    assert "int v2e_patches_mlp_scores(" in header and len(_capi.SIGNATURES["v2e_patches_mlp_scores"][1]) == 20
    assert hasattr(_capi.lib(), "v2e_patches_mlp_scores")
