"""MLPFilter's definition (v2e_amd/mlpf.py) as a numpy loop, on the output of patches_ref.patches_serial in mode "linear".  No GPU.

    a_j = float64(b1[j]);  for k = 0 .. K-1 ascending:  a_j = a_j + float64(w1[j,k]) * float64(x[k])
    h_j = float32(a_j), rounded to nearest even;  h_j = h_j if h_j > 0 else 0      (a NaN becomes 0)
    s = float64(b2);  for j ascending:  s = s + float64(w2[j]) * float64(h_j);  score = float32(s)
x is the row's features flattened as [2, P, P].  The product of two float32 values is exact in float64, so every step of the loops
is one float64 rounding: numpy's multiply-then-add is the device's fma.  A bad row gets the quiet NaN 0x7fc00000."""
import numpy as np

from patches_ref import patches_serial

NAN_BITS = 0x7FC00000


def mlp_scores(features, valid, w1, b1, w2, b2):
    """features float32 [n,2,P,P] (or [n,K]), valid bool [n], the network as float32 arrays -> scores float32 [n]: the loops over k
    and j of the definition, vectorised over rows."""
    return mlp_scores_parts(features, valid, w1, b1, w2, b2)[0]


def mlp_scores_parts(features, valid, w1, b1, w2, b2):
    """(scores float32 [n], s float64 [n]: the sums before their rounding to float32, h float32 [n,hidden]); s and h are those of
    the arithmetic for every row, bad ones included."""
    for a in (features, w1, b1, w2, b2):
        assert np.asarray(a).dtype == np.float32
    x = np.asarray(features).reshape(len(features), -1).astype(np.float64)
    n, K = x.shape
    w1 = np.asarray(w1)
    hidden = w1.shape[0]
    assert w1.shape == (hidden, K) and np.asarray(b1).shape == (hidden,)
    w2 = np.asarray(w2).reshape(hidden).astype(np.float64)
    b2 = np.asarray(b2).reshape(1).astype(np.float64)
    w1 = w1.astype(np.float64)
    a = np.repeat(np.asarray(b1).astype(np.float64)[None, :], n, axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(K):
            a = a + w1[None, :, k] * x[:, k, None]
        h = a.astype(np.float32)
        h = np.where(h > 0, h, np.float32(0))
        s = np.repeat(b2, n)
        for j in range(hidden):
            s = s + w2[j] * h[:, j].astype(np.float64)
        score = s.astype(np.float32)
    out = np.full(n, NAN_BITS, dtype=np.uint32).view(np.float32)
    valid = np.asarray(valid, dtype=bool)
    out[valid] = score[valid]
    return out, s, h


def mlp_filter_serial(rows, H, W, r, tau, w1, b1, w2, b2, keep=None, last_t=None, last_p=None):
    """The whole definition: (scores float32 [n], valid bool [n], mask bool [n] or None, last_t float32 [H,W], last_p int8 [H,W])."""
    feat, valid, mt, mp = patches_serial(rows, H, W, r, "linear", tau, last_t, last_p)
    scores = mlp_scores(feat, valid, w1, b1, w2, b2)
    mask = None
    if keep is not None:
        with np.errstate(invalid="ignore"):
            mask = valid & (scores.astype(np.float64) >= np.float64(keep))
    return scores, valid, mask, mt, mp


def random_network(K, hidden, seed):
    """RandomState normals cast to float32: (w1 [hidden,K], b1 [hidden], w2 [1,hidden], b2 [1])."""
    rng = np.random.RandomState(seed)
    return (rng.randn(hidden, K).astype(np.float32), rng.randn(hidden).astype(np.float32), rng.randn(1, hidden).astype(np.float32),
            rng.randn(1).astype(np.float32))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
