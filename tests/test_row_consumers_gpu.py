"""The two label sources of the labelled row consumers on the MI355X: one bool per row in a single pass, and the frame table
(counts, n_signal) in ragged passes that start at row0 > 0, must give bit-identical results in every class."""
import numpy as np
import pytest
import torch

from denoise_ref import BORDER_TAUS, border_rows

pytestmark = pytest.mark.gpu

H5, W7, N, FRAMES, PASS_ROWS = 5, 7, 3000, 40, 257


@pytest.fixture(scope="module")
def framed_rows():
    """border_rows (bad rows included) cut into FRAMES frames of random length, each with a random number of signal rows."""
    rows, _ = border_rows(H5, W7, N)
    rng = np.random.RandomState(23)
    cuts = np.sort(rng.randint(0, N + 1, size=FRAMES - 1))
    counts = np.diff(np.concatenate([[0], cuts, [N]]))
    n_signal = np.array([rng.randint(0, c + 1) for c in counts])
    assert counts.sum() == N and counts.min() >= 0 and 0 < n_signal.sum() < N
    return rows, counts, n_signal


def _make(name, **kw):
    import v2e_amd
    cls = getattr(v2e_amd, name)
    if name == "DenoiseSweep":
        return cls(H5, W7, BORDER_TAUS, **kw)
    if name == "WindowSweep":
        return cls(H5, W7, [1, 3, 16, 200], [0, 1, 3], **kw)
    if name == "DoubleWindowSweep":
        return cls(H5, W7, [1, 5, 70], [0, 2], supports=(1, 3), **kw)
    return cls(H5, W7, isi_edges=[0.0, 2.0 ** -10, 2.0 ** -6, 1.0], time_bounds=np.linspace(0.0, 4.5, 10), **kw)


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b


@pytest.mark.parametrize("name", ["DenoiseSweep", "WindowSweep", "DoubleWindowSweep", "EventStats"])
def test_row_labels_and_frame_table_in_ragged_passes_agree(framed_rows, name):
    from v2e_amd.patches import frame_labels
    rows, counts, n_signal = framed_rows
    dev_rows = torch.from_numpy(rows).cuda()
    by_row = _make(name)
    out_a = by_row.add_run(dev_rows, labels=frame_labels(counts, n_signal))
    by_frame = _make(name, max_rows_per_pass=PASS_ROWS)
    out_b = by_frame.add_run(dev_rows, counts, n_signal=n_signal)
    assert by_row.passes == 1 and by_frame.passes == (N + PASS_ROWS - 1) // PASS_ROWS and N % PASS_ROWS != 0
    assert int(out_a["n"]) == int(out_b["n"]) and int(out_a["n_bad"]) == int(out_b["n_bad"])
    assert int(out_a["n_bad"]) > 0 and int(out_a["n"]) + int(out_a["n_bad"]) == N
    res_a, res_b = vars(by_row.result()), vars(by_frame.result())
    assert res_a.keys() == res_b.keys()
    for key in res_a:
        assert _same(res_a[key], res_b[key]), key
    assert res_a["n_bad"] == int(out_a["n_bad"])
    if name != "EventStats":   # both labels occur among the valid rows (EventStats: its count is indexed by the label)
        assert res_a["n_signal"] > 0 and res_a["n_noise"] > 0 and res_a["n_signal"] + res_a["n_noise"] == int(out_a["n"])
    else:
        assert res_a["count"][0].sum() > 0 and res_a["count"][1].sum() > 0
