"""The argument check the labelled row consumers share (v2e_amd/_rowpasses.check_run), through each class's add_run: the exception
class each one raises and its own name in front of the message, before the library or the device is touched."""
import numpy as np
import pytest
import torch


def _make(name):
    import v2e_amd
    cls = getattr(v2e_amd, name)
    if name == "DenoiseSweep":
        return cls(4, 6, [0.1, 0.2])
    if name in ("WindowSweep", "DoubleWindowSweep"):
        return cls(4, 6, [1, 2], [0, 1])
    if name == "EventStats":
        return cls(4, 6)
    f32 = np.float32
    return cls(4, 6, np.zeros((2, 18), f32), np.zeros(2, f32), np.zeros(2, f32), f32(0), radius=1, thresholds=[0.0])


# the class, and what its add_run raises for rows that are no device tensor
CONSUMERS = [("DenoiseSweep", TypeError), ("WindowSweep", TypeError), ("DoubleWindowSweep", TypeError), ("EventStats", ValueError),
             ("MLPFilter", ValueError)]


@pytest.mark.parametrize("name,host_error", CONSUMERS)
def test_add_run_label_argument_checks(monkeypatch, name, host_error):
    from v2e_amd import _capi

    def touched(*a, **k):
        raise AssertionError("the library or the device was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", touched)
    monkeypatch.setattr(_capi, "require_gpu", touched)
    consumer = _make(name)
    rows = torch.zeros((6, 4), dtype=torch.float32)
    lab = torch.ones(6, dtype=torch.bool)
    cases = [
        dict(labels=lab, counts=[6], n_signal=[3]),        # both label sources
        dict(n_signal=[3]),                                # n_signal without counts
        dict(counts=[3, 3], n_signal=[3]),                 # lengths
        dict(counts=[3, 3], n_signal=[3, 4]),              # more signal rows than rows
        dict(counts=[3, 2], n_signal=[1, 1]),              # counts do not cover the rows
        dict(labels=torch.ones(5, dtype=torch.bool)),      # one label per row
        dict(labels=torch.ones(6, dtype=torch.uint8)),     # bool
    ]
    for kw in cases:
        with pytest.raises(ValueError) as e:
            consumer.add_run(rows, **kw)
        assert str(e.value).startswith(name + ".add_run: "), (kw, str(e.value))
    for bad in (rows, np.zeros((6, 4), np.float32)):       # rows on the host, rows that are no tensor
        for kw in (dict(), dict(labels=lab), dict(counts=[2, 4], n_signal=[1, 1])):
            with pytest.raises(host_error) as e:
                consumer.add_run(bad, **kw)
            assert type(e.value) is host_error and str(e.value).startswith(name + ".add_run"), (kw, str(e.value))
