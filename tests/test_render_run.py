"""CPU-only: the host side of EventRenderer.render_run -- v2e.py's packet rule (`run_packets`), the reference's frame-times
listing (`frame_times_text`) and the C ABI of the run kernels -- against tests/golden/render_run.npz, which
tests/golden/make_golden_render_run.py recorded from the reference's own EventRenderer driven by v2e.py's loop."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_run.npz")
VIDEO = "dvs-video.avi"
RUN_SYMBOLS = ["v2e_render_run", "v2e_render_run_area_segments", "v2e_render_run_frame_times", "v2e_render_run_windows"]


def cases(z=None):
    z = np.load(GOLDEN) if z is None else z
    return sorted(k[:-len("_packets")] for k in z.keys() if k.endswith("_packets"))


def batch_of(case):
    return int(re.search(r"_b(\d+)_", case).group(1))


def test_fixture_holds_every_mode_two_batches_and_a_small_size():
    z = np.load(GOLDEN)
    names = cases(z)
    assert len(names) == 14
    for mode in ("duration_0p0003", "duration_0p001", "count_50", "source_none", "area_count_6"):
        assert {batch_of(c) for c in names if c.startswith(mode)} == {8, 5}
        assert any(c.endswith("_32x32") for c in names if c.startswith(mode)) == (mode != "area_count_6")
    for c in names:
        assert len(z[c + "_times"]) >= 10
    counts = z["counts"]
    assert len(counts) == 120 and int((counts == 0).sum()) == 5 and int(counts.sum()) == len(z["rows"])
    # the long exposure leaves packets without a complete frame
    c = "duration_0p001_b8_64x64"
    assert sum((c + "_p%d" % k) not in z for k in range(len(z[c + "_packets"]))) >= 1


@pytest.mark.parametrize("case", cases())
def test_run_packets_reproduce_the_loop_of_v2e(case):
    """The packets v2e.py's loop rendered (the leftover one last), from the counts alone; then the same clip split into runs at
    arbitrary frames, the pending rows carried from run to run."""
    from v2e_amd.renderer import run_packets
    z = np.load(GOLDEN)
    counts, want, bs = z["counts"], z[case + "_packets"], batch_of(case)
    n_rows = int(counts.sum())
    packets, pending_frames = run_packets(counts, 0, bs)
    assert packets.dtype == np.int64 and np.array_equal(packets, want[:-1])
    assert (int(packets[-1, 1]), n_rows) == tuple(want[-1])  # the leftover packet is what is still pending
    assert pending_frames == len(counts) - 1 - max(i for i in range(len(counts)) if counts[i] and i % bs == 0)
    for cuts in ([0, 50, 120], [0, 3, 4, 41, 97, 120], [0, 1, 2, 119, 120], [0, 9, 10, 11, 12, 13, 14, 15, 16, 17, 120]):
        got, base, pend = [], 0, 0  # base: clip row of the first row the next run sees (its pending rows included)
        for a, b in zip(cuts, cuts[1:]):
            pk, pf = run_packets(counts[a:b], a, bs, pending_rows=pend)
            assert 0 <= pf <= b - a
            got += [(base + r0, base + r1) for r0, r1 in pk]
            total = pend + int(counts[a:b].sum())
            used = int(pk[-1, 1]) if len(pk) else 0
            base, pend = base + used, total - used
        assert np.array_equal(np.array(got), want[:-1]) and (base, base + pend) == tuple(want[-1]), cuts


def test_run_packets_edge_cases():
    from v2e_amd.renderer import run_packets
    pk, pf = run_packets([], 0, 8)
    assert pk.shape == (0, 2) and pf == 0
    pk, pf = run_packets([0, 0, 0], 0, 1)  # frames without events are never appended and never flush
    assert pk.shape == (0, 2) and pf == 3
    pk, pf = run_packets([4, 0, 2, 1], 0, 2)  # frame 0 flushes, frame 2 flushes, frame 3 stays pending
    assert pk.tolist() == [[0, 4], [4, 6]] and pf == 1
    pk, pf = run_packets([4, 0, 2, 1], 1, 2, pending_rows=3)  # frames 1..4: frame 2 has no events, so only frame 4 flushes
    assert pk.tolist() == [[0, 10]] and pf == 0
    pk, pf = run_packets([4, 2, 0, 1, 5], 1, 2, pending_rows=3)  # frames 1..5: 2 and 4 flush
    assert pk.tolist() == [[0, 9], [9, 10]] and pf == 1
    with pytest.raises(ValueError):
        run_packets([1, -1], 0, 8)
    with pytest.raises(ValueError):
        run_packets([1], 0, 0)


@pytest.mark.parametrize("case", cases())
def test_frame_times_text_is_the_reference_file(case, tmp_path):
    from v2e_amd.renderer import frame_times_text, write_frame_times
    z = np.load(GOLDEN)
    times, want = z[case + "_times"], z[case + "_txt"].tobytes()
    assert want.startswith(b"# frame times for dvs-video.avi\n# frame# time(s)\n")
    assert frame_times_text(VIDEO, times).encode() == want
    # in pieces, as a streamed clip delivers them
    k = len(times) // 3
    text = frame_times_text(VIDEO, times[:k]) + frame_times_text(VIDEO, times[k:], first_frame=k, header=False)
    assert text.encode() == want
    write_frame_times(str(tmp_path / "t.txt"), VIDEO, times)
    assert open(str(tmp_path / "t.txt"), "rb").read() == want


def test_header_declares_the_run_entry_points():
    from v2e_amd import _capi
    src = open(os.path.join(ROOT, "include", "v2e_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in RUN_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _capi.SIGNATURES
        # every entry of the header cites the reference lines it restates
        comment = src[:src.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert re.search(r"renderer\.py:\d+", comment), name
    lib = _capi.lib()
    for name in RUN_SYMBOLS:
        assert hasattr(lib, name)


def test_renderer_surface_of_whole_runs():
    import inspect
    import v2e_amd
    from v2e_amd.renderer import EventRenderer
    sig = inspect.signature(EventRenderer.render_run)
    assert list(sig.parameters)[1:] == ["rows", "counts", "height", "width", "frame0", "batch_size", "return_frames", "as_u8"]
    assert (sig.parameters["frame0"].default, sig.parameters["batch_size"].default) == (0, 8)
    assert (sig.parameters["return_frames"].default, sig.parameters["as_u8"].default) == (True, False)
    assert hasattr(EventRenderer, "flush_run")
    assert v2e_amd.run_packets is not None and v2e_amd.frame_times_text is not None
    from v2e_amd.pipeline import VideoToEvents
    assert "renderer" in inspect.signature(VideoToEvents.run).parameters
    p = inspect.signature(VideoToEvents.run_stream).parameters
    assert "renderer" in p and "on_dvs_frames" in p
