"""GPU: v2e_amd.readers (v2e_amd/csrc/readers.hip) against the reference writer's recorded bytes (tests/golden/sinks.npz), the
numpy / Python reference decoders (tests/event_reader_ref.py), the parser's host entry point, and this project's own sinks;
every comparison is exact."""
import os

import numpy as np
import pytest

from event_reader_ref import LAYOUT, aedat2_header_end, decode_aedat2, decode_text
from fixtures import GOLDEN
from test_event_reader_cpu import boundary_stamps, host_parse, python_bits, sink_stamp_values, stamp_lines

pytestmark = pytest.mark.gpu

PRIME_CHUNK = 10007


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def read_all(path, **kw):
    """(rows, labels, t_us as host arrays, counters) of one pass of EventFileReader over the file"""
    import torch
    from v2e_amd import EventFileReader
    rd = EventFileReader(path, device="cuda:0", **kw)
    rows, labels, t_us = [], [], []
    for chunk in rd:
        assert chunk["rows"].is_cuda and chunk["rows"].dtype == torch.float32 and chunk["rows"].shape[1] == 4
        assert chunk["labels"] is None or (chunk["labels"].dtype == torch.bool and len(chunk["labels"]) == len(chunk["rows"]))
        rows.append(chunk["rows"].cpu().numpy())
        labels.append(None if chunk["labels"] is None else chunk["labels"].cpu().numpy())
        t_us.append(None if chunk["t_us"] is None else chunk["t_us"].cpu().numpy())
    def cat(parts, empty):
        if not parts:
            return empty
        return None if parts[0] is None else np.concatenate(parts)
    return (cat(rows, np.zeros((0, 4), np.float32)), cat(labels, np.zeros(0, bool) if rd.labels else None),
            cat(t_us, np.zeros(0, np.int64) if rd.format == "aedat2" else None), rd.counters())


def aedat2_header(tmp_path, crlf=True, label=False):
    """The header DeviceAEDat2Output writes (CRLF line ends), or the same with bare '\\n'"""
    from v2e_amd.sinks import DeviceAEDat2Output
    p = str(tmp_path / "header_only.aedat")
    DeviceAEDat2Output(p, label_signal_noise=label).close()
    head = open(p, "rb").read()
    assert head.startswith(b"#!AER-DAT2.0\r\n") and head.endswith(b"\r\n") and head.count(b"\r\n") >= 6
    return head if crlf else head.replace(b"\r\n", b"\n")


def assert_aedat2_equals_reference(path, payload, width, height, labels, **kw):
    rows, lab, t_us, cnt = read_all(path, width=width, height=height, labels=labels, **kw)
    r_rows, r_lab, r_t_us, r_cnt = decode_aedat2(payload, width, height, kw.get("layout"), labels)
    assert np.array_equal(bits(rows), bits(r_rows)) and np.array_equal(t_us, r_t_us) and t_us.dtype == np.int64
    assert (lab is None and r_lab is None) or np.array_equal(lab, r_lab)
    assert {k: cnt[k] for k in r_cnt} == r_cnt and cnt["n_host_parsed"] == 0
    return rows, lab, t_us, cnt


# ------------------------------------------------------------------------------------------------- AEDAT-2.0: the reference writer
@pytest.mark.parametrize("crlf", [True, False])
@pytest.mark.parametrize("size", [(346, 260), (640, 480)])
def test_aedat2_records_of_the_reference_writer(tmp_path, size, crlf):
    w, h = size
    z = np.load(os.path.join(GOLDEN, "sinks.npz"))
    ev, payload = z["ev_%dx%d" % (w, h)], z["aedat2_%dx%d" % (w, h)].tobytes()
    assert len(payload) == 8 * 5000 and payload[0:1] != b"#"
    path = str(tmp_path / "golden.aedat")
    with open(path, "wb") as f:
        f.write(aedat2_header(tmp_path, crlf) + payload)
    # the recording was made with label_signal_noise: its rows from 4000 on carry the special-event bit (tests/test_sinks.py).  At
    # 346x260 that bit is free and reads back as the label.  At 640x480 the writer's layout keeps x in bits 1 .. 10, so the bit
    # overwrote the top bit of those rows' flipped x: nothing there is a label, and the x the file holds is 639 - ((639 - x) | 512)
    free = (w, h) == (346, 260)
    rows, labels, t_us, cnt = read_all(path, width=w, height=h, labels=free)
    want = ev[:, 1:4].copy()
    if free:
        assert np.array_equal(labels, np.arange(5000) < 4000)
    else:
        want[4000:, 0] = 639 - ((639 - ev[4000:, 1].astype(np.int64)) | 512)
        assert labels is None and cnt["n_outside"] == int((want[:, 0] < 0).sum()) > 100
        with pytest.raises(ValueError, match="special-event bit"):
            read_all(path, width=w, height=h, labels=True)
    assert np.array_equal(rows[:, 1:4], want) and np.array_equal(rows[:4000, 1:4], ev[:4000, 1:4])
    ts = np.frombuffer(payload, ">i4")[1::2]
    assert np.array_equal(t_us, ts.astype(np.int64))
    assert np.array_equal(bits(rows[:, 0]), bits((ts.astype(np.float64) * 1e-6).astype(np.float32)))
    assert cnt["n_rows"] == 5000 and cnt["n_aps"] == cnt["n_special"] == cnt["n_trailing_bytes"] == 0 and (cnt["n_outside"] == 0) == free
    assert cnt["n_nonmonotonic"] == int((ts[1:] < ts[:-1]).sum())
    from v2e_amd import read_events
    dev_rows, dev_labels = read_events(path, width=w, height=h)  # a jAER reader's view: the special events (if any) are dropped
    assert dev_labels is None and dev_rows.is_cuda and np.array_equal(bits(dev_rows.cpu().numpy()), bits(rows[:4000 if free else 5000]))


# ------------------------------------------------------------------------------------------------- AEDAT-2.0: dropping keeps order
def mixed_records(n, seed=11):
    """n big-endian records at 346x260: a seeded quarter APS / IMU (bit 31), a seeded tenth special (bit 10), a few coordinates
    outside the sensor, a few time stamps that go backwards; the first byte is never '#'"""
    from v2e_amd.readers import READER_BLOCK as B
    rng = np.random.default_rng(seed)
    xs, ys, ps, _, _ = LAYOUT[(346, 260)]
    x, y, p = rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n)
    fx, fy = 345 - x, 259 - y              # the address fields (both axes are flipped)
    fx[rng.random(n) < 0.01] = 400         # outside the sensor: the fields hold up to 511
    fy[rng.random(n) < 0.01] = 300
    addr = (fx << xs) | (fy << ys) | (p << ps)
    addr |= (rng.random(n) < 0.25).astype(np.int64) << 31
    addr |= (rng.random(n) < 0.10).astype(np.int64) << 10
    if n > B + 192:
        addr[B + 128:B + 192] |= 1 << 31  # one whole wave of the second workgroup is dropped, its neighbours are not
        addr[[B + 127, B + 192]] &= ~((1 << 31) | (1 << 10))
    ts = np.cumsum(rng.integers(0, 50, n)) + 17_000_000  # past 16 s: float32 no longer resolves 1 us
    back = rng.choice(n, min(n // 2, 20), replace=False)
    ts[back] -= 1000
    for k in (512, 1250):  # a decreasing pair of kept records exactly on the boundary of 4096- and 10000-byte chunks
        if n > k:
            addr[k - 1:k + 1] &= ~((1 << 31) | (1 << 10))
            ts[k] = ts[k - 1] - 5
    rec = np.stack([addr, ts], axis=1).astype(np.uint32).astype(">u4")
    if n:
        assert rec.tobytes()[0:1] != b"#"
    return rec.tobytes()


@pytest.fixture(scope="module")
def mixed_file(tmp_path_factory):
    from v2e_amd.readers import READER_BLOCK as B
    tmp = tmp_path_factory.mktemp("mixed")
    payload = mixed_records(3 * B + 37)
    path = str(tmp / "mixed.aedat")
    with open(path, "wb") as f:
        f.write(aedat2_header(tmp, label=True) + payload + b"\x01\x02\x03")  # three trailing bytes
    return path, payload + b"\x01\x02\x03"


@pytest.mark.parametrize("labels", [False, True])
def test_aedat2_dropping_keeps_order_across_workgroups(mixed_file, labels):
    from v2e_amd.readers import READER_BLOCK as B
    path, payload = mixed_file
    addr = np.frombuffer(payload[:len(payload) // 8 * 8], ">u4")[0::2].astype(np.int64)
    dropped = (addr >> 31 & 1) | (0 if labels else addr >> 10 & 1)
    assert len(addr) == 3 * B + 37 and all(dropped[k:k + B].any() for k in range(0, len(addr), B))
    assert dropped[B + 128:B + 192].all() and not dropped[B + 127] and not dropped[B + 192] and B % 64 == 0
    rows, lab, t_us, cnt = assert_aedat2_equals_reference(path, payload, 346, 260, labels)
    assert cnt["n_aps"] > 700 and cnt["n_outside"] > 10 and cnt["n_nonmonotonic"] >= 10 and cnt["n_trailing_bytes"] == 3
    assert (cnt["n_special"] == 0 and 150 < (~lab).sum() < 400) if labels else cnt["n_special"] > 150
    assert len(np.unique(t_us)) > len(np.unique(rows[:, 0]))  # past 16 s float32 no longer tells every microsecond apart


@pytest.mark.parametrize("n", [0, 1, 2])
def test_aedat2_tiny_files(tmp_path, n):
    payload = mixed_records(100, seed=3)
    payload = payload[8 * 50:8 * (50 + n)]
    assert payload[0:1] != b"#"
    path = str(tmp_path / "tiny.aedat")
    with open(path, "wb") as f:
        f.write(aedat2_header(tmp_path) + payload)
    assert_aedat2_equals_reference(path, payload, 346, 260, True)
    from v2e_amd import read_events
    rows, labels = read_events(path, labels=True)
    assert tuple(rows.shape) == (n, 4) and tuple(labels.shape) == (n,) and rows.is_cuda


def test_aedat2_explicit_layout_for_another_sensor(tmp_path):
    rng = np.random.default_rng(5)
    n, (W, H), lay = 3000, (128, 96), (1, 9, 0, 0, 1)
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    addr = (x << 1) | ((H - 1 - y) << 9) | p
    payload = np.stack([addr, np.arange(n) * 3], axis=1).astype(">u4").tobytes()
    path = str(tmp_path / "other.aedat")
    with open(path, "wb") as f:
        f.write(b"#!AER-DAT2.0\n# another sensor\n" + payload)
    rows, _, _, _ = assert_aedat2_equals_reference(path, payload, W, H, False, layout=lay)
    assert np.array_equal(rows[:, 1:], np.stack([x, y, 2 * p - 1], axis=1).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ chunk independence
def test_aedat2_chunks_do_not_change_the_result(mixed_file):
    path, payload = mixed_file
    for labels in (False, True):
        whole = read_all(path, labels=labels)
        assert whole[3]["n_rows"] == len(whole[0]) > 2000
        for chunk_bytes in (4096, PRIME_CHUNK):
            part = read_all(path, labels=labels, chunk_bytes=chunk_bytes)
            assert np.array_equal(bits(part[0]), bits(whole[0])) and np.array_equal(part[2], whole[2]) and part[3] == whole[3]
            assert (part[1] is None and whole[1] is None) or np.array_equal(part[1], whole[1])
    ts = np.frombuffer(payload[:len(payload) // 8 * 8], ">i4")[1::2]
    assert ts[512] < ts[511] and ts[1250] < ts[1249]  # the pairs the boundaries of both chunk sizes fall between


@pytest.fixture(scope="module")
def sink_text_file(tmp_path_factory):
    """About 3000 lines written by DeviceTextOutput from the golden rows, a comment line and a bad line inserted mid-file"""
    import torch
    from v2e_amd.sinks import DeviceTextOutput
    tmp = tmp_path_factory.mktemp("text")
    ev = np.load(os.path.join(GOLDEN, "sinks.npz"))["ev_346x260"][:3000]
    path = str(tmp / "sink.txt")
    out = DeviceTextOutput(path)
    out.appendEvents(torch.from_numpy(ev).cuda())
    out.close()
    lines = open(path, "rb").read().split(b"\n")
    k = len(lines) // 2
    lines[k:k] = [b"# a comment in the middle", b"0.5 this line is bad"]
    data = b"\n".join(lines)
    with open(path, "wb") as f:
        f.write(data)
    return path, data, ev


def test_text_chunks_do_not_change_the_result(sink_text_file):
    path, data, ev = sink_text_file
    r_rows, _, r_cnt = decode_text(data, False)
    assert np.array_equal(bits(r_rows), bits(ev)) and r_cnt["n_bad"] == 1 and r_cnt["n_comment"] >= 7
    whole = read_all(path)
    assert np.array_equal(bits(whole[0]), bits(ev)) and whole[1] is None and whole[2] is None
    assert {k: whole[3][k] for k in r_cnt} == r_cnt and whole[3]["n_flagged"] == whole[3]["n_host_parsed"] == 0
    for chunk_bytes in (4096, PRIME_CHUNK):
        part = read_all(path, chunk_bytes=chunk_bytes)
        assert np.array_equal(bits(part[0]), bits(whole[0])) and part[3] == whole[3]


# ------------------------------------------------------------------------------------------------------ text: device equals host
def device_parse(data, want_labels=False, cap_rows=None, cap_flagged=None):
    """v2e_events_parse_text on the bytes: (rows, labels, the eight counters, flagged) as host arrays, before any patch"""
    import torch
    from v2e_amd import _capi
    from v2e_amd._capi import check, ptr, stream_ptr
    lib = _capi.lib()
    nlines = data.count(b"\n") + 1
    cap_rows = nlines if cap_rows is None else cap_rows
    cap_flagged = nlines if cap_flagged is None else cap_flagged
    dev = torch.device("cuda:0")
    dbytes = torch.from_numpy(np.frombuffer(data + b"\0", np.uint8).copy()).to(dev)
    rows = torch.full((max(cap_rows, 1), 4), 7.0, dtype=torch.float32, device=dev)
    lab = torch.full((max(cap_rows, 1),), 7, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    fl = torch.zeros((max(cap_flagged, 1), 2), dtype=torch.int64, device=dev)
    scratch = torch.empty(int(lib.v2e_events_parse_text_scratch_bytes(len(data), cap_rows)), dtype=torch.uint8, device=dev)
    check(lib.v2e_events_parse_text(ptr(dbytes), len(data), int(want_labels), ptr(rows), ptr(lab), cap_rows, ptr(cnt), ptr(fl),
                                    cap_flagged, ptr(scratch), stream_ptr(dev)), "v2e_events_parse_text")
    cnt = cnt.cpu().numpy()
    n = int(cnt[5])
    if n < 0:
        assert bool((rows == 7).all()) and bool((lab == 7).all())
        return None, None, cnt, None
    assert bool((rows[n:] == 7).all()) and bool((lab[n if want_labels else 0:] == 7).all())  # nothing written past the rows
    return rows[:n].cpu().numpy(), lab[:n].cpu().numpy().astype(bool), cnt, fl[:min(int(cnt[7]), cap_flagged)].cpu().numpy()


def cpu_test_lines():
    stamps = ['{}'.format(float(v)) for v in sink_stamp_values()]
    rng = np.random.default_rng(7)
    stamps += ['%.9f' % v for v in rng.uniform(0, 1e4, 20000)]
    stamps += [s for s, _ in boundary_stamps()]
    grammar = (b"# header\r\n\n   \n0.5\t1\t2\t1\n  0.75   3 \t 4  0  \r\n+0.5 +1 -2 1\n.5 1 2 1\n5. 1 2 1\n0.5 1 2\n0.5 1 2 1 0 7\n0.5 1 2 2\n"
               b"0.5 1e3 2 1\nnan 1 2 1\ninf 1 2 1\n- 1 2 1\n0.5 16777216 2 1\n0.5 1 2 1 1\n0.5 1 2 0 0\n0.5 1 2 1 2\n")
    # lines so long that a workgroup's 256 do not fit its LDS stage (and one that alone does not), read from HBM instead
    long_lines = b"".join(b"%d.25" % k + b" " * 90 + b"%d\t\t%d 1   \n" % (k, k + 1) for k in range(400))
    long_lines += b"#" + b"x" * 20000 + b"\n" + b"7.5 " + b" " * 17000 + b"1 2 0\n" + b"bad " * 5000 + b"\n"
    return stamp_lines(stamps) + grammar + long_lines + stamp_lines(stamps[:300]) + b"9.75 1 2 1"  # no newline at the end


@pytest.mark.parametrize("want_labels", [False, True])
def test_text_on_the_device_equals_the_host_entry_and_python(want_labels):
    data = cpu_test_lines()
    if want_labels:
        data = data.replace(b" 3 4 1\n", b" 3 4 1 0\n").replace(b" 3 4 1 0\n", b" 3 4 1\n", 500).replace(b" 3 4 1 0\n", b" 3 4 1 1\n", 9000)
    h_rows, h_lab, h_cnt, h_fl = host_parse(data, want_labels)
    d_rows, d_lab, d_cnt, d_fl = device_parse(data, want_labels)
    assert np.array_equal(bits(d_rows), bits(h_rows)) and len(h_rows) > 30000
    assert h_lab is None or (np.array_equal(d_lab, h_lab) and 8000 < h_lab.sum() < len(h_lab) - 8000)
    assert {k: int(d_cnt[v]) for k, v in {"n_rows": 0, "n_comment": 1, "n_bad": 2, "n_flagged": 3, "n_lines": 4}.items()} == h_cnt
    assert sorted(d_fl.tolist()) == sorted(h_fl.tolist()) and len(h_fl) >= 8
    r_rows, r_lab, r_cnt = decode_text(data, want_labels)
    assert {k: h_cnt[k] for k in r_cnt} == r_cnt and (r_lab is None or np.array_equal(r_lab, h_lab))
    exact = np.ones(len(h_rows), bool)
    exact[h_fl[:, 1]] = False
    assert np.array_equal(bits(d_rows)[exact], bits(r_rows)[exact])


def test_text_flagged_stamps_are_patched_with_float(tmp_path):
    data = cpu_test_lines() + b"\n1.000000059604644775390626 1 2 1\n1234567890123456789012345.5 3 4 0\n"
    path = str(tmp_path / "flagged.txt")
    with open(path, "wb") as f:
        f.write(data)
    r_rows, _, r_cnt = decode_text(data, False)
    for kw in ({}, {"chunk_bytes": 1 << 16}):
        rows, labels, t_us, cnt = read_all(path, labels=False, **kw)
        assert np.array_equal(bits(rows), bits(r_rows)) and labels is None and t_us is None  # float()'s value in every row
        assert {k: cnt[k] for k in r_cnt} == r_cnt
        assert cnt["n_host_parsed"] == cnt["n_flagged"] >= 10
    assert bits(rows[-2:, 0]).tolist() == python_bits(["1.000000059604644775390626", "1234567890123456789012345.5"]).tolist()


def test_text_more_lines_or_flagged_stamps_than_the_first_guess(tmp_path):
    """Lines of 8 bytes (the reader guesses 16 per row) and more stamps for the host than its list holds at first: both decode the
    chunk again with room, and the counters count it once."""
    short = b"0 0 0 0\n" * 3000 + b"1 2 3 1\n"
    many = b"".join(b"1.%024d 1 2 1\n" % (k + 1) for k in range(5000))
    for name, data in (("short", short), ("many", many), ("both", short + many)):
        path = str(tmp_path / (name + ".txt"))
        with open(path, "wb") as f:
            f.write(data)
        r_rows, _, r_cnt = decode_text(data, False)
        rows, _, _, cnt = read_all(path)
        assert np.array_equal(bits(rows), bits(r_rows)) and {k: cnt[k] for k in r_cnt} == r_cnt
        assert cnt["n_flagged"] == cnt["n_host_parsed"] == (0 if name == "short" else 5000)
    rows, _, cnt, _ = device_parse(short, cap_rows=3000)  # the entry point itself: nothing written, the lines it needs reported
    assert rows is None and cnt[5] == -1 and cnt[6] == 3001 and not cnt[:5].any()


def test_text_empty_file_and_comments_only(tmp_path):
    from v2e_amd import read_events
    for name, data, lines in (("empty", b"", 0), ("comments", b"# only\n#comments\n\n", 3)):
        path = str(tmp_path / (name + ".txt"))
        with open(path, "wb") as f:
            f.write(data)
        rows, labels, t_us, cnt = read_all(path)
        assert rows.shape == (0, 4) and cnt["n_rows"] == 0 and cnt["n_lines"] == cnt["n_comment"] == lines
        rows, labels = read_events(path, labels=True)
        assert tuple(rows.shape) == (0, 4) and tuple(labels.shape) == (0,)


# ------------------------------------------------------------------------------------------------------ write -> read with labels
KW = dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.03, cutoff_hz=200, leak_rate_hz=0.1, shot_noise_rate_hz=5.0,
          refractory_period_s=0.0005, output_width=346, output_height=260)  # tests/test_batch_sinks_gpu.py


@pytest.fixture(scope="module")
def labelled_run(tmp_path_factory):
    """The 13-frame clip of tests/test_batch_sinks_gpu.py through a Philox-mode emulator with label_signal_noise, one
    device-resident run written to a text and an AEDAT-2.0 file: (rows, labels, text path, aedat path)"""
    from v2e_amd import EventEmulator, frame_labels
    from v2e_amd.synth import int_gradient_frames
    tmp = tmp_path_factory.mktemp("run")
    frames, times = int_gradient_frames(13, 260, 346, seed=4, noise=10, as_array=True), [i / 300 for i in range(13)]
    emu = EventEmulator(device="cuda", seed=7, rng_mode="philox", output_folder=str(tmp), dvs_aedat2="run", dvs_text="run",
                        label_signal_noise=True, **KW)
    rows, counts = emu.generate_events_batch(frames, times)
    labels = frame_labels(counts, emu.last_n_signal).numpy()
    emu.cleanup()
    assert len(rows) == len(labels) > 1000 and 0 < labels.sum() < len(labels)
    return rows, labels, str(tmp / "run.txt"), str(tmp / "run.aedat")


def test_text_written_by_the_sink_reads_back_bit_for_bit(labelled_run):
    rows, labels, text_path, _ = labelled_run
    got, lab, t_us, cnt = read_all(text_path)  # labels=None: the first data line has five fields
    assert np.array_equal(bits(got), bits(rows)) and np.array_equal(lab, labels) and t_us is None
    assert cnt["n_rows"] == len(rows) and cnt["n_bad"] == cnt["n_flagged"] == cnt["n_host_parsed"] == 0 and cnt["n_comment"] >= 6
    got, lab, _, _ = read_all(text_path, labels=False)
    assert np.array_equal(bits(got), bits(rows)) and lab is None


def test_aedat2_written_by_the_sink_reads_back(labelled_run):
    rows, labels, _, aedat_path = labelled_run
    got, lab, t_us, cnt = read_all(aedat_path, labels=True)
    data = open(aedat_path, "rb").read()
    first = len(rows) - (len(data) - aedat2_header_end(data)) // 8  # leading records the writer dropped (a first byte '#')
    assert 0 <= first < 8 and cnt["n_rows"] == len(rows) - first and cnt["n_aps"] == cnt["n_outside"] == cnt["n_special"] == 0
    assert np.array_equal(got[:, 1:4], rows[first:, 1:4]) and np.array_equal(lab, labels[first:])
    assert np.array_equal(t_us, (np.float32(1e6) * rows[first:, 0]).astype(np.int32))  # as the writer computes it, in float32
    assert np.array_equal(bits(got[:, 0]), bits((t_us.astype(np.float64) * 1e-6).astype(np.float32)))
    got, lab, _, cnt = read_all(aedat_path, labels=False)  # a jAER reader's view: the noise is special events
    keep = labels[first:]
    assert lab is None and np.array_equal(got[:, 1:4], rows[first:][keep, 1:4]) and cnt["n_special"] == int((~keep).sum())


# ---------------------------------------------------------------------------------------------------------- one consumer end to end
def test_denoise_sweep_fed_from_the_text_reader(labelled_run):
    import torch
    from v2e_amd import DenoiseSweep, EventFileReader
    rows, labels, text_path, _ = labelled_run
    taus = np.geomspace(1e-4, 1e-1, 12)
    direct = DenoiseSweep(260, 346, taus, device="cuda:0")
    direct.add_run(torch.from_numpy(rows).cuda(), labels=torch.from_numpy(labels).cuda())
    fed = DenoiseSweep(260, 346, taus, device="cuda:0")
    n_chunks = 0
    for chunk in EventFileReader(text_path, chunk_bytes=1 << 15):
        fed.add_run(chunk["rows"], labels=chunk["labels"])
        n_chunks += 1
    a, b = direct.result(), fed.result()
    assert n_chunks > 1 and np.array_equal(a.hist, b.hist) and a.n_bad == b.n_bad == 0
    assert a.n_signal == int(labels.sum()) and a.n_noise == int((~labels).sum())
