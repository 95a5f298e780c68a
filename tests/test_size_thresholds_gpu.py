"""The device-side event consumers at the sizes where their kernels change launch shape -- a capped grid whose grid-stride loop
takes a second trip, a block-sum scan whose threads own more than one block, a table too large for LDS -- each at the smallest
input that crosses, against the same plain definitions as the small-input tests: DenoiseSweep and EventPatches through tiled rows
(tests/tiled_rows.py), EventTensorizer, the pack32 wire format and EventFileReader directly.  Every comparison is exact, and every
test asserts the inequality that makes it cross its threshold (the constants: tests/test_size_thresholds.py)."""
import numpy as np
import pytest
import torch

from denoise_ref import BORDER_TAUS, border_rows, stcf_serial
from event_reader_ref import decode_aedat2
from event_tensors_ref import event_tensors
from patches_ref import patches_serial
from test_dist_cpu import _rows_runs
from test_event_reader_gpu import aedat2_header, bits, mixed_records
from test_event_tensors_gpu import _assert_equal, _clip_bounds, _explicit_bounds, _make_rows, _mode, _tensorize
from test_size_thresholds import (AGES_ITEMS, FEATURES_ITEMS, LDS_BOUNDS_MAX, LINE_BLOCK, NL_BLOCK_BYTES, P32_BLOCK, READER_BLOCK,
                                  SCAN_THREADS, SCATTER_ROWS)
from tiled_rows import tile_map, tile_rows, wide_width

pytestmark = pytest.mark.gpu

H5, W7 = 5, 7
KEEP = (3, 2.0 ** -6)
M = 1024 * 1024


@pytest.fixture(scope="module")
def base():
    """The 3000 border rows and their labels (shared, never modified)."""
    return border_rows(H5, W7, 3000)


# ------------------------------------------------------------------------------------------------- k_denoise_ages: the grid cap
def test_denoise_ages_second_grid_stride_trip(base):
    """192 tiles of the border case, 576 000 rows at 5 x 1535 in one pass: more valid rows than 2048 workgroups of 256 hold."""
    from v2e_amd import DenoiseSweep
    rows, labels = base
    K = 192
    hist, n_bad, mask, last_t = stcf_serial(rows, H5, W7, BORDER_TAUS, labels, keep=KEEP)
    wide, wlab, base_index, _ = tile_rows(rows, labels, W7, K, 1)
    Ww = wide_width(W7, K, 1)
    n = len(wide)
    assert (n, Ww) == (576000, 1535) and n - K * n_bad > AGES_ITEMS
    ds = DenoiseSweep(H5, Ww, BORDER_TAUS, device="cuda")
    assert n <= ds.max_rows_per_pass
    out = ds.add_run(torch.from_numpy(wide).cuda(), labels=torch.from_numpy(wlab).cuda(), keep=KEEP)
    res = ds.result()
    assert ds.passes == 1 and (int(out["n"]), int(out["n_bad"]), res.n_bad) == (n - K * n_bad, K * n_bad, K * n_bad)
    assert np.array_equal(res.hist, K * hist)
    assert torch.equal(out["mask"], torch.from_numpy(mask).cuda()[torch.from_numpy(base_index).cuda()]) and 0 < mask.sum() < 2900
    assert np.array_equal(bits(ds.last_t.cpu().numpy()), bits(tile_map(last_t, K, 1, -np.inf)))


# --------------------------------------------------------------------------------------------- k_patches_features: the grid cap
@pytest.mark.parametrize("r,mode,tau,K,shape", [(3, "age", None, 120, (360000, 1197)), (1, "linear", 2.0 ** -6, 660, (1980000, 5279))])
def test_patches_features_second_grid_stride_trip(base, r, mode, tau, K, shape):
    """Tiles of the border case with r guard columns between them, one pass: more (row, offset) items than 65 536 workgroups of
    256 hold.  The features are compared on the device, against the base case's indexed by each row's base row."""
    from v2e_amd import EventPatches
    rows, labels = base
    feat, valid, last_t, last_p = patches_serial(rows, H5, W7, r, mode, tau)
    wide, _, base_index, _ = tile_rows(rows, labels, W7, K, r)
    Ww = wide_width(W7, K, r)
    n, P = len(wide), 2 * r + 1
    assert (n, Ww) == shape and K * int(valid.sum()) * P * P > FEATURES_ITEMS
    ep = EventPatches(H5, Ww, radius=r, mode=mode, tau=0.1 if tau is None else tau, device="cuda")
    assert n <= ep.max_rows_per_pass
    out = ep.add_run(torch.from_numpy(wide).cuda())
    index = torch.from_numpy(base_index).cuda()
    assert ep.passes == 1 and (int(out["n"]), int(out["n_bad"])) == (K * int(valid.sum()), K * int((~valid).sum()))
    assert out["features"].shape == (n, 2, P, P) and out["features"].dtype == torch.float32
    assert torch.equal(out["features"].view(torch.int32), torch.from_numpy(feat).cuda()[index].view(torch.int32))
    assert torch.equal(out["valid"], torch.from_numpy(valid).cuda()[index]) and not valid.all()
    assert np.array_equal(bits(ep.last_t.cpu().numpy()), bits(tile_map(last_t, K, r, -np.inf)))
    assert np.array_equal(ep.last_p.cpu().numpy(), tile_map(last_p, K, r, 0))


# ------------------------------------------------------------------------------------------- k_tensorize_scatter: the grid cap
def test_tensorize_scatter_second_grid_stride_trip():
    """4096 x 256 + 257 rows at 5 x 7 over 41 uniform windows whose bounds float32 holds: rows before the first and after the last
    bound and bad rows among them, so that all three per-wave counter sums run behind a second trip."""
    H, W = H5, W7
    kw, t_end = _mode("uniform_256")
    bounds = _clip_bounds(kw, 41)
    n = SCATTER_ROWS + 257
    rows = _make_rows(n, H, W, bounds, seed=31)
    rng = np.random.default_rng(32)
    bad = rng.choice(n, 4000, replace=False)                       # spread over the whole input, the last trip included
    rows[bad[0:1000], 1] = W
    rows[bad[1000:2000], 2] = -1
    rows[bad[2000:3000], 3] = 0
    rows[bad[3000:3500], 1] = 0.5
    rows[bad[3500:4000], 0] = np.nan
    rows[-3:] = ((-1.0, 0, 0, 1), (5.0, 1, 1, -1), (np.nan, 0, 0, 1))  # before, after, bad: the last rows of the second trip
    ref = event_tensors(rows, bounds, H, W, bins=5)
    assert n - 3 >= SCATTER_ROWS and ref["n_bad"] >= 4000 and ref["n_before"] > 1000 and ref["n_after"] > 1000
    tail = event_tensors(rows[SCATTER_ROWS:], bounds, H, W, bins=5)    # what the second trip alone contributes
    assert tail["count"].sum() > 200 and min(tail["n_bad"], tail["n_before"], tail["n_after"]) >= 1 and ref["count"].sum() > 0.8 * n
    tz, got, K = _tensorize(kw, H, W, [(rows, t_end)], bins=5)
    assert K == 41 and tz.scatter_launches == 1
    _assert_equal(got, ref)
    assert tz.counters() == {"n_bad": ref["n_bad"], "n_before": ref["n_before"], "n_after": ref["n_after"]}


# ----------------------------------------------------------------------------------- k_tensorize_scatter: bounds in LDS or not
@pytest.mark.parametrize("n_bounds", [LDS_BOUNDS_MAX, LDS_BOUNDS_MAX + 1])
def test_tensorize_explicit_bounds_at_the_lds_limit(n_bounds):
    """An explicit table of 4096 entries (the last one staged in LDS) and one of 4097 (the first one searched in global memory),
    each taken whole by one launch."""
    H, W = H5, W7
    b = _explicit_bounds(n_bounds)
    assert len(b) == n_bounds and b[0] == -0.25 and b[-1] == 0.75 and (n_bounds > LDS_BOUNDS_MAX) == (n_bounds == 4097)
    rows = _make_rows(5000, H, W, b, seed=n_bounds)
    ref = event_tensors(rows, b, H, W, bins=5)
    tz, got, K = _tensorize(dict(bounds=b), H, W, [(rows, 0.75)], bins=5)
    assert K == n_bounds - 1 and tz.scatter_launches == 1          # one launch with nk + 1 = n_bounds table entries
    _assert_equal(got, ref)
    assert ref["n_before"] > 0 and ref["n_after"] > 0 and ref["count"].sum() > 4000
    assert (ref["count"].reshape(K, -1).sum(1) > 0).sum() > 1500   # and the rows are spread over the whole table
    assert tz.check() == {"n_bad": 0, "n_before": ref["n_before"], "n_after": ref["n_after"]}


# ------------------------------------------------------------------------------------------------------ k_rd_scan: AEDAT-2.0
def read_chunks(path, **kw):
    """(rows, labels, t_us as host arrays, counters, the number of chunks) of one pass of EventFileReader over the file"""
    from v2e_amd import EventFileReader
    rd = EventFileReader(path, device="cuda:0", **kw)
    rows, labels, t_us, sizes = [], [], [], []
    for chunk in rd:
        rows.append(chunk["rows"].cpu().numpy())
        labels.append(chunk["labels"].cpu().numpy())
        t_us.append(None if chunk["t_us"] is None else chunk["t_us"].cpu().numpy())
        sizes.append(len(rows[-1]))
    return (np.concatenate(rows), np.concatenate(labels), None if t_us[0] is None else np.concatenate(t_us), rd.counters(), len(sizes))


def test_aedat2_scan_threads_own_two_blocks(tmp_path):
    """1024 * 1024 + 37 mixed records: one chunk of 1025 workgroups, so every scan thread owns two block counts (most of them
    beyond the end); then the same file in chunks of 8 MiB: a full scan of 1024 blocks, one per thread, and a 37-record tail."""
    n = M + 37
    payload = mixed_records(n)
    path = str(tmp_path / "large.aedat")
    with open(path, "wb") as f:
        f.write(aedat2_header(tmp_path, label=True) + payload)
    r_rows, r_lab, r_t_us, r_cnt = decode_aedat2(payload, 346, 260, None, True)
    assert (n + READER_BLOCK - 1) // READER_BLOCK == SCAN_THREADS + 1 and len(r_rows) > 700000 and 0 < r_lab.sum() < len(r_lab)
    assert 8 * M // 8 == SCAN_THREADS * READER_BLOCK and 8 * n < 64 << 20  # (the second reading's first chunk; the default chunk)
    for kw, chunks in (({}, 1), ({"chunk_bytes": 8 * M}, 2)):
        rows, lab, t_us, cnt, n_chunks = read_chunks(path, width=346, height=260, labels=True, **kw)
        assert n_chunks == chunks
        assert np.array_equal(bits(rows), bits(r_rows)) and np.array_equal(lab, r_lab)
        assert t_us.dtype == np.int64 and np.array_equal(t_us, r_t_us)
        assert {k: cnt[k] for k in r_cnt} == r_cnt and cnt["n_host_parsed"] == 0
    assert r_cnt["n_aps"] > 200000 and r_cnt["n_outside"] > 10000 and r_cnt["n_nonmonotonic"] >= 10 and r_cnt["n_special"] == 0


# ----------------------------------------------------------------------------------------------------------- k_rd_scan: text
def test_text_scan_threads_own_several_blocks(tmp_path):
    """One labelled text file of 720 000 rows, above 16 MiB, with comment, empty and malformed lines sprinkled through it, read as
    a single chunk of about 20 MiB: the newline scan's threads own 2 block counts each, the line scan's 6.  The time stamps are written with
    Python's shortest round-trip formatting, as DVSTextOutput writes them, so every row reads back bit for bit."""
    n = 720000
    rng = np.random.default_rng(41)
    rows = np.empty((n, 4), np.float32)
    rows[:, 0] = (np.cumsum(rng.integers(0, 50, n)) * 1e-6).astype(np.float32)
    rows[:, 1], rows[:, 2] = rng.integers(0, 346, n), rng.integers(0, 260, n)
    rows[:, 3] = rng.integers(0, 2, n) * 2 - 1
    labels = rng.random(n) < 0.7
    t, x, y = rows[:, 0].astype(np.float64).tolist(), rows[:, 1].astype(np.int64).tolist(), rows[:, 2].astype(np.int64).tolist()
    p, s = (rows[:, 3] > 0).astype(np.int64).tolist(), labels.astype(np.int64).tolist()
    lines = ["%r %d %d %d %d\n" % v for v in zip(t, x, y, p, s)]
    extra = {"n_comment": 0, "n_bad": 0}
    for k in range(0, n, 997):                                     # lines that are no rows, in front of row k
        lines[k] = "# a comment in front of row %d\n" % k + lines[k]
        extra["n_comment"] += 1
    for k in range(0, n, 1499):
        lines[k] = ("  \t\n" if k % 2 else "\n") + lines[k]
        extra["n_comment"] += 1
    for k in range(0, n, 2003):                                    # (the third kind: four fields in a labelled file)
        lines[k] = ("0.5 this line is bad\n", "0.5 1 2 2 1\n", "0.5 1 2 1\n")[k % 3] + lines[k]
        extra["n_bad"] += 1
    data = "".join(lines).encode("ascii")
    n_lines = n + extra["n_comment"] + extra["n_bad"]
    path = str(tmp_path / "large.txt")
    with open(path, "wb") as f:
        f.write(data)
    cap_rows = len(data) // 16 + 64                                # EventFileReader's first guess for the chunk holds every line
    assert data.count(b"\n") == n_lines <= cap_rows and len(data) < 64 << 20
    # both scans over more than 1024 blocks: the newline scan's threads own 2 block counts each, the line scan's more than 4
    assert -(-len(data) // NL_BLOCK_BYTES) > SCAN_THREADS and -(-cap_rows // LINE_BLOCK) > 4 * SCAN_THREADS
    got, lab, t_us, cnt, n_chunks = read_chunks(path, labels=True)
    assert n_chunks == 1 and t_us is None
    assert np.array_equal(bits(got), bits(rows)) and np.array_equal(lab, labels)
    assert extra["n_comment"] > 1000 and extra["n_bad"] > 300
    assert {k: cnt[k] for k in ("n_rows", "n_lines", "n_comment", "n_bad", "n_flagged", "n_host_parsed")} == \
        {"n_rows": n, "n_lines": n_lines, "n_comment": extra["n_comment"], "n_bad": extra["n_bad"], "n_flagged": 0, "n_host_parsed": 0}


# --------------------------------------------------------------------------------------------------------------------- pack32
GUARD = 0x5A5A5A5A5A5A5A5A


def pack32_both(ev, cap_runs=None):
    """The rows packed on the device (into a run table with a guard word behind it) and by the CPU definition, compared:
    payload words, runs[0 .. R] and flags; and unpack_events32 on the device restores the rows bit for bit from both streams.
    Returns (flags, R, the device's run table with its guard word)."""
    from v2e_amd.dist import pack_events32, unpack_events32
    n = len(ev)
    host = torch.from_numpy(ev)
    plc, runsc, flc = pack_events32(host, cap_runs=cap_runs)
    cap = n if cap_runs is None else cap_runs
    runs = torch.full((cap + 2,), GUARD, dtype=torch.int64, device="cuda")
    payload = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pl, rn, fl = pack_events32(host.cuda(), payload=payload, runs=runs[:cap + 1], cap_runs=cap)
    flags, R = int(fl[0].item()), int(runsc.numel()) - 1
    assert flags == int(flc[0]) and R <= cap
    assert torch.equal(rn[:R + 1].cpu(), runsc)
    assert int(runs[cap + 1].item()) == GUARD and int(payload[n].item()) == 0x5A5A5A5A    # nothing behind the table or the payload
    if not flags & 1:
        assert torch.equal(pl[:n].cpu(), plc)
    if flags == 0:
        for p, r in ((pl, rn), (plc.cuda(), runsc.cuda())):
            back = unpack_events32(p, r, n)
            assert torch.equal(back.view(torch.int32).cpu(), host.view(torch.int32))
    return flags, R, runs


def stamped(n, t_bits, seed=0):
    """n rows with the given float32 time stamp bits, coordinates up to 2047 x 1023 and random polarities"""
    rng = np.random.default_rng(seed)
    ev = np.empty((n, 4), np.float32)
    ev[:, 0] = np.asarray(t_bits, dtype=np.uint32).view(np.float32)
    ev[:, 1], ev[:, 2] = rng.integers(0, 2048, n), rng.integers(0, 1024, n)
    ev[:, 3] = rng.integers(0, 2, n) * 2 - 1
    if n >= 2:
        ev[0, 1:3], ev[n - 1, 1:3] = (2047, 1023), (0, 0)
    return ev


def stamps_from_starts(n, starts):
    """float32 bits of time stamps that change exactly at the row indices `starts` (multiples of 2^-10 from -2 * 2^-10 on)"""
    flag = np.zeros(n, np.int64)
    flag[[s for s in starts if 0 < s < n]] = 1
    return ((np.cumsum(flag) - 2) * 2.0 ** -10).astype(np.float32).view(np.uint32)


def pattern(name, n):
    if name == "short_runs":                                       # tests/test_dist_cpu._rows_runs: blocks of 2 or 3 rows
        return _rows_runs(n, 1, 2).numpy()
    if name == "every_row":                                        # R = n: every block and every wave is full of starts
        return stamped(n, np.arange(n, dtype=np.uint32) + 0x3F000000, 1)
    if name == "one_stamp":                                        # R = 1: no block but the first holds a start
        return stamped(n, np.full(n, np.float32(0.25).view(np.uint32)), 2)
    if name == "edges":                                            # runs that start at, one before and one after multiples of 64 and 1024
        return stamped(n, stamps_from_starts(n, [m + d for m in range(0, n + 64, 64) for d in (-1, 0, 1)]), 3)
    if name == "long_runs":                                        # runs of 2500 rows and more: blocks and waves without a start
        return stamped(n, stamps_from_starts(n, list(range(700, n, 2500)) + [701]), 4)
    assert name == "bits"                                          # runs split on bits: -0.0 | +0.0 | NaN | the same NaN | another NaN | ...
    special = [0x80000000, 0x00000000, 0x7FC00000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800000, 0x7F800000, 0xFF800000, 0x00000001]
    return stamped(n, np.repeat(np.resize(np.array(special, np.uint32), -(-n // 7)), 7)[:n], 5)


def n_runs(ev):
    tb = ev[:, 0].view(np.uint32)
    return 1 + int((tb[1:] != tb[:-1]).sum())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, M, M + 1, 2 * M + 5])
def test_pack32_short_runs_at_block_wave_and_scan_edges(n):
    """Sizes around a wave, a workgroup, and the scan's width: 1024 * 1024 rows are 1024 blocks, one per scan thread and every
    thread busy; one row more and every thread owns two (most of them beyond the end); 2 * 1024 * 1024 + 5 rows: three."""
    ev = pattern("short_runs", n)
    nblk = (n + P32_BLOCK - 1) // P32_BLOCK
    per = (nblk + SCAN_THREADS - 1) // SCAN_THREADS
    assert per == {M: 1, M + 1: 2, 2 * M + 5: 3}.get(n, 1) and (n != M or nblk == SCAN_THREADS)
    flags, R, _ = pack32_both(ev)
    assert flags == 0 and R == n_runs(ev) and (n < 64 or n / 3.5 < R < n / 2)


@pytest.mark.parametrize("n", [3 * 1024 + 65, M + 1])
@pytest.mark.parametrize("name", ["every_row", "one_stamp", "edges", "long_runs", "bits"])
def test_pack32_run_patterns(name, n):
    ev = pattern(name, n)
    R = n_runs(ev)
    if name == "every_row":
        assert R == n
    elif name == "one_stamp":
        assert R == 1
    elif name == "edges":
        starts = np.flatnonzero(np.diff(ev[:, 0].view(np.uint32))) + 1
        assert {63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049} <= set(starts.tolist())
    elif name == "long_runs":
        starts = np.concatenate(([0], np.flatnonzero(np.diff(ev[:, 0].view(np.uint32))) + 1))
        per_block = np.bincount(starts // P32_BLOCK, minlength=-(-n // P32_BLOCK))
        assert np.diff(np.append(starts, n)).max() > 2048 and (per_block[:-1] == 0).any() and {700, 701} <= set(starts.tolist())
    else:
        tb = ev[:, 0].view(np.uint32)
        assert np.isnan(ev[:14, 0]).sum() == 0 and np.isnan(ev[14:35, 0]).all() and tb[13] == 0 and tb[6] == 0x80000000
        assert tb[20] == tb[21] == 0x7FC00000 and tb[28] == 0x7FC00001 and R < -(-n // 7)
    flags, got_R, runs = pack32_both(ev)
    assert flags == 0 and got_R == R
    if name == "bits":  # -0.0 | +0.0 | NaN | the same NaN | another NaN: split at 7, 14 and 28, not at 21
        assert (runs[1:5].cpu() & 0xFFFFFFFF).tolist() == [0, 7, 14, 28]


@pytest.mark.parametrize("n", [1025, M + 1])
def test_pack32_run_table_capacity(n):
    """cap_runs = R: no flag.  R - 1: the table keeps R - 1 runs, says so in runs[0] with flag bit 1 (bit 63 of the word), and the
    word behind the table is untouched.  0: the same with an empty table."""
    ev = pattern("short_runs", n)
    R = n_runs(ev)
    flags, got, _ = pack32_both(ev, cap_runs=R)
    assert flags == 0 and got == R
    for cap in (R - 1, 0):
        flags, got, runs = pack32_both(ev, cap_runs=cap)           # (the guard word behind the table is checked in there)
        head = int(runs[0].item()) & 0xFFFFFFFFFFFFFFFF
        assert flags == 2 and got == cap and head & 0xFFFFFFFF == cap and head >> 62 == 2


@pytest.mark.parametrize("col,size", [(1, 2048), (2, 1024)])
def test_pack32_coordinate_flag(col, size):
    """The flag's definition (include/v2e_amd.h): x is not an integer value in [0, 2048), or y is not one in [0, 1024) -- too
    large, negative, fractional, NaN or infinite; one row of 3000 at a time, on the device as in the CPU definition."""
    good = pattern("short_runs", 3000)
    for v in (float(size - 1), 0.0):
        ev = good.copy()
        ev[2077, col] = v
        assert pack32_both(ev)[0] == 0
    ev = good.copy()
    ev[2077, col] = -0.0                                           # the integer 0; restored as +0.0, so the round trip is not by bits
    from v2e_amd.dist import pack_events32, unpack_events32
    pl, runs, fl = pack_events32(torch.from_numpy(ev).cuda())
    assert int(fl[0].item()) == 0 and torch.equal(unpack_events32(pl, runs, 3000).cpu(), torch.from_numpy(ev))
    for v in (float(size), -1.0, -0.5, 0.5, size - 0.5, 1e9, -1e9, 3e38, np.inf, -np.inf, np.nan):
        ev = good.copy()
        ev[2077, col] = v
        flags, R, runs = pack32_both(ev)
        head = int(runs[0].item()) & 0xFFFFFFFFFFFFFFFF
        assert flags == 1 and head >> 62 == 1 and head & 0xFFFFFFFF == R == n_runs(ev), v
