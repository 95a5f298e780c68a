"""CPU: the text event parser (v2e_amd/csrc/text_parse.h) through its host entry point v2e_events_parse_text_host -- the same
__host__ __device__ code the GPU kernels run -- against Python's own float() / int() (tests/event_reader_ref.py), bit for bit;
and the argument checks of EventFileReader that need no device."""
import os
import re
from decimal import Decimal

import numpy as np
import pytest

from event_reader_ref import decode_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXC = {"n_rows": 0, "n_comment": 1, "n_bad": 2, "n_flagged": 3, "n_lines": 4}


def host_parse(data, want_labels=False, cap_rows=None, cap_flagged=None, counters=None):
    """(rows float32 [n,4], labels bool [n] or None, counters dict, flagged int64 [k,2]) of v2e_events_parse_text_host."""
    from v2e_amd import _capi
    lib = _capi.lib()
    buf = np.frombuffer(data, np.uint8).copy() if data else np.zeros(1, np.uint8)
    nlines = data.count(b"\n") + 1
    cap_rows = nlines if cap_rows is None else cap_rows
    cap_flagged = nlines if cap_flagged is None else cap_flagged
    rows = np.full((max(cap_rows, 1), 4), 7, np.float32)
    lab = np.full(max(cap_rows, 1), 7, np.uint8)
    cnt = np.zeros(8, np.int64) if counters is None else counters
    fl = np.zeros((max(cap_flagged, 1), 2), np.int64)
    rc = lib.v2e_events_parse_text_host(buf.ctypes.data, len(data), int(want_labels), rows.ctypes.data, lab.ctypes.data, cap_rows,
                                        cnt.ctypes.data, fl.ctypes.data, cap_flagged)
    assert rc == 0
    n = int(cnt[5])
    if n < 0:
        return None, None, cnt, None
    out = {k: int(cnt[v]) for k, v in TXC.items()}
    return rows[:n], (lab[:n].astype(bool) if want_labels else None), out, fl[:min(int(cnt[7]), cap_flagged)]


def stamp_lines(stamps):
    return "".join("%s 3 4 1\n" % s for s in stamps).encode()


def parse_stamps(stamps):
    """float32 bits of each stamp's row, the set of flagged row indices, counters"""
    rows, _, cnt, fl = host_parse(stamp_lines(stamps))
    assert cnt["n_rows"] == len(stamps) and cnt["n_bad"] == 0 and cnt["n_comment"] == 0
    assert np.array_equal(rows[:, 1:], np.tile(np.float32([3, 4, 1]), (len(stamps), 1)))
    return rows[:, 0].copy().view(np.uint32), set(fl[:, 1].tolist()), cnt


def python_bits(stamps):
    with np.errstate(over="ignore"):
        return np.array([np.float32(float(s)) for s in stamps], dtype=np.float32).view(np.uint32)


def sink_stamp_values():
    """float32 time stamps: the edge values tests/test_text_format_cpu.py formats, a sweep of the binade of 1 / 300, subnormals,
    the largest float32, and seeded random bit patterns of every exponent."""
    f32 = np.float32
    vals = [0.0, -0.0, np.float32(1e-45), np.finfo(f32).max, np.finfo(f32).tiny, np.nextafter(np.finfo(f32).tiny, f32(0)), 1.0, 0.5,
            2.0, 3.0, 10.0, 100.0, 1 / 300, 2 / 300, 0.1, 0.2, 0.3, 16777216.0, 16777217.0, 123456789.0, 1e15, 9999999583119360.0,
            1e16, 1e17, 1e18, 1e19, 1e20, 3e16, 1e-5, 1e-6, 1e4, 3.4028235e38]
    vals += [2.0 ** k for k in range(-149, 128)]
    for edge in (f32(1e-4), f32(1e16), f32(1e-5), f32(1e-3), f32(1e-6), f32(1e4)):
        vals += [np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(np.inf))]
    vals += [f32(k) / f32(300) for k in range(1, 400)] + [f32(k) for k in range(0, 2000, 7)]
    t = np.array(vals, dtype=np.float32)
    lo, hi = int(np.float32(2.0 ** -9).view(np.uint32)), int(np.float32(2.0 ** -8).view(np.uint32))
    binade = np.arange(lo, hi, 4099, dtype=np.uint32).view(np.float32)
    rng = np.random.default_rng(20261020)
    bits = rng.integers(0, 1 << 32, 6000, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7F800000) != 0x7F800000][:5000]
    sub = rng.integers(1, 1 << 23, 300, dtype=np.uint64).astype(np.uint32)  # subnormals
    in_range = rng.uniform(1e-6, 1e4, 3000).astype(np.float32)
    t = np.concatenate([t, binade, bits.view(np.float32), sub.view(np.float32), in_range])
    return np.concatenate([t, -t])


def test_every_stamp_the_text_sink_writes_parses_back_to_its_bits():
    t = sink_stamp_values()
    stamps = ['{}'.format(float(v)) for v in t]
    assert "3.4028234663852886e+38" in stamps and "0.0" in stamps and sum(s.endswith("e-05") for s in stamps) > 3
    got, flagged, cnt = parse_stamps(stamps)
    bad = np.flatnonzero(got != t.view(np.uint32))
    assert len(bad) == 0, [(stamps[i], hex(got[i]), hex(t.view(np.uint32)[i])) for i in bad[:5]]
    assert np.array_equal(got, python_bits(stamps))
    # the condition of the device parser: nothing the sink can write for stamps in {0} U [1e-6, 1e4] is left to the host
    a = np.abs(t)
    in_range = (a == 0) | ((a >= np.float32(1e-6)) & (a <= np.float32(1e4)))
    assert in_range.sum() > 4000 and not (flagged & set(np.flatnonzero(in_range).tolist()))
    assert cnt["n_flagged"] == 0 and not flagged  # and in fact nothing at all: every finite float32's repr is in the domain


def test_rpg_style_nine_decimal_stamps():
    rng = np.random.default_rng(7)
    t = np.concatenate([rng.uniform(0, 1e4, 20000), rng.uniform(0, 1, 2000), [0.0, 1e-6, 9999.999999999]])
    stamps = ['%.9f' % v for v in t]
    got, flagged, cnt = parse_stamps(stamps)
    assert np.array_equal(got, python_bits(stamps))
    assert cnt["n_flagged"] == 0 and not flagged


def boundary_stamps():
    """(stamp, must be decided on the device) -- decimals on or next to float64 / float32 rounding boundaries"""
    out = [("9007199254740993", True), ("9007199254740995", True), ("18014398509481986", True), ("18014398509481990", True),
           ("4503599627370496.5", True), ("2251799813685248.25", True), ("1125899906842624.125", True),  # float64 ties, <= 19 digits
           ("4503599627370497.5", True), ("0.1", True), ("0.3", True), ("0.30000000000000004", True), ("0.1000000000000000055", True),
           ("1e23", True), ("1E+23", True), ("9.999999999999999e22", True), ("8.41e21", True),
           ("16777217", True), ("16777219", True), ("16777217.000000001", True),  # float32 ties; the last one only after the float64 rounding
           ("16777217.00000001", True), ("1.00000005960464478", True), ("1.0000000596046448", True), ("1.000000059604644776", True),
           ("12345678901234567", True), ("1234567890123456789", True), ("0.1234567890123456789", True),
           ("1.234567890123456789e-20", True), ("123456789012345678.9e10", True),
           ("1.000000059604644775390625", False), ("1.000000059604644775390626", False),  # 25 digits: 1 + 2^-24 and just above
           ("1234567890123456789012345", False), ("0.3000000000000000166533453", False),
           ("3.4028235677973366e38", True), ("3.4028235677973367e38", True), ("3.5e38", True), ("1e39", True),  # the float32 overflow edge
           ("7.006492321624085e-46", True), ("7.006492321624086e-46", True), ("1e-46", True), ("1.5e-45", True),  # and the underflow edge
           ("1e-62", True), ("1e-63", False), ("1e62", True), ("1e63", False), ("0e999", True), ("0.000e-999", True), ("0", True),
           ("1" + "0" * 30, True), ("0." + "0" * 30 + "1", True), ("1." + "0" * 40, True)]
    # halfway cases float.hex makes easy: the exact midpoint of two neighbouring float64 (or of two float32), one digit below, one above
    for h, f32 in (("0x1.0000000000000p+0", False), ("0x1.fffffffffffffp-1", False), ("0x1.921fb54442d18p+1", False),
                   ("0x1.0000000000000p-20", False), ("0x1.5555555555555p-9", False), ("0x1.000002p+0", True), ("0x1.fffffep+6", True),
                   ("0x1.000000p-126", True), ("0x1.99999ap-4", True)):
        a = float.fromhex(h)
        assert not f32 or float(np.float32(a)) == a
        b = float(np.nextafter(np.float32(a), np.float32(np.inf))) if f32 else float(np.nextafter(a, np.inf))
        s = format((Decimal(a) + Decimal(b)) / 2, "f")
        out += [(s, False), (s[:-1] + "4999", False), (s + "0001", False)]
    return out


def test_decimals_on_rounding_boundaries_are_exact_or_flagged():
    cases = boundary_stamps()
    stamps = [s for s, _ in cases] + ["-" + s for s, _ in cases]
    decided = [d for _, d in cases] * 2
    assert any(len(s) == 25 and "." not in s for s in stamps) and any(len(s.replace(".", "")) > 40 for s in stamps)
    got, flagged, cnt = parse_stamps(stamps)
    want = python_bits(stamps)
    for i, s in enumerate(stamps):
        if decided[i]:
            assert i not in flagged, "%s should be decided by the parser" % s
        if i not in flagged:
            assert got[i] == want[i], "%s: %#x, float() gives %#x" % (s, got[i], want[i])
    assert cnt["n_flagged"] == len(flagged) >= 8
    # the double rounding is float()'s: 2^24 + 1 + 1e-9 rounds to the tie 2^24 + 1 as float64, and from there to the even float32
    assert want[stamps.index("16777217.000000001")] == np.float32(16777216.0).view(np.uint32)


def test_seeded_random_decimals_of_up_to_19_digits():
    import random
    r = random.Random(5)
    stamps = []
    for _ in range(30000):
        nd = r.randint(1, 19)
        d = str(r.randint(1, 9)) + "".join(r.choice("0123456789") for _ in range(nd - 1))
        kind = r.random()
        if kind < 0.4:
            pt = r.randint(0, nd)
            s = d[:pt] + "." + d[pt:] if r.random() < 0.7 else "0." + "0" * r.randint(0, 30) + d
        elif kind < 0.8:
            s = d[0] + "." + d[1:] + r.choice("eE") + str(r.randint(-44, 40))
        else:
            s = d + "e" + r.choice(["", "+", "-"]) + str(r.randint(0, 42))
        stamps.append(s)
    got, flagged, _ = parse_stamps(stamps)
    want = python_bits(stamps)
    keep = np.array([i not in flagged for i in range(len(stamps))])
    assert keep.sum() > 29000 and np.array_equal(got[keep], want[keep])


# ------------------------------------------------------------------------------------------------------------------ grammar
def check(data, want_labels=False):
    rows, lab, cnt, _ = host_parse(data, want_labels)
    r_rows, r_lab, r_cnt = decode_text(data, want_labels)
    assert np.array_equal(rows.view(np.uint32), r_rows.view(np.uint32))
    assert (lab is None and r_lab is None) or np.array_equal(lab, r_lab)
    assert {k: cnt[k] for k in r_cnt} == r_cnt
    return rows, lab, cnt


def test_line_ends():
    rows, _, cnt = check(b"0.5 1 2 1\r\n0.75 3 4 0\r\n")
    assert rows.tolist() == [[0.5, 1, 2, 1], [0.75, 3, 4, -1]] and cnt["n_lines"] == 2
    rows, _, cnt = check(b"0.5 1 2 1\n0.75 3 4 0")  # a last line without newline
    assert len(rows) == 2 and cnt["n_lines"] == 2
    rows, _, cnt = check(b"0.5 1 2 1\n0.75 3 4 0\r")
    assert len(rows) == 2
    assert check(b"")[2]["n_lines"] == 0
    assert check(b"\n")[2] == {"n_rows": 0, "n_comment": 1, "n_bad": 0, "n_flagged": 0, "n_lines": 1}


def test_blanks_between_and_around_fields():
    rows, _, cnt = check(b"0.5\t1\t2\t1\n  0.75   3 \t 4  0  \n\t1 5 6 1\t\r\n")
    assert rows.tolist() == [[0.5, 1, 2, 1], [0.75, 3, 4, -1], [1, 5, 6, 1]] and cnt["n_bad"] == 0


def test_empty_and_comment_lines():
    rows, _, cnt = check(b"# header\n#!events.txt\n\n0.5 1 2 1\n   \n  # indented comment\n\r\n0.75 3 4 0\n#\n")
    assert len(rows) == 2 and cnt["n_comment"] == 7 and cnt["n_bad"] == 0 and cnt["n_lines"] == 9


def test_signs_and_bare_points():
    rows, _, cnt = check(b"+0.5 +1 -2 1\n-0.5 1 2 0\n.5 1 2 1\n5. 1 2 1\n-.5e1 1 2 1\n5.e-1 -0 2 1\n")
    assert rows[:, 0].tolist() == [0.5, -0.5, 0.5, 5.0, -5.0, 0.5] and rows[0, 1:3].tolist() == [1, -2] and cnt["n_bad"] == 0
    assert rows[5, 1] == 0 and not np.signbit(rows[5, 1])


@pytest.mark.parametrize("line", [b"0.5 1 2", b"0.5 1 2 1 0 7", b"0.5 1 2 2", b"0.5 1e3 2 1", b"nan 1 2 1", b"inf 1 2 1", b"-inf 1 2 1",
                                  b"- 1 2 1", b". 1 2 1", b"1e 1 2 1", b"1e+ 1 2 1", b"0x10 1 2 1", b"1_0 1 2 1", b"0.5 1.0 2 1",
                                  b"0.5 1 2 1x", b"0.5 1 2 01", b"0.5 16777216 2 1", b"0.5 1 -16777216 1", b"0.5 1 2 1 2", b"0.5,1,2,1",
                                  b"0.5 1 2 1\r\r", b"0.5 1 2 -1", b"1.5.2 1 2 1", b"0.5 + 2 1"])
def test_bad_lines(line):
    rows, _, cnt = check(b"0.25 9 9 1\n" + line + b"\n0.75 8 8 0\n")
    assert cnt["n_bad"] == 1 and rows.tolist() == [[0.25, 9, 9, 1], [0.75, 8, 8, -1]]


def test_largest_coordinates():
    rows, _, cnt = check(b"0.5 16777215 -16777215 1\n0.5 0016777215 2 1\n")
    assert rows[0].tolist() == [0.5, 16777215, -16777215, 1] and cnt["n_bad"] == 0


def test_want_labels_against_four_and_five_fields():
    data = b"0.5 1 2 1 1\n0.6 1 2 0 0\n0.7 1 2 1\n0.8 3 4 0 1\n"
    rows, lab, cnt = check(data, want_labels=True)
    assert rows[:, 0].tolist() == [np.float32(0.5), np.float32(0.6), np.float32(0.8)] and lab.tolist() == [True, False, True]
    assert cnt["n_bad"] == 1
    rows, lab, cnt = check(data, want_labels=False)  # the fifth column is ignored
    assert len(rows) == 4 and lab is None and cnt["n_bad"] == 0


def test_counters_accumulate_and_a_buffer_too_small_changes_nothing():
    cnt = np.zeros(8, np.int64)
    host_parse(b"0.5 1 2 1\n# c\nbad\n", counters=cnt)
    rows, _, out, _ = host_parse(b"0.5 1 2 1\n1234567890123456789012345 1 2 1\n", counters=cnt)
    assert out == {"n_rows": 3, "n_comment": 1, "n_bad": 1, "n_flagged": 1, "n_lines": 5} and len(rows) == 2
    before = cnt.copy()
    rows, _, raw, _ = host_parse(b"0.5 1 2 1\n0.5 1 2 1\n0.5 1 2 1\n", cap_rows=2, counters=cnt)
    assert rows is None and raw[5] == -1 and raw[6] == 3 and np.array_equal(raw[:5], before[:5])


def test_flagged_entries_name_the_line_and_the_row():
    data = b"# c\n0.5 1 2 1\nbad\n 1234567890123456789012345 1 2 1\n0.75 1 2 1\n1e-70 1 2 0\n"
    rows, _, cnt, fl = host_parse(data)
    assert cnt["n_flagged"] == 2 and sorted(fl.tolist()) == [[data.index(b" 123"), 1], [data.index(b"1e-70"), 3]]
    assert rows[1, 0] == np.float32(1234567890123456789012345.0) and rows[3, 0] == 0  # the best effort happens to be right here


def test_python_constants_match_the_header():
    from v2e_amd import readers
    src = open(os.path.join(ROOT, "include", "v2e_amd.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (V2E_[A-Z0-9_]+) (\d+)\b", src, flags=re.M)}
    assert defs["V2E_READER_BLOCK"] == readers.READER_BLOCK and defs["V2E_READER_COUNTERS"] == 8
    assert {k: defs["V2E_A2C_" + k[2:].upper()] for k in readers._A2C} == readers._A2C
    assert {k: defs["V2E_TXC_" + k[2:].upper()] for k in readers._TXC} == readers._TXC == TXC
    assert (defs["V2E_A2C_CALL_ROWS"], defs["V2E_TXC_CALL_ROWS"], defs["V2E_TXC_CALL_LINES"], defs["V2E_TXC_CALL_FLAGGED"]) == \
        (readers._A2C_CALL_ROWS, readers._TXC_CALL_ROWS, readers._TXC_CALL_LINES, readers._TXC_CALL_FLAGGED)


# ---------------------------------------------------------------------------------------- EventFileReader without a device
def test_reader_argument_errors_need_no_device(tmp_path):
    from v2e_amd import EventFileReader
    aedat = tmp_path / "a.aedat"
    aedat.write_bytes(b"#!AER-DAT2.0\r\n# comment\r\n" + bytes(16))
    with pytest.raises(ValueError, match="layout"):
        EventFileReader(str(aedat), width=128, height=128, device="cuda:9")  # unknown size, no layout
    with pytest.raises(ValueError, match="layout"):
        EventFileReader(str(aedat), width=128, height=128, layout=(1, 2, 3), device="cuda:9")
    with pytest.raises(ValueError, match="format"):
        EventFileReader(str(aedat), format="aedat4", device="cuda:9")
    with pytest.raises(ValueError, match="special-event bit"):  # at 640x480 address bit 10 belongs to x
        EventFileReader(str(aedat), width=640, height=480, labels=True, device="cuda:9")
    assert EventFileReader(str(aedat), width=640, height=480, device="cuda:9").layout == (1, 11, 0, 1, 1)
    rd = EventFileReader(str(aedat), width=128, height=128, layout=(1, 8, 0, 0, 0), device="cuda:9")  # no device yet: nothing read
    assert rd.format == "aedat2" and rd.data_start == 25 and rd.labels is False and rd.counters()["n_rows"] == 0
    text = tmp_path / "e.txt"
    text.write_bytes(b"# c\n0.123456789 1 2 1 0\n0.2 1 2 1 1\n")
    with pytest.raises(ValueError, match="chunk_bytes"):
        EventFileReader(str(text), chunk_bytes=16, device="cuda:9")  # smaller than the first data line
    with pytest.raises(ValueError, match="chunk_bytes"):
        EventFileReader(str(text), chunk_bytes=4, device="cuda:9")
    rd = EventFileReader(str(text), width=128, height=128, device="cuda:9")  # text needs no address layout
    assert rd.format == "text" and rd.labels is True
    assert EventFileReader(str(text), labels=False, device="cuda:9").labels is False
    assert EventFileReader(str(aedat), format="text", device="cuda:9").format == "text"


def test_aedat2_header_end_with_crlf_bare_lf_and_trailing_bytes(tmp_path):
    from v2e_amd import EventFileReader
    for name, nl in (("crlf", b"\r\n"), ("lf", b"\n")):
        head = b"#!AER-DAT2.0" + nl + b"# one" + nl + b"# two" + nl
        p = tmp_path / (name + ".aedat")
        p.write_bytes(head + bytes(8 * 5 + 3))
        rd = EventFileReader(str(p), device="cuda:9")
        assert rd.data_start == len(head) and rd.n_trailing_bytes == 3 and rd.counters()["n_trailing_bytes"] == 3
    p = tmp_path / "header_only.aedat"
    p.write_bytes(b"#!AER-DAT2.0\r\n# only a header\r\n")
    rd = EventFileReader(str(p), device="cuda:9")
    assert rd.data_start == rd.file_bytes and rd.n_trailing_bytes == 0
