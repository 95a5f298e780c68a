"""Pure numpy / Python reference decoders for tests/test_event_reader_*.py: what v2e_amd.readers must return, written the slow
and obvious way.  AEDAT-2.0 by np.frombuffer(..., '>i4') and bit operations; text by line.split() with float() / int() and
the grammar of v2e_amd/csrc/text_parse.h."""
import re
import warnings

import numpy as np

LAYOUT = {(346, 260): (12, 22, 11, 1, 1), (240, 180): (12, 22, 11, 1, 1), (640, 480): (1, 11, 0, 1, 1)}  # aedat2_output.py:41-77

TIME_RE = re.compile(rb"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?\Z")
INT_RE = re.compile(rb"[+-]?[0-9]+\Z")


def aedat2_header_end(data):
    """Offset of the first byte after the run of '#' lines at the start of the file's bytes."""
    pos = 0
    while data[pos:pos + 1] == b"#":
        nl = data.find(b"\n", pos)
        if nl < 0:
            return len(data)
        pos = nl + 1
    return pos


def _mask(size):
    m = 1
    while m < size:
        m <<= 1
    return m - 1


def decode_aedat2(payload, width, height, layout=None, labels=False):
    """payload: the bytes after the header.  Returns rows float32 [n,4], labels bool [n] or None, t_us int64 [n], counters."""
    xs, ys, ps, fx, fy = layout or LAYOUT[(width, height)]
    n = len(payload) // 8
    rec = np.frombuffer(payload[:8 * n], ">i4").reshape(n, 2).astype(np.int64)
    addr, ts = rec[:, 0] & 0xFFFFFFFF, rec[:, 1]
    aps = (addr >> 31) & 1 == 1
    bit10_is_data = ((_mask(width) << xs) | (_mask(height) << ys) | (1 << ps)) >> 10 & 1  # 640x480: x lies in bits 1 .. 10
    assert not (bit10_is_data and labels)
    special = ((addr >> 10) & 1 == 1) & ~aps & (not bit10_is_data)
    keep = ~aps if labels else ~aps & ~special
    a, t_us = addr[keep], ts[keep]
    x, y = (a >> xs) & _mask(width), (a >> ys) & _mask(height)
    if fx:
        x = (width - 1) - x
    if fy:
        y = (height - 1) - y
    p = np.where((a >> ps) & 1 == 1, 1.0, -1.0)
    rows = np.stack([(t_us.astype(np.float64) * 1e-6).astype(np.float32), x.astype(np.float32), y.astype(np.float32),
                     p.astype(np.float32)], axis=1) if len(a) else np.zeros((0, 4), np.float32)
    counters = {"n_rows": int(keep.sum()), "n_aps": int(aps.sum()), "n_special": 0 if labels else int(special.sum()),
                "n_outside": int(((x < 0) | (x >= width) | (y < 0) | (y >= height)).sum()),
                "n_nonmonotonic": int((t_us[1:] < t_us[:-1]).sum()), "n_trailing_bytes": len(payload) % 8}
    return rows, ((a >> 10) & 1 == 0) if labels else None, t_us, counters


def parse_text_line(line, want_labels):
    """One line without its '\\n'.  None: empty or comment; "bad"; or (t float32, x, y, p, label or None)."""
    if line.endswith(b"\r"):
        line = line[:-1]
    s = line.strip(b" \t")
    if not s or s.startswith(b"#"):
        return None
    f = re.split(rb"[ \t]+", s)
    if len(f) not in (4, 5) or (want_labels and len(f) != 5):
        return "bad"
    if not TIME_RE.match(f[0]) or not INT_RE.match(f[1]) or not INT_RE.match(f[2]) or f[3] not in (b"0", b"1"):
        return "bad"
    if len(f) == 5 and f[4] not in (b"0", b"1"):
        return "bad"
    x, y = int(f[1]), int(f[2])
    if abs(x) >= 1 << 24 or abs(y) >= 1 << 24:
        return "bad"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # float32 overflow -> inf, as numpy gives it
        t = np.float32(float(f[0].decode()))
    return t, x, y, (1.0 if f[3] == b"1" else -1.0), (f[4] == b"1" if len(f) == 5 else None)


def decode_text(data, labels=False):
    """data: the file's bytes.  Returns rows float32 [n,4], labels bool [n] or None, counters."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # the text ended with '\n' (or is empty): no last line without one
    rows, labs = [], []
    counters = {"n_rows": 0, "n_lines": len(lines), "n_comment": 0, "n_bad": 0}
    for line in lines:
        r = parse_text_line(line, labels)
        if r is None:
            counters["n_comment"] += 1
        elif r == "bad":
            counters["n_bad"] += 1
        else:
            rows.append(r[:4])
            labs.append(bool(r[4]))
    counters["n_rows"] = len(rows)
    rows = np.array(rows, dtype=np.float32).reshape(-1, 4)
    return rows, (np.array(labs, dtype=bool) if labels else None), counters
