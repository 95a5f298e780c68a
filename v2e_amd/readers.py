"""Event files read back into device rows: the sinks of sinks.py inverted (v2e_amd/csrc/readers.hip).

    rd = EventFileReader(path, width=346, height=260)
    for chunk in rd:                      # {"rows": float32 [n,4] device, "labels": bool [n] device or None, "t_us": int64 [n] device or None}
        sweep.add_run(chunk["rows"], labels=chunk["labels"])
    rd.counters()                         # what was dropped and why
    rows, labels = read_events(path)      # the whole file on the device

Two formats: AEDAT-2.0 (jAER; DeviceAEDat2Output, AEDat2Output) and text lines `t x y p[ label]` (DeviceTextOutput, RPG-style
events.txt).  The host finds the AEDAT header's end and cuts the file into chunks (AEDAT at multiples of 8 bytes, text after a
'\\n'); the bytes go through pinned memory to the device, where the records / lines are decoded and the ones that are no rows --
APS and IMU samples, special events, comment and malformed lines -- are dropped in order.  The text time stamp is
np.float32(float(s)) exactly; a stamp outside the domain the device parser decides exactly (text_parse.h: more than 19
significant digits, a decimal exponent outside +-62) is parsed again here with float() and patched into its row.
Rows, labels and counters do not depend on chunk_bytes.
"""
import os
import warnings

import numpy as np

from . import _capi
from ._capi import check, ptr, stream_ptr

# aedat2_output.py:41-77 (sinks._AEDAT2_LAYOUT): (xshift, yshift, pshift, flipx, flipy)
AEDAT2_LAYOUT = {(346, 260): (12, 22, 11, 1, 1), (240, 180): (12, 22, 11, 1, 1), (640, 480): (1, 11, 0, 1, 1)}
READER_BLOCK = 1024  # V2E_READER_BLOCK (include/v2e_amd.h): records per workgroup of the ordered compaction
# counter slots of include/v2e_amd.h (V2E_A2C_*, V2E_TXC_*)
_A2C = {"n_rows": 0, "n_aps": 1, "n_special": 2, "n_outside": 3, "n_nonmonotonic": 4}
_A2C_CALL_ROWS = 7
_TXC = {"n_rows": 0, "n_comment": 1, "n_bad": 2, "n_flagged": 3, "n_lines": 4}
_TXC_CALL_ROWS, _TXC_CALL_LINES, _TXC_CALL_FLAGGED = 5, 6, 7
COUNTER_NAMES = ("n_rows", "n_aps", "n_special", "n_outside", "n_nonmonotonic", "n_trailing_bytes", "n_lines", "n_comment", "n_bad",
                 "n_flagged", "n_host_parsed")
_FLAGGED_CAP = 4096
_MAX_HEADER_LINE = 1 << 20


def _layout(width, height, layout):
    if layout is None:
        if (width, height) not in AEDAT2_LAYOUT:
            raise ValueError("EventFileReader: no AEDAT-2.0 address layout is known for width=%d height=%d; pass "
                             "layout=(xshift, yshift, pshift, flipx, flipy)" % (width, height))
        return AEDAT2_LAYOUT[(width, height)]
    lay = tuple(int(v) for v in layout)
    if len(lay) != 5 or not all(0 <= s < 31 for s in lay[:3]):
        raise ValueError("EventFileReader: layout must be (xshift, yshift, pshift, flipx, flipy) with shifts in 0 .. 30")
    return lay


def _field_mask(size):
    m = 1
    while m < size:
        m <<= 1
    return m - 1


def _bit10_is_data(width, height, layout):
    """True where address bit 10 -- jAER's special-event bit, the sinks' noise label -- lies inside the x, y or p field."""
    xs, ys, ps = layout[:3]
    return bool(((_field_mask(width) << xs) | (_field_mask(height) << ys) | (1 << ps)) >> 10 & 1)


class EventFileReader(object):
    """An event file as chunks of device rows (module docstring).

    format   "aedat2", "text", or None: AEDAT-2.0 if the file's first line starts with `#!AER-DAT2.0`, else text
    labels   True: the special-event bit (AEDAT-2.0 written with label_signal_noise) / the fifth column (text) as labels, True =
             signal; False: special events are dropped / a fifth column is ignored; None: True for a text file whose first data
             line has five fields, else False.  The 640x480 layout keeps x in address bits 1 .. 10, so there bit 10 is a
             coordinate bit: nothing is dropped as special, and labels=True is a ValueError
    layout   AEDAT-2.0 address layout (xshift, yshift, pshift, flipx, flipy); None: the writer's for 346x260, 240x180, 640x480
    chunk_bytes   how much of the file goes to the device at a time; a text line longer than this is a ValueError
    Every ValueError about the arguments is raised before the device is touched."""

    def __init__(self, path, width=346, height=260, format=None, labels=None, layout=None, chunk_bytes=64 << 20, device="cuda:0"):
        if format not in (None, "aedat2", "text"):
            raise ValueError("EventFileReader: format must be 'aedat2', 'text' or None, got %r" % (format,))
        self.path = path
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1 or self.width > 1 << 15 or self.height > 1 << 15:
            raise ValueError("EventFileReader: width and height must be in 1 .. 32768")
        self.chunk_bytes = int(chunk_bytes)
        if self.chunk_bytes < 8:
            raise ValueError("EventFileReader: chunk_bytes must be at least 8")
        self.device = device
        self.file_bytes = os.path.getsize(path)
        with open(path, "rb") as f:
            first = f.readline(_MAX_HEADER_LINE)
            self.format = format or ("aedat2" if first.startswith(b"#!AER-DAT2.0") else "text")
            if self.format == "aedat2":
                self.layout = _layout(self.width, self.height, layout)
                self.labels = bool(labels)
                if self.labels and _bit10_is_data(self.width, self.height, self.layout):
                    raise ValueError("EventFileReader: in this AEDAT-2.0 layout the special-event bit (10) lies inside a coordinate "
                                     "field, so it cannot carry labels (label_signal_noise at 640x480 overwrites a bit of x)")
                self.data_start = self._aedat_header_end(f)
                self.n_trailing_bytes = (self.file_bytes - self.data_start) % 8
            else:
                self.layout = None
                self.data_start = 0
                self.n_trailing_bytes = 0
                five = self._first_data_line_fields(f) == 5
                self.labels = five if labels is None else bool(labels)
        self.n_host_parsed = 0
        self._counters = None

    @staticmethod
    def _aedat_header_end(f):
        """The offset of the first byte after the run of '#' lines at the file's start (CRLF or bare LF line ends)."""
        f.seek(0)
        pos = 0
        while True:
            c = f.read(1)
            if c != b"#":
                return pos
            line = f.readline(_MAX_HEADER_LINE)
            if not line.endswith(b"\n"):  # a header line without an end: the file is header only (or not AEDAT-2.0 at all)
                if len(line) >= _MAX_HEADER_LINE:
                    raise ValueError("EventFileReader: an AEDAT-2.0 header line of more than %d bytes" % _MAX_HEADER_LINE)
                return pos + 1 + len(line)
            pos += 1 + len(line)

    def _first_data_line_fields(self, f):
        """The number of fields of the first line that is neither empty nor a comment (0: there is none)."""
        f.seek(0)
        while True:
            line = f.readline(self.chunk_bytes + 1)
            if not line:
                return 0
            if len(line) > self.chunk_bytes:
                raise ValueError("EventFileReader: a line of %s is longer than chunk_bytes=%d" % (self.path, self.chunk_bytes))
            s = line.strip(b" \t\r\n")
            if s and not s.startswith(b"#"):
                return len(s.split())

    # ---------------------------------------------------------------------------------------------------------------- chunks
    def _pieces(self, pinned):
        """(buffer index, n bytes) of each chunk, read into pinned[0] / pinned[1] in turn: AEDAT-2.0 whole records, text whole lines
        (the rest of a piece after its last '\\n' is moved in front of the next one)."""
        cap = int(pinned[0].numel())
        views = [p.numpy() for p in pinned]
        with open(self.path, "rb") as f:
            f.seek(self.data_start)
            if self.format == "aedat2":
                left = (self.file_bytes - self.data_start) // 8 * 8
                k = 0
                while left > 0:
                    n = f.readinto(memoryview(views[k])[:min(cap, left)])
                    if n <= 0 or n % 8:
                        raise IOError("EventFileReader: short read of %s" % self.path)
                    left -= n
                    yield k, n
                    k ^= 1
                return
            k, tail = 0, np.empty(0, np.uint8)
            while True:
                carry = len(tail)  # (moved only now: the other buffer's chunk has been handed out and is done with)
                views[k][:carry] = tail
                got = f.readinto(memoryview(views[k])[carry:cap]) if carry < cap else 0
                fill = carry + got
                if fill == 0:
                    return
                if not f.peek(1):  # the file's end: what is left is the last chunk, with or without a last '\n'
                    yield k, fill
                    return
                cut = _last_newline(views[k], fill)
                if cut < 0:
                    raise ValueError("EventFileReader: a line of %s is longer than chunk_bytes=%d" % (self.path, self.chunk_bytes))
                tail = views[k][cut + 1:fill].copy()
                yield k, cut + 1
                k ^= 1

    def __iter__(self):
        import torch
        lib = _capi.lib()
        dev = torch.device(self.device)
        aedat = self.format == "aedat2"
        payload = max(self.file_bytes - self.data_start, 16)
        cap = min(self.chunk_bytes // 8 * 8 if aedat else self.chunk_bytes, (payload + 15) // 16 * 16)
        with torch.cuda.device(dev):
            pinned = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            dbytes = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
            self._counters = torch.zeros(8, dtype=torch.int64, device=dev)
        self.n_host_parsed = 0
        decode = self._decode_aedat2 if aedat else self._decode_text
        pieces = self._pieces(pinned)
        nxt = next(pieces, None)
        while nxt is not None:
            k, n = nxt
            with torch.cuda.device(dev):  # (not held across the yield: the caller's current device stays the caller's)
                dbytes[k][:n].copy_(pinned[k][:n], non_blocking=True)
                pending = decode(lib, dev, dbytes[k], n)   # enqueued; the next piece is read from the file meanwhile
            nxt = next(pieces, None)
            with torch.cuda.device(dev):
                chunk = pending(pinned[k])
            if int(chunk["rows"].shape[0]):
                yield chunk

    def _decode_aedat2(self, lib, dev, dbytes, n):
        import torch
        nrec = n // 8
        rows = torch.empty((nrec, 4), dtype=torch.float32, device=dev)
        labels = torch.empty(nrec, dtype=torch.uint8, device=dev) if self.labels else None
        t_us = torch.empty(nrec, dtype=torch.int64, device=dev)
        scratch = torch.empty(int(lib.v2e_events_unpack_aedat2_scratch_bytes(nrec)), dtype=torch.uint8, device=dev)
        xs, ys, ps, fx, fy = self.layout
        check(lib.v2e_events_unpack_aedat2(ptr(dbytes), nrec, self.width, self.height, xs, ys, ps, fx, fy, 1 if self.labels else 0,
                                           ptr(rows), ptr(labels), ptr(t_us), ptr(self._counters), ptr(scratch), stream_ptr(dev)),
              "v2e_events_unpack_aedat2")

        def finish(_host_bytes):
            kept = int(self._counters[_A2C_CALL_ROWS].item())
            return {"rows": rows[:kept], "labels": None if labels is None else labels[:kept].view(torch.bool), "t_us": t_us[:kept]}
        return finish

    def _decode_text(self, lib, dev, dbytes, n):
        import torch
        state = {"cap_rows": n // 16 + 64, "cap_flagged": _FLAGGED_CAP}
        saved = self._counters.clone()

        def launch():
            cr, cf = state["cap_rows"], state["cap_flagged"]
            state["rows"] = torch.empty((cr, 4), dtype=torch.float32, device=dev)
            state["labels"] = torch.empty(cr, dtype=torch.uint8, device=dev) if self.labels else None
            state["flagged"] = torch.empty((cf, 2), dtype=torch.int64, device=dev)
            scratch = torch.empty(int(lib.v2e_events_parse_text_scratch_bytes(n, cr)), dtype=torch.uint8, device=dev)
            check(lib.v2e_events_parse_text(ptr(dbytes), n, 1 if self.labels else 0, ptr(state["rows"]), ptr(state["labels"]), cr,
                                            ptr(self._counters), ptr(state["flagged"]), cf, ptr(scratch), stream_ptr(dev)),
                  "v2e_events_parse_text")
        launch()

        def finish(host_bytes):
            while True:
                c = self._counters.cpu().numpy()
                kept, lines, nflag = int(c[_TXC_CALL_ROWS]), int(c[_TXC_CALL_LINES]), int(c[_TXC_CALL_FLAGGED])
                if kept >= 0 and nflag <= state["cap_flagged"]:
                    break
                # more lines than the guess, or more flagged ones than the list holds: make room and decode the chunk again
                self._counters.copy_(saved)
                state["cap_rows"] = max(state["cap_rows"], lines)
                state["cap_flagged"] = max(state["cap_flagged"], nflag)
                launch()
            rows, labels = state["rows"][:kept], state["labels"]
            if nflag:
                self._patch_flagged(rows, state["flagged"][:nflag].cpu().numpy(), host_bytes.numpy(), n)
            return {"rows": rows, "labels": None if labels is None else labels[:kept].view(torch.bool), "t_us": None}
        return finish

    def _patch_flagged(self, rows, flagged, host, n):
        """The time stamps the device parser could not decide exactly, parsed by float() from the chunk's bytes on the host."""
        import torch
        vals = np.empty(len(flagged), np.float32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (a stamp beyond float32's range becomes inf, as it does for every host reader)
            for j, (off, _row) in enumerate(flagged):
                vals[j] = np.float32(float(_first_token(host, int(off), n).decode("ascii")))
        idx = torch.from_numpy(flagged[:, 1].copy()).to(rows.device)
        rows[idx, 0] = torch.from_numpy(vals).to(rows.device)
        self.n_host_parsed += len(flagged)

    def counters(self):
        """{name: int} for COUNTER_NAMES -- what was read so far and what was dropped (one small read-back; zeros before the first
        chunk): n_rows; AEDAT-2.0: n_aps, n_special, n_outside (kept), n_nonmonotonic (kept), n_trailing_bytes; text: n_lines,
        n_comment (and empty), n_bad, n_flagged = n_host_parsed (stamps parsed again on the host)."""
        out = dict.fromkeys(COUNTER_NAMES, 0)
        if self._counters is not None:
            c = self._counters.cpu().numpy()
            for name, slot in (_A2C if self.format == "aedat2" else _TXC).items():
                out[name] = int(c[slot])
        out["n_trailing_bytes"] = int(self.n_trailing_bytes)
        out["n_host_parsed"] = int(self.n_host_parsed)
        return out


def _first_token(buf, off, n):
    """The first blank-separated token of buf[off:n] (uint8 array) as bytes."""
    window = 256
    while True:
        parts = buf[off:min(off + window, n)].tobytes().split(None, 1)
        if len(parts) == 2 or off + window >= n:
            return parts[0]
        window *= 8


def _last_newline(buf, fill):
    """Index of the last '\\n' in buf[:fill] (uint8 array), -1 if there is none; looks at the tail first."""
    hi, step = fill, 1 << 16
    while hi > 0:
        lo = max(0, hi - step)
        hit = np.flatnonzero(buf[lo:hi] == 10)
        if len(hit):
            return lo + int(hit[-1])
        hi, step = lo, step * 4
    return -1


def read_events(path, **kwargs):
    """The whole file: (rows float32 [n,4], labels bool [n] or None) on the device, EventFileReader's chunks concatenated.
    kwargs: EventFileReader's."""
    import torch
    rd = EventFileReader(path, **kwargs)
    rows, labels = [], []
    for chunk in rd:
        rows.append(chunk["rows"])
        labels.append(chunk["labels"])
    if not rows:
        dev = torch.device(rd.device)
        return (torch.empty((0, 4), dtype=torch.float32, device=dev),
                torch.empty(0, dtype=torch.bool, device=dev) if rd.labels else None)
    return torch.cat(rows), (torch.cat(labels) if rd.labels else None)
