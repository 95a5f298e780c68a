"""Device-side packing of events into the reference writers' integer formats."""
import logging
import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import check, ptr, stream_ptr

# aedat2_output.py:41-77
_AEDAT2_LAYOUT = {(346, 260): (12, 22, 11, 1, 1), (240, 180): (12, 22, 11, 1, 1), (640, 480): (1, 11, 0, 1, 1)}

logger = logging.getLogger(__name__)


_REC_DT = np.dtype([("max_events", "<i4"), ("flags", "<u4"), ("n_signal", "<u4"), ("n_events", "<u4"), ("n_on", "<u4"),
                    ("n_off", "<u4"), ("ev_offset", "<u8")])  # struct v2e_frame_rec


def frames_from_labels(signnoise_label):
    """The reference's boolean label array (True = signal) as a frame table (ev_offset, n_signal): one frame per stretch of
    equal labels, all signal or all noise, so that any labelling goes through the frame-table kernels."""
    lab = np.asarray(signnoise_label.detach().cpu().numpy() if torch.is_tensor(signnoise_label) else signnoise_label).astype(bool)
    n = len(lab)
    if n == 0:
        return np.zeros(1, np.int64), np.zeros(1, np.int64)
    starts = np.concatenate([[0], np.flatnonzero(lab[1:] != lab[:-1]) + 1]).astype(np.int64)
    lens = np.diff(np.concatenate([starts, [n]]))
    return starts, np.where(lab[starts], lens, 0).astype(np.int64)


class _Staging:
    """Buffers of one sink: a device frame table, device bytes and scratch, pinned host bytes, all grown on demand and reused;
    and the sink's own stream, on which a run's bytes are made and copied (never the caller's stream, which carries the chain)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(self.device)
        self.buf = {}

    def get(self, name, n, dtype, pinned=False):
        t = self.buf.get(name)
        if t is None or t.numel() < n:
            n = max(int(n * 1.25), 1 << 12)
            t = torch.empty(n, dtype=dtype, pin_memory=True) if pinned else torch.empty(n, dtype=dtype, device=self.device)
            self.buf[name] = t
        return t

    def frame_table(self, ev_offset, n_signal):
        """Device struct v2e_frame_rec[F] with ev_offset and n_signal set (what the kernels read), uploaded on the current stream."""
        rec = _frame_recs(ev_offset, n_signal)
        F = len(rec)
        nb = F * _REC_DT.itemsize
        host = self.get("rec_host", nb, torch.uint8, pinned=True)
        host[:nb].copy_(torch.from_numpy(rec.view(np.uint8)))
        dev = self.get("rec_dev", nb, torch.uint8)
        dev[:nb].copy_(host[:nb], non_blocking=True)
        return dev, F

    def to_host(self, src, nbytes):
        """src[:nbytes] (device uint8) into the pinned buffer on the current stream; the caller synchronises."""
        host = self.get("host_bytes", nbytes, torch.uint8, pinned=True)
        host[:nbytes].copy_(src[:nbytes], non_blocking=True)
        return host


def _device_rows(events):
    ev = events if torch.is_tensor(events) else torch.from_numpy(np.ascontiguousarray(events, dtype=np.float32))
    if not ev.is_cuda:
        ev = ev.cuda()
    return ev.contiguous()


def _frame_recs(ev_offset, n_signal):
    rec = np.zeros(len(ev_offset), dtype=_REC_DT)
    rec["ev_offset"] = np.asarray(ev_offset, dtype=np.int64)
    rec["n_signal"] = np.asarray(n_signal, dtype=np.int64)
    return rec


def _format_text_call(ev, n, labels, recs, nrec, nsig0, out, scratch, stream):
    check(_capi.lib().v2e_events_format_text(ptr(ev) if n else None, n, recs, nrec, nsig0, 1 if labels else 0, ptr(out),
                                             int(out.numel()), ptr(scratch), C.c_void_p(stream.cuda_stream)),
          "v2e_events_format_text")


def format_text(events_dev, labels=False, n_signal=None, frames=None, out=None):
    """events_dev: device float32 [N,4] -> (device uint8 text, its length in bytes): the lines DVSTextOutput.appendEvents
    writes for these rows (ae_text_output.py:86-101), formatted on the GPU (v2e_events_format_text) on the current stream.
    labels: add the signal/noise column -- 1 for the first n_signal rows (one frame), or per frame with frames = (ev_offset,
    n_signal) arrays of a run.  out: a device uint8 buffer to write into; one that is too small raises V2EAmdError and is
    left untouched.  Zero rows give zero bytes."""
    ev = events_dev.contiguous()
    n = int(ev.shape[0])
    dev = ev.device
    stream = torch.cuda.current_stream(dev)
    scratch = torch.empty(int(_capi.lib().v2e_events_format_text_scratch_words(n)), dtype=torch.int64, device=dev)
    recs, nrec, nsig0 = None, 0, 0
    if labels and frames is not None:
        rec = torch.from_numpy(_frame_recs(*frames).view(np.uint8)).to(dev)
        recs, nrec = ptr(rec), len(frames[0])
    elif labels:
        nsig0 = n if n_signal is None else int(n_signal)
    own = out is None
    if own:
        out = torch.empty(max(32 * n, 1), dtype=torch.uint8, device=dev)
    _format_text_call(ev, n, labels, recs, nrec, nsig0, out, scratch, stream)
    total = int(scratch[0].item())
    if total > out.numel():
        if not own:
            raise _capi.V2EAmdError("v2e_events_format_text: the text needs %d bytes, the buffer holds %d" % (total, out.numel()))
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        _format_text_call(ev, n, labels, recs, nrec, nsig0, out, scratch, stream)
    return out, total


def pack_aedat2(events_dev, width, height, noise_from=-1):
    """events_dev: device float32 [N,4] -> device uint8 [N*8], the bytes AEDat2Output.appendEvents would write."""
    if (width, height) not in _AEDAT2_LAYOUT:
        raise ValueError(f'AEDAT-2.0 output width={width} height={height} not supported')  # aedat2_output.py:78-80
    xs, ys, ps, fx, fy = _AEDAT2_LAYOUT[(width, height)]
    n = int(events_dev.shape[0])
    out = torch.empty((n * 8,), dtype=torch.uint8, device=events_dev.device)
    s = stream_ptr(events_dev.device)
    check(_capi.lib().v2e_events_pack_aedat2(ptr(events_dev.contiguous()), ptr(out), n, width, height, xs, ys, ps, fx, fy,
                                             int(noise_from), s), "v2e_events_pack_aedat2")
    return out


def pack_h5(events_dev):
    """events_dev: device float32 [N,4] -> device int64-free uint32 rows (as int32 tensor bit pattern) [N,4]."""
    n = int(events_dev.shape[0])
    out = torch.empty((n, 4), dtype=torch.int32, device=events_dev.device)  # torch has no uint32 arithmetic; same bits
    s = stream_ptr(events_dev.device)
    check(_capi.lib().v2e_events_pack_h5(ptr(events_dev.contiguous()), ptr(out), n, s), "v2e_events_pack_h5")
    return out


class DeviceAEDat2Output:
    """AEDAT-2.0 file sink fed from the device-resident event buffer (mirrors v2ecore/output/aedat2_output.py: same
    header lines, same address layout per sensor size, big-endian (address, timestamp) int32 pairs, noise events marked
    as special events with label_signal_noise).  The integer conversion and the byte order are done on the GPU
    (v2e_events_pack_aedat2, byte-identical to the reference writer: tests/test_sinks.py); the host only moves bytes."""

    def __init__(self, filepath, output_width=346, output_height=260, label_signal_noise=False):
        import atexit
        if (output_width, output_height) not in _AEDAT2_LAYOUT:
            raise ValueError(f'AEDAT-2.0 output width={output_width} height={output_height} not supported')  # aedat2_output.py:78-80
        self.filepath = filepath
        self.width, self.height = output_width, output_height
        self.label_signal_noise = label_signal_noise
        self.numEventsWritten = self.numOnEvents = self.numOffEvents = 0
        self.file = open(filepath, 'wb')
        self._staging = None
        self._writeHeader()
        atexit.register(self.cleanup)

    def cleanup(self):
        self.close()

    def close(self):
        if self.file:
            self.file.close()
            self.file = None

    def _writeHeader(self):  # aedat2_output.py:111-133, CRLF line ends (jAER)
        import datetime
        import getpass
        import time
        date = datetime.datetime.now().strftime('# Creation time: %I:%M%p %B %d %Y\r\n')
        tms = '# Creation time: System.currentTimeMillis() {}\r\n'.format(int(time.time() * 1000.))
        user = '# User name: {}\r\n'.format(getpass.getuser())
        sn_comment = ('# noise events are labeled as addressed external input events when the --label_signal_noise option is '
                      'selected for output\r\n') if self.label_signal_noise else ''
        header = ('#!AER-DAT2.0\r\n',
                  '# This is a raw AE data file created by AEDat2Output in v2e (see https://github.com/SensorsINI/v2e) as '
                  'specified at https://inivation.com/support/software/fileformat/#aedat-20\r\n',
                  '# Data format is int32 address, int32 timestamp (8 bytes total), repeated for each event\r\n',
                  '# Timestamps tick is 1 us\r\n', sn_comment, date, tms, user)
        for line in header:
            self.file.write(line.encode('UTF-8'))

    def appendEvents(self, events, signnoise_label=None, n_signal=None):
        """events: [N,4] float32 rows (t, x, y, p) as a device tensor or a host array; noise labelling either by the
        reference's boolean array (True = signal) or by `n_signal` (rows from n_signal on are noise, how the emulator
        orders a frame's events)."""
        if self.file is None or events is None or len(events) == 0:
            return
        ev = events if torch.is_tensor(events) else torch.from_numpy(events.astype('float32', copy=False))
        if not ev.is_cuda:
            ev = ev.cuda()
        n = int(ev.shape[0])
        noise_from = -1
        if self.label_signal_noise:
            if n_signal is not None:
                noise_from = int(n_signal)
            elif signnoise_label is not None:  # general labels: sort is not needed, mark per run of equal labels
                lab = torch.as_tensor(signnoise_label).bool().cpu().numpy()
                out = bytearray()
                i = 0
                while i < n:
                    j = i
                    while j < n and lab[j] == lab[i]:
                        j += 1
                    out += bytes(pack_aedat2(ev[i:j], self.width, self.height, noise_from=-1 if lab[i] else 0).cpu().numpy())
                    i = j
                data = bytes(out)
                self._write(data, ev)
                return
        data = pack_aedat2(ev, self.width, self.height, noise_from=noise_from).cpu().numpy().tobytes()
        self._write(data, ev)

    def _write(self, data, ev):
        n = len(data) // 8
        if self.numEventsWritten == 0:  # aedat2_output.py:173-179: a first byte '#' would read as a comment line
            while data[0:1] == b'#':
                data = data[8:]
        self.file.write(data)
        self.numEventsWritten += n
        on = int((ev[:, 3] > 0).sum().item())
        self.numOnEvents += on
        self.numOffEvents += n - on
        self.file.flush()

    def appendRun(self, events_dev, ev_offset, n_signal):
        """The rows of a whole run, as if appendEvents had been called once per frame: device rows that are final (the caller
        has waited for them), frame f starting at row ev_offset[f] with its first n_signal[f] rows signal.  Packed on the
        sink's own stream (v2e_events_pack_aedat2_run: the noise bit per frame), copied once into pinned memory, one write."""
        if self.file is None or events_dev is None or int(events_dev.shape[0]) == 0:
            return
        ev = events_dev.contiguous()
        n = int(ev.shape[0])
        st = self._staging = self._staging or _Staging(ev.device)
        xs, ys, ps, fx, fy = _AEDAT2_LAYOUT[(self.width, self.height)]
        with torch.cuda.stream(st.stream):
            recs, nrec = None, 0
            if self.label_signal_noise:
                rec_t, nrec = st.frame_table(ev_offset, n_signal)
                recs = ptr(rec_t)
            out = st.get("dev_bytes", 8 * n, torch.uint8)
            check(_capi.lib().v2e_events_pack_aedat2_run(ptr(ev), ptr(out), n, self.width, self.height, xs, ys, ps, fx, fy, recs,
                                                         nrec, C.c_void_p(st.stream.cuda_stream)), "v2e_events_pack_aedat2_run")
            on = (ev[:, 3] > 0).sum()
            host = st.to_host(out, 8 * n)
            st.stream.synchronize()
        data = memoryview(host.numpy())[:8 * n]
        if self.numEventsWritten == 0:
            # the '#' rule of the per-frame path applies to the first frame that has rows: its leading rows only
            off = np.append(np.asarray(ev_offset, dtype=np.int64), n)
            f = int(np.flatnonzero(off[1:] > off[:-1])[0])
            a, b = int(off[f]), int(off[f + 1])
            k = a
            while k < b and data[8 * k] == 0x23:
                k += 1
            if k > a:
                self.file.write(data[:8 * a])
                data = data[8 * k:]
        self.file.write(data)
        self.numEventsWritten += n
        on = int(on.item())
        self.numOnEvents += on
        self.numOffEvents += n - on
        self.file.flush()


class DeviceTextOutput:
    """Text event sink (v2ecore/output/ae_text_output.py:51-101: `t x y p[ label]` per line, p in {0, 1}, t the Python
    repr of the float64 value of the float32 time stamp).  The lines are made on the GPU (v2e_events_format_text: the
    shortest round-trip decimal of t included, v2e_amd/csrc/text_format.h), copied once into pinned memory and written
    with one file.write per call."""

    def __init__(self, filepath, label_signal_noise=False):
        import atexit
        self.filepath = filepath
        self.label_signal_noise = label_signal_noise
        self.numEventsWritten = 0
        self.file = open(filepath, 'wb')
        self._staging = None
        self._writeHeader()
        atexit.register(self.cleanup)

    def cleanup(self):
        self.close()

    def close(self):
        if self.file:
            self.file.close()
            self.file = None

    def _writeHeader(self):  # ae_text_output.py:51-66
        import datetime
        import getpass
        import time
        if not self.label_signal_noise:
            fmt = '# Format is time (float s), x, y, polarity (0=off, 1=on) as specified at http://rpg.ifi.uzh.ch/davis_data.html\n'
        else:
            fmt = ('# Format is time (float s), x, y, polarity (0=off, 1=on), signal/noise (1/0)\n#  as specified at '
                   'http://rpg.ifi.uzh.ch/davis_data.html\n')
        date = datetime.datetime.now().strftime('# Creation time: %I:%M%p %B %d %Y\n')
        tms = '# Creation time: System.currentTimeMillis() {}\n'.format(int(time.time() * 1000.))
        user = '# User name: {}\n'.format(getpass.getuser())
        for line in ('#!events.txt\n', '# This is a text DVS created by v2e (see https://github.com/SensorsINI/v2e)\n', fmt, date,
                     tms, user):
            self.file.write(line.encode('UTF-8'))

    def appendEvents(self, events, signnoise_label=None, n_signal=None):
        """events: [N,4] float32 rows as a device tensor or a host array; the label column (label_signal_noise) from
        `n_signal` (the first n_signal rows are signal) or the reference's boolean array.  Formatted on the current stream,
        behind whatever made the rows."""
        if self.file is None:
            raise Exception('output file closed already')
        if events is None or len(events) == 0:
            return
        ev = _device_rows(events)
        frames, nsig0 = None, 0
        labels = self.label_signal_noise and (n_signal is not None or signnoise_label is not None)
        if labels:
            if n_signal is not None:
                nsig0 = int(n_signal)
            else:
                frames = frames_from_labels(signnoise_label)
        self._emit(ev, labels, frames, nsig0, torch.cuda.current_stream(ev.device))

    def appendRun(self, events_dev, ev_offset, n_signal):
        """The rows of a whole run, as if appendEvents had been called once per frame: device rows that are final (the caller
        has waited for them), frame f starting at row ev_offset[f] with its first n_signal[f] rows signal.  Formatted on the
        sink's own stream."""
        if self.file is None:
            raise Exception('output file closed already')
        if events_dev is None or int(events_dev.shape[0]) == 0:
            return
        st = self._stage(events_dev.device)
        frames = (ev_offset, n_signal) if self.label_signal_noise else None
        self._emit(events_dev.contiguous(), self.label_signal_noise, frames, 0, st.stream)

    def _stage(self, device):
        if self._staging is None:
            self._staging = _Staging(device)
        return self._staging

    def _emit(self, ev, labels, frames, nsig0, stream):
        n = int(ev.shape[0])
        st = self._stage(ev.device)
        with torch.cuda.stream(stream):
            recs, nrec = None, 0
            if frames is not None:
                rec_t, nrec = st.frame_table(*frames)
                recs = ptr(rec_t)
            scratch = st.get("scratch", int(_capi.lib().v2e_events_format_text_scratch_words(n)), torch.int64)
            total_h = st.get("total", 1, torch.int64, pinned=True)
            out = st.get("dev_bytes", 32 * n, torch.uint8)
            for _ in range(2):
                _format_text_call(ev, n, labels, recs, nrec, nsig0, out, scratch, stream)
                total_h[:1].copy_(scratch[:1], non_blocking=True)
                stream.synchronize()
                total = int(total_h[0])
                if total <= out.numel():
                    break
                out = st.get("dev_bytes", total, torch.uint8)  # the lines are longer than the guess: grow, format again
            host = st.to_host(out, total)
            stream.synchronize()
        self.file.write(memoryview(host.numpy())[:total])
        self.numEventsWritten += n


class HostAEDat4Output:
    """AEDAT-4.0 sink (v2ecore/output/aedat4_output.py:17-99) over the third-party `dv_processing` package the reference
    requires for this format (requirements.txt: dv-processing >= 1.7.8; not part of either tree).  Same conversions as the
    reference's appendEvents -- t = int(t * 1e6) in the precision this host's numpy gives a float32 scalar times a Python float
    (float64 before numpy 2, float32 from numpy 2 on), p = int((p + 1) / 2), no flips, one EventStore written at close() -- vectorised on the host; the file
    container (flatbuffers + compression) is dv_processing's.  Raises NotImplementedError where dv_processing is not importable:
    pass any object with appendEvents(events, signnoise_label=None) / close() as `dvs_aedat4` instead."""

    def __init__(self, filepath, output_width=640, output_height=480):
        try:
            import dv_processing as dv
        except ImportError as e:
            raise NotImplementedError("dvs_aedat4 needs the dv_processing package (%s); alternatively pass a writer object with "
                                      "appendEvents(events, signnoise_label=None) and close() as dvs_aedat4" % e)
        self.filepath = filepath
        self.numEventsWritten = self.numOnEvents = self.numOffEvents = 0
        self.sizex, self.sizey = output_width, output_height
        self.store = dv.EventStore()
        config = dv.io.MonoCameraWriter.EventOnlyConfig("DVXplorer_sample", (640, 480))  # aedat4_output.py:36-38
        self.writer = dv.io.MonoCameraWriter(filepath, config)

    def cleanup(self):
        self.close()

    def close(self):
        if self.writer:
            self.writer.writeEvents(self.store)
            self.writer = None

    def appendEvents(self, events, signnoise_label=None):
        import numpy as np
        if self.writer is None or events is None or len(events) == 0:
            return
        ev = events.detach().cpu().numpy() if torch.is_tensor(events) else np.asarray(events)
        # aedat4_output.py:82 `int(event[0] * 1e6)`: a float32 SCALAR times a Python float -- float64 under numpy < 2 (value-based
        # promotion), float32 under numpy >= 2 (NEP 50: the Python float is weak); this host's numpy decides, as it would for the reference
        if int(np.__version__.split(".")[0]) >= 2:
            t = (ev[:, 0].astype(np.float32) * np.float32(1e6)).astype(np.int64)
        else:
            t = (ev[:, 0].astype(np.float64) * 1e6).astype(np.int64)
        x = ev[:, 1].astype(np.int64)
        y = ev[:, 2].astype(np.int64)
        p = ((ev[:, 3].astype(np.float64) + 1) / 2).astype(np.int64)
        for i in range(ev.shape[0]):
            try:  # aedat4_output.py:84-87: an event the store refuses (a time stamp that goes backwards) is logged and skipped
                self.store.push_back(int(t[i]), int(x[i]), int(y[i]), int(p[i]))
            except RuntimeError as e:
                logger.warning('caught exception event {} to store'.format(e))
        on = int((p == 1).sum())
        self.numOnEvents += on
        self.numOffEvents += int(ev.shape[0]) - on
        self.numEventsWritten += int(ev.shape[0])


class EventFrameAccumulator:
    """Device version of EventRenderer.accumulate_event_frame (renderer.py:368-400): ON/OFF 2-D histogram of a
    slice of events added to a running, clipped frame.  The exposure-mode slicing (renderer.py:161-366) stays
    with the caller."""

    def __init__(self, height, width, full_scale_count, device="cuda", histrange=None):
        self.height, self.width, self.full_scale_count = int(height), int(width), float(full_scale_count)
        self.device = torch.device(device)
        self.histrange = histrange
        self.currentFrame = torch.zeros((self.height, self.width), dtype=torch.float64, device=self.device)
        self._diff = torch.zeros((self.height, self.width), dtype=torch.int32, device=self.device)

    def accumulate(self, events_dev, sensor_height=None, sensor_width=None):
        hr = self.histrange or [(0, sensor_height or self.height), (0, sensor_width or self.width)]  # renderer.py:232
        n = int(events_dev.shape[0])
        s = stream_ptr(self.device)
        check(_capi.lib().v2e_events_accumulate_frame(ptr(events_dev.contiguous()) if n else None, n, ptr(self.currentFrame),
                                                      ptr(self._diff), self.height, self.width, float(hr[0][0]), float(hr[0][1]),
                                                      float(hr[1][0]), float(hr[1][1]), self.full_scale_count, s),
              "v2e_events_accumulate_frame")
        return self.currentFrame
