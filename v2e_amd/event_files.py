"""The event files of `EventEmulator` (emulator.py:312-346, 374-400, 953-983): opening the four sinks, `prepare_storage`'s
datasets, writing one frame's events or one device-resident run's rows, closing.

AEDAT-2.0 and text: v2e_amd.sinks writers fed from the device-resident event buffer (integer conversion on the GPU,
byte-identical to the reference writers).  HDF5: the reference's own layout through h5py -- `events` uint32 [N, 4], `frame`,
`frame_ts`, `frame_idx` -- rows converted on the GPU; this module is the only place that knows that layout.  AEDAT-4:
v2e_amd.sinks.HostAEDat4Output over the third-party dv_processing package (as the reference's writer is), or any writer object
the caller passes as `dvs_aedat4`.

The functions take the emulator: the open sinks are its public attributes `dvs_h5`, `dvs_aedat2`, `dvs_aedat4`, `dvs_text` and
the four `*_dataset`s, under the reference's names; None means closed.
"""
import os

import numpy as np
import torch

def open_sinks(emu, dvs_h5, dvs_aedat2, dvs_aedat4, dvs_text):
    """emulator.py:312-346; the file names get the reference's suffixes, under emu.output_folder."""
    if not (dvs_h5 or dvs_aedat2 or dvs_aedat4 or dvs_text):
        return

    def suffixed(name, suffix):  # v2e_utils.checkAddSuffix
        return name if name.endswith(suffix) else name + suffix

    folder = emu.output_folder or ""
    if dvs_h5:
        try:
            import h5py
        except ImportError as e:
            raise NotImplementedError("dvs_h5 needs h5py: %s" % e)
        emu.dvs_h5 = h5py.File(suffixed(os.path.join(folder, dvs_h5), '.h5'), "w")
        emu.dvs_h5_dataset = emu.dvs_h5.create_dataset(
            name="events", shape=(0, 4), maxshape=(None, 4), dtype="uint32", compression="gzip")
    if dvs_aedat2:
        from .sinks import DeviceAEDat2Output
        emu.dvs_aedat2 = DeviceAEDat2Output(suffixed(os.path.join(folder, dvs_aedat2), '.aedat'),
                                            output_width=emu.output_width, output_height=emu.output_height,
                                            label_signal_noise=emu.label_signal_noise)
    if dvs_text:
        from .sinks import DeviceTextOutput
        emu.dvs_text = DeviceTextOutput(suffixed(os.path.join(folder, dvs_text), '.txt'),
                                        label_signal_noise=emu.label_signal_noise)
    if dvs_aedat4:
        if hasattr(dvs_aedat4, "appendEvents"):  # a caller-supplied writer object
            emu.dvs_aedat4 = dvs_aedat4
        else:
            from .sinks import HostAEDat4Output  # over dv_processing; NotImplementedError where that is absent
            emu.dvs_aedat4 = HostAEDat4Output(suffixed(os.path.join(folder, dvs_aedat4), '.aedat4'))


def prepare_storage(emu, n_frames, frame_ts):  # emulator.py:374-400
    if emu.dvs_h5:
        emu.frame_h5_dataset = emu.dvs_h5.create_dataset(
            name="frame", shape=(n_frames, emu.output_height, emu.output_width), dtype="uint8",
            compression="gzip")
        frame_ts_arr = np.array(frame_ts, dtype=np.float32) * 1e6
        emu.frame_ts_dataset = emu.dvs_h5.create_dataset(
            name="frame_ts", shape=(n_frames,), data=frame_ts_arr.astype(np.uint32), dtype="uint32",
            compression="gzip")
        emu.frame_ev_idx_dataset = emu.dvs_h5.create_dataset(
            name="frame_idx", shape=(n_frames,), dtype="uint64", compression="gzip")
    else:
        emu.frame_h5_dataset = emu.frame_ts_dataset = emu.frame_ev_idx_dataset = None


def any_open(emu):
    return emu.dvs_h5 is not None or emu.dvs_aedat2 is not None or emu.dvs_aedat4 is not None or emu.dvs_text is not None


def _append_h5(emu, rows_dev):
    """Device rows [n, 4] float32 to the end of `events`; the integer conversions (emulator.py:957-960) run on the GPU, on the
    current stream."""
    from .sinks import pack_h5
    temp = pack_h5(rows_dev).cpu().numpy().view(np.uint32)
    emu.dvs_h5_dataset.resize(emu.dvs_h5_dataset.shape[0] + temp.shape[0], axis=0)
    emu.dvs_h5_dataset[-temp.shape[0]:] = temp


def write_frame(emu, events, n_signal, events_dev=None):
    """emulator.py:953-977: append this frame's events to the open sinks.  The integer conversions of the HDF5 rows, the
    AEDAT-2.0 words and the text columns run on the GPU on the device-resident rows."""
    if not any_open(emu):
        return
    ev_dev = events_dev if events_dev is not None else torch.from_numpy(np.ascontiguousarray(events, dtype=np.float32)).to(
        emu._engine.device)
    sig = n_signal if emu.label_signal_noise else None
    if emu.dvs_h5 is not None:
        _append_h5(emu, ev_dev)
    if emu.dvs_aedat2 is not None:
        emu.dvs_aedat2.appendEvents(ev_dev, n_signal=sig)
    if emu.dvs_aedat4 is not None:
        label = None
        if emu.label_signal_noise:
            label = np.zeros(len(events), dtype=bool)
            label[:n_signal] = True
        emu.dvs_aedat4.appendEvents(events, signnoise_label=label)
    if emu.dvs_text is not None:
        emu.dvs_text.appendEvents(ev_dev, n_signal=sig)


def write_run(emu, frame0, r, rows_dev, rows_host):
    """write_frame for a whole device-resident run whose first frame is frame `frame0` of the clip: the run's rows go to every
    open sink, with the per-frame signal / noise labels of its records `r`.  The rows are final on the device (result() waited
    for them); the packing, formatting and copies run on the sinks' own streams."""
    total = int(rows_dev.shape[0])
    off = r["ev_offset"].astype(np.int64)
    nsig = r["n_signal"].astype(np.int64)
    nev = r["n_events"].astype(np.int64)
    if emu.dvs_h5 is not None:
        if total > 0:
            if emu._h5_stream is None:
                emu._h5_stream = torch.cuda.Stream(rows_dev.device)
            with torch.cuda.stream(emu._h5_stream):
                _append_h5(emu, rows_dev)
        if emu.frame_ev_idx_dataset is not None:  # after each frame's events (emulator.py:979-983)
            ends = emu.dvs_h5_dataset.shape[0] - total + np.cumsum(nev)
            emu.frame_ev_idx_dataset[frame0:frame0 + len(ends)] = ends.astype(np.uint64)
    if total == 0:
        return
    if emu.dvs_aedat2 is not None:
        emu.dvs_aedat2.appendRun(rows_dev, off, nsig)
    if emu.dvs_aedat4 is not None:
        if rows_host is None:
            rows_host = rows_dev.cpu().numpy()
        label = None
        if emu.label_signal_noise:
            label = np.zeros(total, dtype=bool)
            for o, k in zip(off, nsig):
                label[o:o + k] = True
        emu.dvs_aedat4.appendEvents(rows_host, signnoise_label=label)
    if emu.dvs_text is not None:
        emu.dvs_text.appendRun(rows_dev, off, nsig)


def close(emu):
    for w in ("dvs_h5", "dvs_aedat2", "dvs_aedat4", "dvs_text"):
        o = getattr(emu, w)
        if o is not None:
            try:
                o.close()
            except Exception:
                pass
            setattr(emu, w, None)
