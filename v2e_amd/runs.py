"""Device-resident runs of `EventEmulator` (generate_events_batch / generate_events_batch_async), from the point where the
call's arguments are validated: the run handle, the choice of the buffer set the run writes (`take_buffer_set`), the recorder's
sample claims (`claim_samples`), what the handle's result() does (`finish`), and the queue of runs held for the event files.

The buffer-set protocol lives here.  Event rows and records of a run are in one of three sets: 0 and 1 alternate between
asynchronous runs, 2 is the blocking call's own, so that a pending handle whose result() has not been read yet is never
overwritten by it.  Before a set is reused, the unread handle that last used it is collected (`_async_slots`, weak references:
a handle the caller has dropped needs no collecting, and a strong reference would tie the emulator and its device memory into
a cycle only the GC breaks).  While an event file is open or the single-pixel recorder is on, every run is also held strongly in
`_sink_runs` until its rows are in the files and its samples in single_pixel_states -- in the order the runs were enqueued,
whoever reads which handle first; what is still held at cleanup() / reset() is written then (`write_held`).

The functions take the emulator; the state they keep on it (`_async_flip`, `_async_slots`, `_sink_runs`, `_failed`,
`_refr_mostly_on`) is declared in its constructor and reset().
"""
import dataclasses
import logging

import numpy as np

from . import _capi, event_files, model_states

logger = logging.getLogger("v2e_amd.emulator")  # the emulator's modules log under its name, as before they were split


def default_event_capacity(n_frames, H, W):
    """Event rows a device-resident run of n_frames frames of H x W gets when no cap is given: 4 events per pixel and frame (the
    reference never drops events; a run that exceeds this raises and leaves the instance unusable until reset()), bounded to
    4 GiB of rows for very long runs."""
    per_frame = max(4 * H * W, 1 << 16)
    return per_frame * min(n_frames, max(64, (4 << 30) // (16 * per_frame)))


@dataclasses.dataclass(eq=False, repr=False)  # (identity, not field, comparison: handles are searched for with `is`)
class PendingRun:
    """Handle of an enqueued device-resident run (EventEmulator.generate_events_batch_async)."""
    emu: object            # the emulator that enqueued the run
    counts: np.ndarray     # int64 [F]: events per frame of the call (0 for the clip's very first frame), filled by result()
    start: int             # 1 where the call's first frame was the clip's first (it only initialises the state), else 0
    return_device: bool    # result() gives the device rows, not a host copy
    empty: object = None   # the [0, 4] device tensor a run without frames returns with return_device
    ev: object = None      # the buffer set's event rows [1][cap][4]; None: a run without frames (the clip's first frame alone)
    recs: object = None    # the buffer set's device records [F_run][1][32 bytes]; None like ev
    _done: object = None   # torch event behind the run on the caller's stream; None for a pipelined run until `done` is asked for
    ticket: int = None     # pipelined runs (v2e_emu_run, RUN_PIPELINED): what result() waits for on the host (v2e_emu_run_wait)
    dts: object = None     # float64 [F_run]: the frame intervals (for the refractory heuristic of the next run)
    times: list = None     # the run's frame times (the `time` series of probes)
    which: int = None      # the buffer set the run's rows and records are in
    frame0: int = 0        # 0-based index of the run's first frame in the clip (the HDF5 frame_idx slot)
    cs_steps_dev: object = None  # CSDVS: int32 [F_run] on the device, the Euler steps each frame took
    probe_dev: object = None     # a probed run's device block [F_run][probes][PROBE_FIELDS], until result() reads it
    probe_rec: bool = False      # the recorder's pixel is probe 0 of the run
    probe_claim: int = 0         # the samples the run will add to single_pixel_states
    thres: tuple = (None, None)  # (pos, neg) as Python floats where the reference would record those (emulator.py:992-995)
    probes: dict = None    # probe_pixels=...: the ten series of the probed pixels, float64 [F_run, P] each (after result())
    rec_host: object = None  # the run's records as a structured host array [F_run] (after result())
    n_signal: np.ndarray = None  # int64 [F], aligned with counts: each frame's rows start with that many signal rows, the rest
    #                              are shot noise (0 for the clip's very first frame); after result()
    _res: tuple = None     # what result() returned

    @property
    def done(self):
        """A torch event behind which the run's rows and records are final (for callers that order their own streams behind it)."""
        if self._done is None and self.recs is not None:
            self._done = self.emu._engine.run_done_event()
        return self._done

    def result(self):
        if self._res is None:
            if self.recs is None:
                self.n_signal = self.emu.last_n_signal = np.zeros(len(self.counts), dtype=np.int64)
                self._res = ((self.empty if self.return_device else None), self.counts)
            else:
                self._res = finish(self)
        return self._res


def write_held(emu):
    """Finish and write, in order, every device-resident run still held for the open sinks (cleanup(), reset()).  Runs of
    a failed instance cannot be written: they are dropped with an error in the log."""
    q = emu._sink_runs
    while q:
        pend = q[0]
        try:
            pend.result()  # writes it and takes it off the queue
        except Exception as e:
            logger.error("v2e_amd.EventEmulator: %d enqueued run(s) not written to the event files: %s", len(q), e)
            q.clear()
        if q and q[0] is pend:  # (a result computed before it could be written)
            q.pop(0)


def claim_samples(emu, nrun):
    """emulator.py:985-1009 frame by frame: a frame that finds the series full saves the file and ends the recording.  Samples
    of runs enqueued and not yet read count as taken.  Returns the samples this run will add."""
    room = emu.SINGLE_PIXEL_MAX_SAMPLES - emu.single_pixel_sample_count - sum(p.probe_claim for p in emu._sink_runs)
    if room > 0:
        return min(nrun, room)
    write_held(emu)
    if emu.record_single_pixel_states is not None:
        model_states.end_recording(emu)
    return 0


def take_buffer_set(emu, single_buffer):
    """The set this run writes, after whatever still needs the set's previous contents has read them."""
    which = 2 if single_buffer else emu._async_flip
    if not single_buffer:
        emu._async_flip = which ^ 1
    # the run that last used this buffer set and has not been read yet: collect it now -- its rows and records (and, for pipelined
    # runs, its scratch set's pinned records) are about to be reused, and a later result() would hand back this run's data instead
    old = emu._async_slots.get(which)
    old = old() if old is not None else None
    if old is not None and old._res is None and old.recs is not None:
        ev_old, counts_old = old.result()
        if old.return_device and ev_old is not None:
            old._res = (ev_old.clone(), counts_old)
    # a run held for the sinks (its handle dropped) in this buffer set: written, with every run before it, now
    last = [p for p in emu._sink_runs if p.which == which]
    if last:
        last[-1].result()
    return which


def finish(pend):
    """result() of a run with frames: the ticket or event wait, flags to errors, counters, probes, sinks."""
    emu = pend.emu
    eng = emu._engine
    held = emu._sink_runs
    if any(p is pend for p in held):
        while held[0] is not pend:  # the files get the runs in the order they were enqueued
            held[0].result()
    emu._raise_if_failed("this run started from its state: ")  # (an earlier pending run failed: its state is not the clip's)
    if pend.ticket is not None:
        eng.run_wait(pend.ticket)  # (host-blocking; no device-side wait is put into any stream's queue)
        r = eng.run_recs(pend.ticket)[:, 0]
    else:
        r = eng.read_recs_after(pend.recs, pend.done)[:, 0]
    if emu.refractory_period_s > 0:  # emulator.py:830 on the frames just run: how often was the rule active?
        m = np.maximum(r["max_events"], 1)
        emu._refr_mostly_on = bool(np.mean(emu.refractory_period_s > pend.dts / m) > 0.05)
    # the device state has already advanced past the failed run: the instance refuses further frames until reset()
    err = None
    if (r["flags"] & _capi.FLAG_ITERS_CLAMPED).any():
        err = ("a pixel produced more than max_iters=%d events in one frame; construct with a larger max_iters"
               % eng.max_iters)
    elif (r["flags"] & _capi.FLAG_SYNC_TIMEOUT).any():
        err = ("in-kernel workgroup rendezvous of a redo pass timed out (GPU shared with another process?); "
               "use_graph | 128 runs one frame per launch, which needs none")
    elif (r["flags"] & _capi.FLAG_EVENTS_DROPPED).any():
        err = "event buffer capacity %d exceeded (needed %d); pass a larger cap" % (
            pend.ev.shape[1], int(r["n_events"].sum()))
    if err is not None:
        emu._failed = err
        raise _capi.V2EAmdError(err + " -- the pixel state is past this run: call reset() before feeding more frames")
    pend.counts[pend.start:] = r["n_events"]
    pend.rec_host = r
    pend.n_signal = np.zeros(len(pend.counts), dtype=np.int64)
    pend.n_signal[pend.start:] = r["n_signal"]
    emu.last_n_signal = pend.n_signal
    if pend.cs_steps_dev is not None:
        emu.cs_steps_taken.extend(int(v) for v in pend.cs_steps_dev.cpu().tolist())  # emulator.py:1124
    total = int(r["n_events"].sum())
    emu.num_events_total += total
    emu.num_events_on += int(r["n_on"].sum())
    emu.num_events_off += int(r["n_off"].sum())
    if pend.probe_dev is not None:
        _collect_probes(pend)
    out = pend.ev[0, :total]
    host = None if pend.return_device or total == 0 else out.cpu().numpy()
    if held and held[0] is pend:
        held.pop(0)
        event_files.write_run(emu, pend.frame0, r, out, host)
    if pend.return_device:
        return out, pend.counts
    return host, pend.counts


def _collect_probes(pend):
    """The block a probed run left on the device (v2e_emu_set_probes): the recorder's pixel, if it was on, is probe 0 and goes to
    single_pixel_states as the per-frame path would have put it there; the caller's pixels to pend.probes."""
    emu = pend.emu
    blk = emu._engine.read_after(pend.probe_dev, pend.done)  # [F_run][probes][PROBE_FIELDS]
    pend.probe_dev = None
    times = np.asarray(pend.times, dtype=np.float64)
    pos, neg = pend.thres
    first = 1 if pend.probe_rec else 0
    if pend.probe_rec and emu.record_single_pixel_states is not None:
        emu.single_pixel_sample_count, stop = model_states.append_pixel_states(
            emu.single_pixel_states, emu.single_pixel_sample_count, emu.SINGLE_PIXEL_MAX_SAMPLES, times, blk[:, 0, :], pos, neg)
        if stop:  # emulator.py:1007-1009
            model_states.end_recording(emu)
    if blk.shape[1] > first:
        user = blk[:, first:, :]
        d = {"time": np.repeat(times[:, None], user.shape[1], axis=1)}
        for i, name in enumerate(_capi.PROBE_FIELD_NAMES):
            d[name] = np.ascontiguousarray(user[:, :, i])
        if pos is not None:
            d["pos_thres"][:] = pos
        if neg is not None:
            d["neg_thres"][:] = neg
        pend.probes = d
