#!/usr/bin/env python
"""Golden DVS video of the reference's EventRenderer over a whole run (v2ecore/renderer.py:161-400, imported from the reference
tree with ref_harness' stubs; numba's @jit is an identity stub, cv2 a stub whose video writer swallows the frames): the events
of the first 120 frames of philox_moving_dot_64x64.npz (100 us frames, five of them without events) fed to
render_events_to_frames by v2e.py's own loop (v2e.py:829-850, written out below), with `output_path` and `dvs_vid` set so that
the class opens and writes its real `-frame_times.txt`.

  render_run.npz   counts                per-frame event counts of the 120 frames
                   rows                  their events, concatenated ([N,4] float32)
    per case `<mode>_<value>_b<batch>_<h>x<w>`:
                   ..._packets           [P,2] row range of every packet the loop rendered, the leftover one last
                   ..._p<k>              frames render_events_to_frames returned for packet k ([n,h,w] float64 in 0..1; absent: None)
                   ..._cur               the accumulator left behind (absent: None)
                   ..._times             the time `t` of every frame written, exactly as the class held it (float64 of it)
                   ..._txt               the bytes of the frame-times file

Cases: every exposure mode (two DURATION values: at 1 ms some packets of batch 8 complete no frame), batch sizes 8 and 5, and
32x32 output at batch 8 (not AREA_COUNT: the reference indexes its area counters out of bounds when down-scaled).  The numbers
carry the arithmetic of the numpy this was generated with (float32 `currentFrameStartTime` under numpy >= 2).
"""
import glob
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

N_FRAMES = 120
VIDEO = "dvs-video.avi"
CASES = [("duration", 300e-6, None), ("duration", 1e-3, None), ("count", 50, None), ("source", None, None), ("area_count", 6, 16)]
BATCHES = [8, 5]
FULL, SMALL = (64, 64), (32, 32)


class TimesTap:
    """The frame-times file, with the value `t` of every line taken from the writing frame before it is formatted."""

    def __init__(self, f):
        self.f, self.times = f, []

    def write(self, s):
        caller = sys._getframe(1)
        if caller.f_code.co_name == "render_events_to_frames":
            self.times.append(float(caller.f_locals["t"]))
        return self.f.write(s)

    def close(self):
        self.f.close()


def case_key(mode, val, bs, h, w):
    return "%s_%s_b%d_%dx%d" % (mode, "none" if val is None else ("%g" % val).replace(".", "p").replace("-", "m"), bs, h, w)


def main():
    rh.install_stubs()
    from v2ecore.renderer import EventRenderer, ExposureMode
    modes = {"duration": ExposureMode.DURATION, "count": ExposureMode.COUNT, "source": ExposureMode.SOURCE,
             "area_count": ExposureMode.AREA_COUNT}
    z = np.load(os.path.join(HERE, "philox_moving_dot_64x64.npz"))
    evs = [np.asarray(z["ev_%04d" % i], dtype=np.float32).reshape(-1, 4) for i in range(N_FRAMES)]
    counts = np.array([len(e) for e in evs], dtype=np.int64)
    out = {"counts": counts, "rows": np.concatenate(evs)}
    for mode, val, area in CASES:
        for bs, (h, w) in [(b, FULL) for b in BATCHES] + [(BATCHES[0], SMALL)]:
            if mode == "area_count" and (h, w) != FULL:
                continue
            key = case_key(mode, val, bs, h, w)
            with tempfile.TemporaryDirectory() as tmp:
                r = EventRenderer(full_scale_count=3, output_path=tmp, dvs_vid=VIDEO, exposure_mode=modes[mode],
                                  exposure_value=val if val is not None else 1 / 300.0, area_dimension=area)
                r.width, r.height = w, h
                r._check_outputs_open()
                tap = r.frame_times_output_file = TimesTap(r.frame_times_output_file)
                packets, nfr, row = [], 0, 0

                def render(events):
                    nonlocal nfr
                    fr = r.render_events_to_frames(events, height=h, width=w, return_frames=True)
                    if fr is not None:
                        out[key + "_p%d" % len(packets)] = fr
                        nfr += len(fr)
                    packets.append((row - len(events), row))

                # v2e.py:829-850
                events = np.zeros((0, 4), dtype=np.float32)
                for i in range(N_FRAMES):
                    newEvents = evs[i]
                    if newEvents is not None and newEvents.shape[0] > 0:
                        events = np.append(events, newEvents, axis=0)
                        events = np.array(events)
                        row += len(newEvents)
                        if i % bs == 0:
                            render(events)
                            events = np.zeros((0, 4), dtype=np.float32)
                if len(events) > 0:
                    render(events)
                r.cleanup()
                (fn,) = glob.glob(os.path.join(tmp, "*frame_times.txt"))
                txt = open(fn, "rb").read()
            assert nfr == len(tap.times) == r.numFramesWritten and nfr >= 10, (key, nfr)
            out[key + "_packets"] = np.array(packets, dtype=np.int64)
            out[key + "_times"] = np.array(tap.times, dtype=np.float64)
            out[key + "_txt"] = np.frombuffer(txt, dtype=np.uint8)
            if r.currentFrame is not None:
                out[key + "_cur"] = r.currentFrame
            per = [len(out[key + "_p%d" % k]) if key + "_p%d" % k in out else 0 for k in range(len(packets))]
            print("%-32s packets %2d (%d-%d events)  frames %3d  packets without a frame %d" % (
                key, len(packets), min(b - a for a, b in packets), max(b - a for a, b in packets), nfr, sum(p == 0 for p in per)))
    path = os.path.join(HERE, "render_run.npz")
    np.savez_compressed(path, **out)
    print("render_run.npz", os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
