"""The research tooling of `EventEmulator`: looking at the pixel model's state, not computing it.

  * `show_dvs_model_state` / `save_dvs_model_state` (emulator.py:580-617, 756-767): the named state planes are read back after
    every frame and displayed / appended to <name>.avi through cv2 where it is importable (`show_states`); nothing else in the
    package knows cv2.
  * `record_single_pixel_states` (emulator.py:279-300, 985-1009): ten series of one pixel, one sample per frame, pickled when the
    series are full or at cleanup().  The reference's rule is stated once, in `append_pixel_states`; the per-frame path
    (`record_pixel`) and the device-resident runs (v2e_amd/runs.py, from a probed run's block) both go through it.
  * `probe_pixel_indices`: the pixels of `probe_pixels=` as v2e_emu_set_probes takes them.

The functions take the emulator: the state they keep is the reference's public attributes (`single_pixel_states`,
`single_pixel_sample_count`, `record_single_pixel_states`, `show_list`, `dont_show_list`, `video_writers`), declared in its
constructor.
"""
import logging
import os
import pickle

import numpy as np
import torch

from . import _capi

logger = logging.getLogger("v2e_amd.emulator")  # the emulator's modules log under its name, as before they were split

PIXEL_STATE_SERIES = ("time",) + _capi.PROBE_FIELD_NAMES  # the reference's ten series, in its order (emulator.py:287-294)


def probe_pixel_indices(pixels, H, W, most=_capi.PROBE_MAX):
    """[(a, b), ...] -- addressed as the reference's plane[a, b], row then column, like record_single_pixel_states -- as the
    indices a * W + b v2e_emu_set_probes takes.  ValueError for more than `most` pixels, for anything that is not a pair of
    integers and for a pixel outside the H x W array (no negative indices: an event row never carries one)."""
    pixels = list(pixels)
    if len(pixels) > most:
        raise ValueError("at most %d pixels can be probed in one run, got %d" % (most, len(pixels)))
    out = []
    for px in pixels:
        try:
            a, b = px
            a, b = int(a.__index__()), int(b.__index__())
        except (TypeError, ValueError, AttributeError):
            raise ValueError("a probed pixel is a pair of integers (row, column), got %r" % (px,))
        if not (0 <= a < H and 0 <= b < W):
            raise ValueError("probed pixel %r lies outside the %d x %d pixel array" % (px, H, W))
        out.append(a * W + b)
    return out


def append_pixel_states(states, count, max_samples, times, block, pos_thres=None, neg_thres=None):
    """What emulator.py:985-1009 does frame after frame, for the frames of one device-resident run (or the one frame of
    generate_events): `block` [F, PROBE_FIELDS] (one probe of v2e_emu_set_probes, the clip's very first frame not among them) and
    their frame times go to samples count, count + 1, ... of the ten series while there is room; pos_thres / neg_thres: the
    Python-float thresholds, recorded instead of the block's where the reference holds scalars (emulator.py:992-995).  Returns
    (new count, stop): stop when a frame came after the series were full -- where the reference saves the file and ends the
    recording."""
    F = len(times)
    n = max(0, min(F, max_samples - count))
    for k in range(count, count + n):
        if k % 250 == 0:
            logger.info(f'recorded {k} single pixel states')
    sl = slice(count, count + n)
    states['time'][sl] = np.asarray(times, dtype=np.float64)[:n]
    for i, name in enumerate(_capi.PROBE_FIELD_NAMES):
        states[name][sl] = block[:n, i]
    if pos_thres is not None:
        states['pos_thres'][sl] = pos_thres
    if neg_thres is not None:
        states['neg_thres'][sl] = neg_thres
    return count + n, F > n


def wants_states(emu):
    return emu.show_dvs_model_state is not None or emu.record_single_pixel_states is not None


def record_pixel(emu, new_frame, t_frame, events, n_signal):
    """emulator.py:985-1009 for one frame of generate_events, as a block of one frame for append_pixel_states.  The index tuple
    addresses the [H, W] planes as the reference's does (plane[a, b]); the final per-pixel ON / OFF counts are the frame's signal
    events at that pixel (what final_pos/neg_evts_frame hold)."""
    ij = emu.record_single_pixel_states
    on = off = 0
    if events is not None and n_signal > 0:
        sig = events[:n_signal]
        here = (sig[:, 2] == ij[0]) & (sig[:, 1] == ij[1])  # rows are [t, x = column, y = row, p]
        on = int(np.count_nonzero(here & (sig[:, 3] > 0)))
        off = int(np.count_nonzero(here & (sig[:, 3] < 0)))
    pos, neg = (t if type(t) is float else t[ij] for t in (emu.pos_thres, emu.neg_thres))  # emulator.py:992-995
    row = [new_frame[ij], emu.base_log_frame[ij], emu.lp_log_frame[ij], emu.log_new_frame[ij], pos, neg, emu.diff_frame[ij], off, on]
    emu.single_pixel_sample_count, stop = append_pixel_states(
        emu.single_pixel_states, emu.single_pixel_sample_count, emu.SINGLE_PIXEL_MAX_SAMPLES, [t_frame],
        np.array([[float(v) for v in row]]))  # (in _capi.PROBE_FIELD_NAMES' order)
    if stop:
        end_recording(emu)


def save_pixel_states(emu):  # emulator.py:431-437
    try:
        with open(emu.SINGLE_PIXEL_STATES_FILENAME, 'wb') as outfile:
            pickle.dump(emu.single_pixel_states, outfile, protocol=pickle.HIGHEST_PROTOCOL)
            logger.info(f'saved single pixel states with {emu.single_pixel_sample_count} samples to '
                        f'{emu.SINGLE_PIXEL_STATES_FILENAME}')
    except Exception as e:
        logger.error(f'could not save pickled pixel states, got {e}')


def end_recording(emu):
    """emulator.py:428-429, 1007-1009: the file is written and the recording is over."""
    emu.save_recorded_single_pixel_states()
    emu.record_single_pixel_states = None


def show_states(emu, new_frame, t_frame):
    """The attributes the reference holds at emulator.py:756 (after the leak, before the events), as device views; then
    emulator.py:756-767: show / save the requested ones."""
    eng = emu._engine
    sd = torch.float64 if eng.f64_state else torch.float32
    emu.new_frame = new_frame
    emu.log_new_frame = eng.plane(emu._state_planes[0]).to(torch.float32)  # lin_log returns float32 (emulator_utils.py:45)
    emu.c_minus_s_frame = eng.plane(emu._state_planes[1]).to(sd) if emu.csdvs_enabled else None
    emu.diff_frame = eng.plane(emu._state_planes[2]).to(sd)
    if emu.show_dvs_model_state is None:
        return
    cv2 = _host_cv2(emu)
    for s in emu.show_dvs_model_state:
        if s in emu.dont_show_list:
            continue
        f = getattr(emu, s, None)
        if f is None:
            logger.error(f'{s} does not exist so we cannot show it')
            emu.dont_show_list.append(s)
        elif cv2 is not None:
            _show(emu, f, s)
    if cv2 is not None:
        try:
            k = cv2.waitKey(30)
        except Exception:
            k = -1
        if k == 27 or k == ord('x'):
            raise SystemExit(0)  # v2e_quit()


def _host_cv2(emu):
    if emu._cv2 is None and not emu._show_warned:
        try:
            import cv2
            if not callable(getattr(cv2, "imshow", None)):
                raise ImportError("cv2 has no imshow")
            emu._cv2 = cv2
        except Exception as e:
            logger.warning("v2e_amd.EventEmulator: show_dvs_model_state / save_dvs_model_state need OpenCV on the host (%s): "
                           "nothing is displayed or saved; the state planes stay readable as attributes (%s)", e,
                           ", ".join(emu.show_dvs_model_state))
            emu._show_warned = True
    return emu._cv2


def _show(emu, inp, name):
    """emulator.py:580-617: normalise by MODEL_STATES[name], show, and append to <name>.avi with save_dvs_model_state."""
    cv2 = emu._cv2
    img = np.array(inp.detach().cpu().numpy() if torch.is_tensor(inp) else inp, dtype=np.float64)
    (lo, hi) = emu.MODEL_STATES[name]
    img = (img - lo) / (hi - lo)
    try:
        cv2.namedWindow(name, cv2.WINDOW_NORMAL)
        if name not in emu.show_list:
            emu.show_list.append(name)
            if emu.save_dvs_model_state:
                fn = os.path.join(emu.output_folder or "", name + '.avi')
                emu.video_writers[name] = cv2.VideoWriter(fn, cv2.VideoWriter_fourcc(*'XVID'), 30,
                                                          (int(emu.output_width or img.shape[1]),
                                                           int(emu.output_height or img.shape[0])))
        for org, col in (((0, img.shape[0]), (0, 0, 0)), ((1, img.shape[0] - 1), (255, 255, 255))):
            cv2.putText(img, f'fr:{emu.frame_counter} t:{emu.t_previous:.4f}s', org=org, fontScale=1.3, color=col,
                        fontFace=cv2.FONT_HERSHEY_PLAIN, thickness=1)
        cv2.imshow(name, img)
        if emu.save_dvs_model_state:
            g = (img * 255).astype(np.uint8)
            emu.video_writers[name].write(np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)))
    except Exception as e:  # no display
        logger.warning("v2e_amd.EventEmulator: cannot show %s (%s)", name, e)
        emu.dont_show_list.append(name)
