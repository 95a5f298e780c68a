"""Drop-in `EventEmulator` running the DVS pixel model on MI355X HIP kernels.

This module holds the class itself: the reference's constructor surface and every attribute of an instance (declared in
__init__, or in reset() where it is per clip), the parameter snapshot, the first frame, the per-frame path `generate_events`
(tape replay and the one-call Philox frame), the centre-surround host arithmetic, and the entry points of device-resident runs,
which validate their arguments and hand over to v2e_amd/runs.py.  The event files are v2e_amd/event_files.py, the research
tooling (cv2 display, single-pixel recorder, probes) v2e_amd/model_states.py.

Mirrors the public surface of the reference class (v2ecore/emulator.py:35-1059):
same constructor signature (:86-117), `generate_events(new_frame, t_frame)` (:619),
`set_dvs_params` (:513), `reset` (:558), `prepare_storage` (:374), `cleanup` (:402),
the counters `num_events_total/on/off`, `t_previous`, and the class attributes that
v2ecore/v2e_args.py:209,216 reads.

Random numbers come in two modes, selected with the extra keyword
`rng_mode` (or env V2E_AMD_RNG):
  "tape"   (default) the host issues exactly the reference's torch calls in the
           reference's order from torch's global CPU generator -- normal, normal, randn
           on the first frame; randn, one randperm per non-empty iteration, rand on every
           later frame, plus torch.linspace for the timestamps -- and hands the values to
           the kernels.  Event-for-event identical to the reference torch-CPU path under
           the same seed.
  "philox" counter-based Philox4x32-10 inside the kernels, timestamps and the
           per-iteration shuffle computed on device; no host round trip except the final
           copy of the event list.  `generate_events_batch` keeps a whole clip on device.

`show_dvs_model_state` / `save_dvs_model_state` (emulator.py:580-617, 756-764) and `record_single_pixel_states`
(emulator.py:279-300, 985-1009) are host pass-throughs in generate_events: the named state planes are read back from the device after
every frame (three of them -- log_new_frame, c_minus_s_frame, diff_frame -- are left in extra planes by k_count while one of the two
options is on, v2e_emu_set_model_state_planes) and displayed / saved through cv2 where it is importable, resp. recorded and pickled
as the reference does; both put generate_events on the step-wise kernels.  In generate_events_batch the recorder's pixel -- and up to
64 pixels of the caller's, `probe_pixels` -- is read on the device instead (v2e_emu_set_probes, csrc/probe.hip: nine float64 per
pixel and frame come back with the run's result; such a run takes the per-frame kernels, not k_chain).  `hdr=True`
(log-encoded input, emulator.py:304, 666), `photoreceptor_noise=True` (emulator.py:694-703), `scidvs=True` (float64 and float32
state: torch's float32 sinh is restated bit for bit in include/v2e_detmath.h)
and the centre-surround pixel (`cs_lambda_pixels`, emulator.py:1061-1124: the diffuser is stepped on the device between
frames, csrc/csdvs.hip; in generate_events_batch too: the stepping loop is enqueued whole with its stop rule on the device)
are supported.
"""
import atexit
import ctypes as C
import logging
import math
import os
import random
from typing import Optional

import weakref

import numpy as np
import torch

from . import _capi, event_files, model_states, runs
from ._capi import EmuParams, RNG_PHILOX, RNG_TAPE
from .engine import EmuEngine
from .model_states import PIXEL_STATE_SERIES, append_pixel_states, probe_pixel_indices  # noqa: F401 (importable from here, as ever)
from .runs import default_event_capacity  # noqa: F401

logger = logging.getLogger(__name__)


class _TorchTape:
    """The reference's own random draws, issued on the host (tape mode)."""

    def normal(self, mean, std, shape):
        return torch.normal(mean, std, size=shape, dtype=torch.float32)  # emulator.py:460-471

    def randn(self, shape):
        return torch.randn(shape, dtype=torch.float32)  # emulator.py:501, emulator_utils.py:122

    def rand(self, shape):
        return torch.rand(size=shape, dtype=torch.float32)  # emulator_utils.py:338

    def randperm(self, n, frame=None, it=None):
        return torch.randperm(n)  # emulator.py:868

    def linspace(self, start, end, n):
        return torch.linspace(start=start, end=end, steps=n, dtype=torch.float32)  # emulator.py:793

    def exp_noise_rate(self, cov, randn):
        return torch.exp(math.log(10) * cov * randn)  # emulator.py:504-505

    def exp_scidvs(self, draw):
        return torch.exp(draw)  # emulator.py:481-483


def photoreceptor_noise_vrms(shot_noise_rate_hz, f3db, sample_rate_hz, pos_thr, neg_thr, sigma_thr):
    """Gaussian RMS amplitude (ln units) to inject before the photoreceptor low-pass so that threshold crossings of
    the filtered noise occur at the requested event rate: the curve fit of Graca & Delbruck (2021) evaluated over
    sampled thresholds, then scaled by the noise-equivalent-bandwidth factor of this IIR measured on a white
    sequence (what emulator_utils.py:177-290 computes; like there, the draws are unseeded numpy ones)."""
    rate_per_bw = (shot_noise_rate_hz / f3db) / 2  # the fit is for ON events only
    x = math.log10(rate_per_bw)
    rng = np.random.default_rng()
    n = 300
    thr = np.minimum(pos_thr + sigma_thr * rng.standard_normal(n), neg_thr + sigma_thr * np.random.default_rng().standard_normal(n))
    y = -0.0026 * x ** 3 - 0.036 * x ** 2 - 0.1949 * x + 0.321  # log10(thr / vn)
    vn = float(np.mean(thr / 10 ** y))
    tau = 1 / (f3db * 2 * math.pi)
    dt = 1 / sample_rate_hz
    rin = vn * np.random.default_rng().standard_normal(np.arange(0, 1000 * tau, dt).shape)
    eps = dt / tau
    rout = np.zeros_like(rin)
    for i in range(1, len(rin)):
        rout[i] = rout[i - 1] * (1 - eps) + rin[i] * eps
    return float(np.std(rin) / np.std(rout) * vn)


_THREAD_OVERRIDE = {"users": 0, "prev": None}  # tape-mode emulators alive that rely on the one-thread setting


def _release_host_threads():
    """cleanup() of a tape-mode emulator: the previous thread count comes back when the LAST one that relies on it is gone."""
    o = _THREAD_OVERRIDE
    if o["users"] > 0:
        o["users"] -= 1
        if o["users"] == 0 and o["prev"] is not None:
            torch.set_num_threads(o["prev"])
            o["prev"] = None


def _limit_host_threads(n):
    """Tape mode issues a handful of small torch CPU ops per frame (randn / rand of one frame, a randperm per
    iteration).  Their values do not depend on the intra-op thread count, but on a many-core host fanning each of
    them out over the OpenMP pool costs milliseconds: 250 -> 1 170 frames/s on the MI355X box with one thread.
    The setting is process-global in torch, so it is applied once, when a tape-mode emulator is constructed
    (`tape_host_threads`, default 1; None leaves torch alone), said so in the log, and put back by cleanup().
    Returns the previous value (None if nothing was changed)."""
    if n is None:
        return None
    o = _THREAD_OVERRIDE
    if o["users"] > 0 or torch.get_num_threads() == int(n):  # already in force (or nothing to change): just count this user
        o["users"] += 1
        return True
    prev = torch.get_num_threads()
    o["users"], o["prev"] = 1, prev
    logger.warning("v2e_amd.EventEmulator (tape mode): torch.set_num_threads(%d) for this process (was %d; restored by "
                   "cleanup(); pass tape_host_threads=None to leave torch alone)", int(n), prev)
    torch.set_num_threads(int(n))
    return prev


def _as_f32_tensor(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _cleanup_at_exit(ref):
    emu = ref()
    if emu is not None:
        emu.cleanup()


class EventEmulator(object):
    """compute events based on the input frame (MI355X implementation)."""

    # class attributes read by v2ecore/v2e_args.py (emulator.py:41-56)
    l255 = np.log(255)
    gr = (0, 255)
    lg = (0, l255)
    slg = (-l255 / 8, l255 / 8)
    MODEL_STATES = {'new_frame': gr, 'log_new_frame': lg, 'lp_log_frame': lg, 'scidvs_highpass': slg,
                    'photoreceptor_noise_arr': slg, 'cs_surround_frame': lg, 'c_minus_s_frame': slg,
                    'base_log_frame': slg, 'diff_frame': slg}
    MAX_CHANGE_TO_TERMINATE_EULER_SURROUND_STEPPING = 1e-5  # emulator.py:52
    SINGLE_PIXEL_STATES_FILENAME = 'pixel-states.dat'
    SINGLE_PIXEL_MAX_SAMPLES = 10000
    SCIDVS_GAIN = 2
    SCIDVS_TAU_S = .01
    SCIDVS_TAU_COV = 0.5

    def __init__(
            self,
            pos_thres: float = 0.2,
            neg_thres: float = 0.2,
            sigma_thres: float = 0.03,
            cutoff_hz: float = 0.0,
            leak_rate_hz: float = 0.1,
            refractory_period_s: float = 0.0,
            shot_noise_rate_hz: float = 0.0,
            photoreceptor_noise: bool = False,
            leak_jitter_fraction: float = 0.1,
            noise_rate_cov_decades: float = 0.1,
            seed: int = 0,
            output_folder: str = None,
            dvs_h5: str = None,
            dvs_aedat2: str = None,
            dvs_aedat4: str = None,
            dvs_text: str = None,
            show_dvs_model_state: str = None,
            save_dvs_model_state: bool = False,
            output_width: int = None,
            output_height: int = None,
            device: str = "cuda",
            cs_lambda_pixels: float = None,
            cs_tau_p_ms: float = None,
            hdr: bool = False,
            scidvs: bool = False,
            record_single_pixel_states=None,
            label_signal_noise=False,
            *,
            rng_mode: Optional[str] = None,
            shuffle: bool = True,
            tape=None,
            max_iters: int = 64,
            photoreceptor_noise_vrms: Optional[float] = None,
            tape_host_threads: Optional[int] = 1,
    ):
        # what cleanup() reads, declared before anything below can raise: __del__ runs it on a half-built instance too
        self.cs_steps_taken = []  # CSDVS (emulator.py:245-272): Euler steps each frame took; cleanup() reports and empties it
        self._host_threads_prev = None  # what _limit_host_threads returned: not None while this instance counts as its user
        self.video_writers = {}  # save_dvs_model_state: cv2.VideoWriter per shown state
        self._sink_runs = []  # device-resident runs not yet in the event files / the recorder's series, oldest first (runs.py)
        self.record_single_pixel_states = None  # the recorded pixel; None once the recording has ended
        # event file writers are outside the hot path (emulator.py:312-346; event_files.py); None: closed
        self.dvs_h5 = self.dvs_aedat2 = self.dvs_aedat4 = self.dvs_text = None
        self.dvs_h5_dataset = self.frame_h5_dataset = self.frame_ts_dataset = self.frame_ev_idx_dataset = None
        self._h5_stream = None  # side stream the HDF5 rows of device-resident runs are packed on

        # research tooling (host pass-throughs, model_states.py)
        self.dont_show_list = []
        self.show_list = []
        self._state_planes = None  # three float64 planes k_count fills while states are shown or recorded
        self._cv2 = None
        self._show_warned = False
        if show_dvs_model_state is not None and len(show_dvs_model_state) == 1 and show_dvs_model_state[0] == 'all':
            logger.info(f'will show all model states that exist from {EventEmulator.MODEL_STATES.keys()}')  # emulator.py:365-368
            show_dvs_model_state = list(EventEmulator.MODEL_STATES.keys())
        if record_single_pixel_states is not None:  # emulator.py:279-300; checked before it is kept: cleanup() pickles for whatever is
            if not (type(record_single_pixel_states) is tuple):
                raise ValueError(f'--record_single_pixel_states {record_single_pixel_states} should be a tuple, e.g. (10,20)')
            if len(record_single_pixel_states) != 2:
                raise ValueError(f'--record_single_pixel_states {record_single_pixel_states} should have two pixel addresses (x,y)')
            for i in record_single_pixel_states:
                if not (type(i) is int):
                    raise ValueError(f'--record_single_pixel_states {record_single_pixel_states} should have two '
                                     f'integer-value pixel addresses (x,y)')
        self.record_single_pixel_states = record_single_pixel_states
        self.single_pixel_sample_count = 0
        self.single_pixel_states = None if self.record_single_pixel_states is None else {
            k: np.full(self.SINGLE_PIXEL_MAX_SAMPLES, np.nan) for k in PIXEL_STATE_SERIES}
        self.last_probes = None  # generate_events_batch(probe_pixels=...): the series of the last such call
        self.last_n_signal = None  # the last finished device-resident run's signal rows per frame (PendingRun.n_signal, runs.py)

        # device-resident runs (runs.py); what is per clip is in reset()
        self._async_flip = 0  # the buffer set (0 / 1) the next asynchronous run writes
        self._blocking_lengths = {}  # run length -> blocking calls seen: the hipGraph is built from the second on
        self._refr_mostly_on = False  # the refractory rule was active in most frames of the last run read

        self.no_events_warning_count = 0
        logger.info("ON/OFF log_e temporal contrast thresholds: {} / {} +/- {}".format(
            pos_thres, neg_thres, sigma_thres))
        self.reset()
        self.t_previous = 0
        self.device = device

        self.sigma_thres = sigma_thres
        self.pos_thres = pos_thres
        self.neg_thres = neg_thres
        self.pos_thres_nominal = pos_thres
        self.neg_thres_nominal = neg_thres
        self.cutoff_hz = cutoff_hz
        self.leak_rate_hz = leak_rate_hz
        self.refractory_period_s = refractory_period_s
        self.shot_noise_rate_hz = shot_noise_rate_hz
        self.photoreceptor_noise = bool(photoreceptor_noise)
        self.photoreceptor_noise_vrms = photoreceptor_noise_vrms  # None: computed like emulator_utils.py:177-290
        self._pn_vrms = 0.0  # the amplitude in force (_prepare_pnoise)
        self._pn_plane = None  # photoreceptor_noise_arr's padded device plane, from the first noisy frame on
        if self.photoreceptor_noise and (shot_noise_rate_hz == 0 or cutoff_hz == 0):  # emulator.py:196-204 (v2e_quit)
            logger.error('--photoreceptor_noise needs a finite --shot_noise_rate_hz and --cutoff_hz')
            raise SystemExit(1)
        self.leak_jitter_fraction = leak_jitter_fraction
        self.noise_rate_cov_decades = noise_rate_cov_decades
        self.SHOT_NOISE_INTEN_FACTOR = 0.25
        self.output_folder = output_folder
        self.output_width = output_width
        self.output_height = output_height
        self.show_dvs_model_state = show_dvs_model_state
        self.save_dvs_model_state = save_dvs_model_state
        self.label_signal_noise = label_signal_noise
        self.log_input = bool(hdr)  # emulator.py:304: frames are log-encoded already
        self.scidvs = bool(scidvs)  # emulator.py:307-309: nonlinear CR high-pass amplified log intensity
        self._sc_planes = self._sc_tau = None  # the padded device planes behind scidvs_highpass, scidvs_previous_photo, scidvs_tau_arr
        # CSDVS (emulator.py:245-272)
        self.cs_steps_warning_printed = False
        self.cs_alpha_warning_printed = False
        self.cs_tau_p_ms = cs_tau_p_ms
        self.cs_lambda_pixels = cs_lambda_pixels
        self._cs_planes = None  # [surround, ping-pong scratch, the coming frame's lp_log_frame], from the first frame on
        self.csdvs_enabled = cs_lambda_pixels is not None
        if self.csdvs_enabled:
            self.cs_tau_h_ms = 0 if (cs_tau_p_ms is None or cs_tau_p_ms == 0) else cs_tau_p_ms / (cs_lambda_pixels ** 2)
            logger.info(f'Center-surround parameters:\n\tcs_tau_p_ms: {self.cs_tau_p_ms}\n\tcs_tau_h_ms:  {self.cs_tau_h_ms}\n\t'
                        f'cs_lambda_pixels:  {self.cs_lambda_pixels:.2f}\n\t')
        self.seed = seed

        self.rng_mode = (rng_mode or os.environ.get("V2E_AMD_RNG", "tape")).lower()
        if self.rng_mode not in ("tape", "philox"):
            raise ValueError("rng_mode must be 'tape' or 'philox', got %r" % (self.rng_mode,))
        self.shuffle = bool(shuffle)
        self._tape = tape if tape is not None else _TorchTape()
        if self.rng_mode == "tape":
            self._host_threads_prev = _limit_host_threads(tape_host_threads)
        self._max_iters = max_iters
        if seed != 0:  # emulator.py:221-224
            torch.manual_seed(seed)
            # numpy takes 32 bits.  Philox mode keys its streams with all 64 bits of the seed (P.seed), so there a larger seed is
            # valid and numpy gets its low word; tape mode raises ValueError like the reference
            np.random.seed(seed if self.rng_mode == "tape" else seed & 0xFFFFFFFF)
            random.seed(seed)

        event_files.open_sinks(self, dvs_h5, dvs_aedat2, dvs_aedat4, dvs_text)

        self._engine: Optional[EmuEngine] = None
        self._thres_scalar = None  # (pos, neg) as Python floats, as they were when the first frame drew the planes
        self._thres_is_scalar = False  # ... and whether they stayed scalars (sigma_thres == 0)
        self._idx_pin = self._idx_dev = None  # tape mode: pinned / device staging of a frame's shuffle indices
        # emulator.py:296 registers cleanup with atexit.  Through a weak reference here: a bound method would keep every emulator -- and
        # the gigabytes of device scratch a 1280x720 one holds -- alive until the process ends; one that is dropped is cleaned up then
        # (__del__), one that is still alive at exit by the hook
        atexit.register(_cleanup_at_exit, weakref.ref(self))

    # ------------------------------------------------------------- plumbing
    def prepare_storage(self, n_frames, frame_ts):  # emulator.py:374-400
        event_files.prepare_storage(self, n_frames, frame_ts)

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass

    def cleanup(self):  # emulator.py:402-429
        """Order: the held device-resident runs are finished and written (event files, recorder series, their CSDVS steps); the
        CSDVS statistics line; the thread override; the AVI writers; the recorder's pickle; the event files.  The held runs come
        first -- before the statistics line, where the reference has no such step -- because a run's Euler steps reach
        cs_steps_taken only when its result is read: logged first, the line would miss them.  Everything it closes it also forgets
        (cs_steps_taken is emptied once reported, the thread override, the writers, the recorder, the sinks), so a second call --
        the atexit hook or __del__ after the caller's own -- finds nothing to do: no second statistics line, no file touched."""
        # every run enqueued while the sinks were open (or the recorder on) reaches them before they close -- and first of all, so
        # that the statistics below include the Euler steps of the runs read here
        runs.write_held(self)
        if len(self.cs_steps_taken) > 1:
            logger.info(f'CSDVS steps statistics: mean+std= {np.mean(self.cs_steps_taken):.0f} + {np.std(self.cs_steps_taken):.0f} '
                        f'(median= {np.median(self.cs_steps_taken):.0f})')
            self.cs_steps_taken = []
        if self._host_threads_prev is not None:
            _release_host_threads()
            self._host_threads_prev = None
        for name, vw in list(self.video_writers.items()):  # emulator.py:424-426
            logger.info(f'closing video AVI {name}')
            try:
                vw.release()
            except Exception:
                pass
        self.video_writers = {}
        if self.record_single_pixel_states is not None:  # emulator.py:428-429
            model_states.end_recording(self)
        event_files.close(self)

    DVS_PARAMS = {  # emulator.py:513-556
        'clean': dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.02, cutoff_hz=0, leak_rate_hz=0, leak_jitter_fraction=0,
                      noise_rate_cov_decades=0, shot_noise_rate_hz=0, refractory_period_s=0),
        'noisy': dict(pos_thres=0.2, neg_thres=0.2, sigma_thres=0.05, cutoff_hz=30, leak_rate_hz=0.1, shot_noise_rate_hz=5.0,
                      refractory_period_s=0, leak_jitter_fraction=0.1, noise_rate_cov_decades=0.1)}

    def set_dvs_params(self, model: str):
        if model not in self.DVS_PARAMS:
            logger.warning("dvs_params {} not known: Using commandline assigned options".format(model))
        for name, value in self.DVS_PARAMS.get(model, {}).items():
            setattr(self, name, value)

    def reset(self):  # emulator.py:558-578
        runs.write_held(self)  # runs still held for the open sinks are written first (dropped if a run failed)
        self._failed = None  # the error text of a device-resident run that failed: the instance refuses frames until the next reset()
        # buffer set -> weakref of the run that last used it; handles of runs enqueued before the reset are no longer collected on
        # the caller's behalf
        self._async_slots = {}
        # buffer set -> the device frames of the run that last used it (kept across a reset: such a run may still be executing)
        self._run_frames = getattr(self, "_run_frames", {})
        self.num_events_total = 0
        self.num_events_on = 0
        self.num_events_off = 0
        self.new_frame = None
        self.log_new_frame = None
        self.lp_log_frame = None
        self.base_log_frame = None
        self.diff_frame = None
        self.c_minus_s_frame = None
        self.frame_counter = 0
        self.timestamp_mem = None
        self.noise_rate_array = None
        self.photoreceptor_noise_arr = None
        self.scidvs_highpass = self.scidvs_previous_photo = self.scidvs_tau_arr = None
        self.cs_surround_frame = None
        self._pn_last_rate = None  # the noise amplitude is recomputed for the first frame pair of the next clip
        self._initialized = False

    # ------------------------------------------------------------- parameters
    def _raise_if_failed(self, why=""):
        if self._failed:
            raise _capi.V2EAmdError("a previous device-resident run failed (%s); %scall reset()" % (self._failed, why))

    def _params(self) -> EmuParams:
        """Snapshot the (mutable) attributes into the C struct, every call."""
        P = EmuParams()
        # the state planes are float64 iff the reference's are: with the low-pass on, or log-encoded input.  (The one statement of
        # the rule: the first frame allocates by P.f64_state, later ones compare it with the engine's.)
        P.f64_state = 1 if (self.cutoff_hz > 0 or self.log_input) else 0
        P.log_input = 1 if self.log_input else 0
        P.scalar_thres = 1 if self._thres_scalar is not None and self._thres_is_scalar else 0
        P.rng_mode = RNG_PHILOX if self.rng_mode == "philox" else RNG_TAPE
        P.shuffle = 1 if self.shuffle else 0
        P.pos_thres_nominal = float(self.pos_thres_nominal)
        P.neg_thres_nominal = float(self.neg_thres_nominal)
        P.pos_thres_scalar, P.neg_thres_scalar = self._thres_scalar
        P.sigma_thres = float(self.sigma_thres)
        P.cutoff_hz = float(self.cutoff_hz)
        P.leak_rate_hz = float(self.leak_rate_hz)
        P.leak_jitter_fraction = float(self.leak_jitter_fraction)
        P.noise_rate_cov_decades = float(self.noise_rate_cov_decades)
        P.refractory_period_s = float(self.refractory_period_s)
        # photoreceptor noise replaces the shot-event generator and its base reset (emulator.py:893, 940)
        P.shot_noise_rate_hz = 0.0 if self.photoreceptor_noise else float(self.shot_noise_rate_hz)
        P.photoreceptor_noise = 1 if self.photoreceptor_noise else 0
        P.photoreceptor_noise_vrms = float(self._pn_vrms)
        P.shot_noise_inten_factor = float(self.SHOT_NOISE_INTEN_FACTOR)
        if P.scalar_thres:  # emulator.py:475-478 with Python-float thresholds
            P.pos_pre_scalar = float(torch.div(self.pos_thres_nominal, P.pos_thres_scalar))
            P.neg_pre_scalar = float(torch.div(self.neg_thres_nominal, P.neg_thres_scalar))
        P.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return P

    def _ensure_engine(self, H, W):
        if self._engine is not None and (self._engine.H, self._engine.W) != (H, W):
            if self._initialized:
                raise ValueError("frame shape changed from %dx%d to %dx%d after the first frame; call reset() first" % (
                    self._engine.H, self._engine.W, H, W))
            self._engine = None
        if self._engine is None:
            self._engine = EmuEngine(H, W, n_clips=1, device=self.device, max_iters=self._max_iters)
        return self._engine

    # ------------------------------------------------------------- first frame
    def _first_frame(self, frame_dev, H, W, t_frame):
        """emulator.py:681-717 + _init :439-511."""
        eng = self._ensure_engine(H, W)
        # thresholds are scalars (Python floats) until _init draws them; remember the
        # values current at this moment (set_dvs_params may have changed them)
        if torch.is_tensor(self.pos_thres) or torch.is_tensor(self.neg_thres):
            # re-initialisation after reset(): the per-pixel planes of the previous run are dropped and
            # new ones are drawn around the same scalar thresholds (the reference's reset() leaves the old
            # tensors in place, which its own _init cannot consume)
            prev = self._thres_scalar or (float(self.pos_thres_nominal), float(self.neg_thres_nominal))
            self.pos_thres, self.neg_thres = prev
        self._thres_scalar = (float(self.pos_thres), float(self.neg_thres))
        self._thres_is_scalar = not (self.sigma_thres > 0)
        P = self._params()
        eng.alloc_state(bool(P.f64_state))
        tp = tn = nr = None
        sc_tau_host = None
        if self.scidvs:  # two more state planes + per-pixel time constants (emulator.py:480-483, 719-722)
            sd = torch.float64 if eng.f64_state else torch.float32  # zeros_like(lp_log_frame)
            self._sc_planes = [torch.zeros((1, eng.npx_pad), dtype=sd, device=eng.device) for _ in range(2)]
            self._sc_tau = torch.zeros((1, eng.npx_pad), dtype=torch.float32, device=eng.device)
            _capi.check(eng.lib.v2e_emu_set_scidvs(eng._h, self._sc_planes[0].data_ptr(), self._sc_planes[1].data_ptr(),
                                                   self._sc_tau.data_ptr(), int(self.frame_counter)), "v2e_emu_set_scidvs")
        if self.rng_mode == "tape":
            dev = eng.device
            if self.sigma_thres > 0:
                tp = _as_f32_tensor(self._tape.normal(self.pos_thres, self.sigma_thres, (H, W))).to(dev)
                tn = _as_f32_tensor(self._tape.normal(self.neg_thres, self.sigma_thres, (H, W))).to(dev)
            if self.scidvs and self.SCIDVS_TAU_COV > 0:  # drawn between the thresholds and the noise rates
                d = _as_f32_tensor(self._tape.normal(0, self.SCIDVS_TAU_COV, (H, W)))
                sc_tau_host = self.SCIDVS_TAU_S * _as_f32_tensor(self._tape.exp_scidvs(d))
            if self.leak_rate_hz > 0:
                r = _as_f32_tensor(self._tape.randn((H, W)))
                nr = _as_f32_tensor(self._tape.exp_noise_rate(self.noise_rate_cov_decades, r)).to(dev)
        eng.init_state(P, frame_dev, t_frame, tp, tn, nr)
        if self.scidvs:
            if sc_tau_host is not None:
                self._sc_tau[0, :H * W] = sc_tau_host.reshape(-1).to(eng.device)
            self.scidvs_highpass = eng.plane(self._sc_planes[0])
            self.scidvs_previous_photo = eng.plane(self._sc_planes[1])
            self.scidvs_tau_arr = eng.plane(self._sc_tau)
        if self.csdvs_enabled:
            # emulator.py:1062-1063 and :715: the surround starts as a copy of lp_log_frame, so base_log_frame =
            # lp_log_frame - cs_surround_frame is zero; [surround, ping-pong scratch, the coming frame's lp_log_frame]
            self._cs_planes = [eng.lp.clone(), torch.empty_like(eng.lp), torch.empty_like(eng.lp)]
            eng.base.zero_()
            eng.set_csdvs(self._cs_planes[0])
            self.cs_surround_frame = eng.plane(self._cs_planes[0])
        else:
            eng.set_csdvs(None)
        self._state_planes = None
        if model_states.wants_states(self):
            self._state_planes = [torch.zeros((1, eng.npx_pad), dtype=torch.float64, device=eng.device) for _ in range(3)]
        eng.set_model_state_planes(self._state_planes)
        # public state attributes, as [H,W] device views
        self.lp_log_frame = eng.plane(eng.lp)
        self.base_log_frame = eng.plane(eng.base)
        if self.sigma_thres > 0:
            self.pos_thres = eng.plane(eng.pos_thres)
            self.neg_thres = eng.plane(eng.neg_thres)
        if self.leak_rate_hz > 0:
            self.noise_rate_array = eng.plane(eng.noise_rate)
        if self.refractory_period_s > 0:
            self.timestamp_mem = eng.plane(eng.ts_mem)
        self._initialized = True

    # ------------------------------------------------------------- hot path
    def generate_events(self, new_frame, t_frame):
        """Compute events in new frame (emulator.py:619-1022).

        new_frame: np.ndarray or torch tensor [height, width]; t_frame: seconds.
        Returns np.ndarray [N,4] float32 rows [t, x, y, p(+1/-1)] or None.
        """
        self._raise_if_failed()
        if self.frame_h5_dataset is not None:
            fr = new_frame.detach().cpu().numpy() if torch.is_tensor(new_frame) else np.asarray(new_frame)
            self.frame_h5_dataset[self.frame_counter] = fr.astype(np.uint8)
        self.frame_counter += 1
        if t_frame < self.t_previous:
            raise ValueError("this frame time={} must be later than previous frame time={}".format(
                t_frame, self.t_previous))
        shape = tuple(new_frame.shape)
        if len(shape) != 2:
            raise ValueError("new_frame must be [height, width], got shape %r" % (shape,))
        H, W = shape
        eng = self._ensure_engine(H, W)
        # Philox mode after the first frame: the whole frame is ONE C call (v2e_emu_frame), the host frame goes through
        # the handle's pinned staging instead of a torch tensor
        fast = self._initialized and self.rng_mode == "philox" and not self.photoreceptor_noise and not self.csdvs_enabled \
            and not model_states.wants_states(self)
        host_frame = None
        if fast and isinstance(new_frame, np.ndarray) and new_frame.dtype in (np.uint8, np.float32, np.float64):
            host_frame = np.ascontiguousarray(new_frame)
        frame_dev = None if host_frame is not None else eng.to_device_frame(new_frame)

        if not self._initialized:
            self._first_frame(frame_dev, H, W, float(t_frame))
            return None  # t_previous intentionally not advanced (emulator.py:717)

        t_prev = float(self.t_previous)
        t_frame = float(t_frame)
        fidx = self.frame_counter - 1
        P = self._params()
        if bool(P.f64_state) != eng.f64_state:
            raise ValueError("cutoff_hz changed sign after the first frame: the state dtype "
                             "(float64 iff cutoff_hz > 0 or hdr) is fixed by the first frame")
        tape = self.rng_mode == "tape"
        dev = eng.device

        counted = False
        if fast:
            ev = eng.event_buffer(max(4 * H * W, 1 << 16))
            rc, out8, events = eng.frame(P, host_frame if host_frame is not None else frame_dev, t_prev, t_frame, fidx, ev)
            n_events, n_on, n_off, n_signal, M = (int(out8[k]) for k in range(5))
            if rc == 0:
                return self._frame_done(new_frame, t_frame, M, n_events, n_on, n_off, n_signal, events, ev)
            # rc 1: more iterations than the scratch holds; rc 2: more rows than the buffer: the frame is counted, the general
            # path below grows what is needed and finishes it
            counted = True
            if frame_dev is None:
                frame_dev = eng.to_device_frame(new_frame)

        if self.photoreceptor_noise:  # emulator.py:694-703
            self._prepare_pnoise(eng, [1.0 / (t_frame - t_prev)])
            P = self._params()
            # the tape's draw comes before the leak draw, as in the reference; set_pnoise keeps its address for count(): the tensor
            # has to live until then
            pn_draw = _as_f32_tensor(self._tape.randn((H, W))).to(dev) if tape else None
            eng.set_pnoise(self._pn_plane, pn_draw)
        leak = None
        if tape and self.leak_rate_hz > 0:
            leak = _as_f32_tensor(self._tape.randn((H, W))).to(dev)
        if self.csdvs_enabled:  # emulator.py:707-708: between the low-pass and the event computation
            self._update_csdvs(P, frame_dev, t_prev, t_frame, fidx)
        if not counted:
            eng.count(P, frame_dev, [t_prev], [t_frame], fidx, leak_randn=leak)
        if self._state_planes is not None:
            model_states.show_states(self, new_frame, t_frame)
        rec = eng.read_rec(fidx)[0]
        M = int(rec.max_events)
        eng.reserve_iters(M)
        n = M if M > 0 else 1
        ts_dev = None
        if tape:
            ts_step = (t_frame - t_prev) / n
            ts = self._tape.linspace(t_prev + ts_step, t_frame, n)
            ts_dev = _as_f32_tensor(ts).to(dev).view(1, n)

        eng.rank(P, fidx, ts_dev)
        itc = eng.read_iter_counts(fidx, M)[0]  # [M+1][2]; last row = shot pair
        perms = []  # tape mode: (iteration's first row, its randperm) of every non-empty iteration
        if tape:
            row = 0
            for i in range(M):
                n_i = int(itc[i, 0]) + int(itc[i, 1])
                if n_i > 0:
                    perms.append((row, self._tape.randperm(n_i, fidx, i)))
                row += n_i
            if self.shot_noise_rate_hz > 0 and not self.photoreceptor_noise:
                u = _as_f32_tensor(self._tape.rand((H, W))).to(dev)
                eng.shot(P, frame_dev, fidx, u)
                eng.rank(P, fidx, ts_dev)
                itc = eng.read_iter_counts(fidx, M)[0]
        n_events = int(itc.sum())
        n_on = int(itc[:, 0].sum())
        n_off = int(itc[:, 1].sum())
        n_signal = int(itc[:M].sum())

        events = None
        ev = eng.event_buffer(max(n_events, 1))
        eng.emit(P, fidx, ev, ts_dev, ev_offset0=[0])
        if n_signal > 0 and perms:
            # events_curr_iter[idx] for every iteration (emulator.py:868-869) as ONE gather: the per-iteration
            # permutations, offset to absolute rows, in one pinned upload and one launch
            if eng._events_tmp is None or eng._events_tmp.shape != ev.shape:
                eng._events_tmp = torch.empty_like(ev)
            out = eng._events_tmp
            idx_all = np.empty(n_signal, dtype=np.int32)
            for row, idx in perms:  # (the shot pass in between leaves the iterations' counts as they were)
                idx = idx.numpy() if torch.is_tensor(idx) else np.asarray(idx)
                np.add(idx, row, out=idx_all[row:row + len(idx)], casting="unsafe")
            pin = self._idx_pin
            if pin is None or pin.numel() < n_signal:
                cap_n = max(n_signal, 1 << 16) * 2
                self._idx_pin = pin = torch.empty(cap_n, dtype=torch.int32).pin_memory()
                self._idx_dev = torch.empty(cap_n, dtype=torch.int32, device=dev)
            pin[:n_signal].copy_(torch.from_numpy(idx_all))
            idx_dev = self._idx_dev[:n_signal]
            idx_dev.copy_(pin[:n_signal], non_blocking=True)
            eng.permute(ev, out, idx_dev, 0, n_signal)
            if n_events > n_signal:
                out[0, n_signal:n_events] = ev[0, n_signal:n_events]
            eng._events, eng._events_tmp = out, ev
            ev = out
        if n_events > 0:
            events = ev[0, :n_events].cpu().numpy()

        return self._frame_done(new_frame, t_frame, M, n_events, n_on, n_off, n_signal, events, ev)

    def _frame_done(self, new_frame, t_frame, M, n_events, n_on, n_off, n_signal, events, ev):
        """The tail of every frame after the first, whichever path computed it: the reference's two warnings (emulator.py:776-777,
        805-807), the counters, the event files, the recorder, t_previous.  events: the frame's host rows or None; ev: the device
        buffer they are the first n_events rows of."""
        if M > 100:
            logger.warning(f'Too many events generated for this frame: num_iter={M}>100 events')
        if M == 0 and self.no_events_warning_count < 100:
            logger.warning(f'no signal events generated for frame #{self.frame_counter:,} at t={t_frame:.4f}s')
            self.no_events_warning_count += 1
        self.num_events_on += n_on
        self.num_events_off += n_off
        self.num_events_total += n_events
        if events is not None:
            event_files.write_frame(self, events, n_signal, events_dev=ev[0, :n_events])
        if self.frame_ev_idx_dataset is not None:  # emulator.py:979-983: where the frame's events end
            self.frame_ev_idx_dataset[self.frame_counter - 1] = self.dvs_h5_dataset.shape[0]
        if self.record_single_pixel_states is not None:  # (never on the one-call Philox frame)
            model_states.record_pixel(self, new_frame, t_frame, events, n_signal)
        self.t_previous = t_frame
        return events

    def _prepare_pnoise(self, eng, rates):
        """emulator.py:694-703 before the frames whose sample rates (1 / interval) are `rates`, one for generate_events, a run's
        for a device-resident run: the noise plane, created on the first such frame (zeros_like(lp_log_frame), emulator.py:684; it
        stays on the device), and the amplitude.  The reference recomputes the amplitude when the sample rate has moved by 10 % from
        the rate it was last computed for (emulator_utils.py:217-220); inside one device-resident run the amplitude is one
        number, so every frame of the run must stay within 10 % of the rate that number belongs to."""
        if self.photoreceptor_noise_arr is None:
            self._pn_plane = torch.zeros((1, eng.npx_pad), dtype=torch.float64, device=eng.device)
            self.photoreceptor_noise_arr = eng.plane(self._pn_plane)
        if self.photoreceptor_noise_vrms is not None:
            self._pn_vrms = float(self.photoreceptor_noise_vrms)
            return

        def moved(rate):
            return abs(rate / self._pn_last_rate - 1) >= 0.1

        if self._pn_last_rate is None or moved(rates[0]):
            self._pn_vrms = photoreceptor_noise_vrms(self.shot_noise_rate_hz, self.cutoff_hz, rates[0], self.pos_thres_nominal,
                                                     self.neg_thres_nominal, self.sigma_thres)
            self._pn_last_rate = rates[0]
        if any(moved(r) for r in rates):
            raise ValueError("photoreceptor_noise: the frame interval moves by more than 10 % from the rate the noise "
                             "amplitude was computed for inside this run; split the run there (or use generate_events "
                             "per frame)")

    def save_recorded_single_pixel_states(self):  # emulator.py:431-437
        model_states.save_pixel_states(self)

    # ------------------------------------------------------------- centre-surround
    CSDVS_RUN_MAX_STEPS = 8192  # Euler steps per frame a device-resident run enqueues up front
    CSDVS_RUN_MAX_TOTAL_STEPS = 65536  # ... and per run: every step is a launch (a graph node), taken or not (round-4 advisor)

    def _csdvs_step_params(self, delta_time):
        """emulator.py:1066-1096: (num_steps, alpha_p, alpha_h) of one frame interval, with the reference's warnings and its
        refusal of a diverging diffuser."""
        abs_min_tau_p = 1e-9
        tau_p = abs_min_tau_p if (self.cs_tau_p_ms is None or self.cs_tau_p_ms == 0) else self.cs_tau_p_ms * 1e-3
        tau_h = abs_min_tau_p / (self.cs_lambda_pixels ** 2) if (self.cs_tau_h_ms is None or self.cs_tau_h_ms == 0) \
            else self.cs_tau_h_ms * 1e-3
        min_tau = min(tau_p, tau_h)
        NUM_STEPS_PER_TAU = 5
        num_steps = int(np.ceil((delta_time / min_tau) * NUM_STEPS_PER_TAU))
        actual_delta_time = delta_time / num_steps
        if num_steps > 1000 and not self.cs_steps_warning_printed:
            if self.cs_tau_p_ms == 0:
                logger.warning(f'You set time constant cs_tau_p_ms to zero which set the minimum tau of {abs_min_tau_p}s')
            logger.warning(f'CSDVS timestepping of diffuser could take up to {num_steps} steps per frame for Euler delta time '
                           f'{actual_delta_time:.3g}s; simulation of each frame will terminate when max change is smaller than '
                           f'{self.MAX_CHANGE_TO_TERMINATE_EULER_SURROUND_STEPPING}')
            self.cs_steps_warning_printed = True
        alpha_p = actual_delta_time / tau_p
        alpha_h = actual_delta_time / tau_h
        if alpha_p >= 1 or alpha_h >= 1:
            logger.error(f'CSDVS update alpha (of IIR update) is too large; simulation would explode: '
                         f'alpha_p={alpha_p:.3f} alpha_h={alpha_h:.3f}')
            self.cs_alpha_warning_printed = True
            raise SystemExit(1)  # v2e_quit(1)
        if alpha_p > .25 or alpha_h > .25:
            logger.warning(f'CSDVS update alpha (of IIR update) is too large; simulation will be inaccurate: '
                           f'alpha_p={alpha_p:.3f} alpha_h={alpha_h:.3f}')
            self.cs_alpha_warning_printed = True
        return num_steps, alpha_p, alpha_h

    def _update_csdvs(self, P, frame_dev, t_prev, t_frame, fidx):
        """emulator.py:1061-1124.  The host part (step count, IIR coefficients, warnings, the refusal of a diverging
        diffuser) as the reference writes it; the stepping loop is v2e_csdvs_update on the device planes, driven by the
        coming frame's lp_log_frame (v2e_emu_lp_preview: the low-pass applied to the state as it is)."""
        eng = self._engine
        num_steps, alpha_p, alpha_h = self._csdvs_step_params(t_frame - t_prev)
        sur, scratch, lp_new = self._cs_planes
        eng.lp_preview(P, frame_dev, [t_prev], [t_frame], fidx, lp_new)
        steps = eng.csdvs_update(lp_new, sur, scratch, alpha_p, alpha_h, num_steps, self.MAX_CHANGE_TO_TERMINATE_EULER_SURROUND_STEPPING)
        self.cs_steps_taken.append(steps)

    # ------------------------------------------------------------- device-resident clip
    def generate_events_batch(self, frames, t_frames, return_device=False, use_graph=True, cap=None, *, probe_pixels=None):
        """Philox mode: run a whole clip [F,H,W] with timestamps t_frames[F] on device.

        Equivalent to calling generate_events once per frame (same events, same order) but
        with no host synchronisation between frames.  Returns (events, counts): events is
        an [N,4] float32 array (or device tensor) of all frames' events concatenated,
        counts[f] the number of events of frame f (0 for the very first frame).
        probe_pixels: see generate_events_batch_async; the series are left in `last_probes`.
        """
        pipelined = None
        if use_graph is True:
            # the default: one hipGraph per run -- from the SECOND run of a length on.  Capturing and instantiating the graph costs ~2.3 ms,
            # more than it saves a run that is never repeated (an emulator per clip, BASELINE configs[2]: 88.3 -> 86.0 ms per clip)
            seen = self._blocking_lengths
            n = int(frames.shape[0])
            if seen.get(n, 0) == 0:
                use_graph, pipelined = 0, False
            seen[n] = seen.get(n, 0) + 1
        pend = self.generate_events_batch_async(frames, t_frames, return_device=return_device, use_graph=use_graph,
                                                cap=cap, _single_buffer=True, pipelined=pipelined, probe_pixels=probe_pixels)
        res = pend.result()
        if probe_pixels is not None:
            self.last_probes = pend.probes
        return res

    def generate_events_batch_async(self, frames, t_frames, return_device=False, use_graph=True, cap=None,
                                    _single_buffer=False, pipelined=None, frames_resident=False, *, probe_pixels=None):
        """generate_events_batch without waiting for the device: enqueues the run and returns a handle whose
        result() gives (events, counts).  The host can prepare and enqueue the next run (it executes behind this one
        on the same stream) before reading this one's result: two sets of event / record buffers alternate, so a
        result stays valid until the second-next call (a handle still unread at that point is collected by that call, device rows
        copied aside).  Pixel state, frame counter and t_previous advance at enqueue
        time; the event counters (num_events_*) when result() is called; errors (capacity, max_iters) are raised there.
        use_graph: True / 1 one hipGraph per run (what the blocking call uses: lowest latency of a single run), 0 plain launches.
        pipelined (default: on where use_graph is 0): consecutive runs overlap -- the run's upload and first records go out beside the run
        before, its last emission batches finish beside the run after, the current stream carries the chain's launches only
        (v2e_emu_run, RUN_PIPELINED): the throughput mode of a loop that keeps one run enqueued ahead (bench.py).  The current stream then
        orders the pixel state only; result() waits for the rows.  frames_resident=True: the caller vouches that nothing enqueued on
        the current stream still writes `frames`; the run's head then need not wait for the chain of the run before.
        probe_pixels=[(a, b), ...] (at most 64; one fewer beside record_single_pixel_states): the handle carries `.probes` after
        result(), a dict of the reference's ten single-pixel series (emulator.py:985-1009; PIXEL_STATE_SERIES) as float64 arrays
        [frames of the run, P], `time` broadcast, the pixels addressed as the reference's plane[a, b].  An emulator built with
        record_single_pixel_states records that pixel run after run the same way (appended to single_pixel_states in the order the
        runs were enqueued, when their results are read -- by the caller, by the call that reuses a dropped handle's buffers, or by
        cleanup()).  Either makes the run a probed one: the per-frame kernels instead of k_chain, never pipelined, three small
        launches beside them (v2e_emu_set_probes).
        """
        self._raise_if_failed()
        if self.rng_mode != "philox":
            raise ValueError("generate_events_batch needs rng_mode='philox' (tape mode needs the host per frame)")
        if self.show_dvs_model_state is not None:
            raise ValueError("show_dvs_model_state / save_dvs_model_state show or save a picture of the state after every frame: "
                             "use generate_events per frame")
        if isinstance(frames, np.ndarray):
            if frames.dtype not in (np.uint8, np.float32, np.float64):
                frames = frames.astype(np.float64)
        F = int(frames.shape[0])
        H, W = int(frames.shape[1]), int(frames.shape[2])
        t_frames = [float(t) for t in t_frames]
        if len(t_frames) != F:
            raise ValueError("need one timestamp per frame")
        user_idx = probe_pixel_indices(probe_pixels, H, W) if probe_pixels is not None else []
        if self.record_single_pixel_states is not None:
            probe_pixel_indices([self.record_single_pixel_states], H, W)
            if len(user_idx) >= _capi.PROBE_MAX:
                raise ValueError("at most %d pixels can be probed beside record_single_pixel_states" % (_capi.PROBE_MAX - 1))
        eng = self._ensure_engine(H, W)
        frames_dev = eng.to_device_frame(frames)
        counts = np.zeros(F, dtype=np.int64)
        start = 0
        if self.frame_h5_dataset is not None:  # emulator.py:636-638 per frame: the input frames of the HDF5 file
            fr = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
            self.frame_h5_dataset[self.frame_counter:self.frame_counter + F] = fr.astype(np.uint8)
        if not self._initialized:
            if t_frames[0] < self.t_previous:
                raise ValueError("frame time must not decrease")
            self.frame_counter += 1
            self._first_frame(frames_dev[0], H, W, t_frames[0])
            start = 1
        nrun = F - start
        if nrun <= 0:
            pend = runs.PendingRun(self, counts, start, return_device, empty=torch.empty((0, 4), dtype=torch.float32, device=eng.device))
            if probe_pixels is not None:
                pend.probes = {k: np.empty((0, len(user_idx))) for k in PIXEL_STATE_SERIES}
            return pend
        t_prev = []
        tp = float(self.t_previous)
        for f in range(start, F):
            if t_frames[f] < tp:
                raise ValueError("this frame time={} must be later than previous frame time={}".format(
                    t_frames[f], tp))
            t_prev.append(tp)
            tp = t_frames[f]
        if self.photoreceptor_noise:
            self._prepare_pnoise(eng, [1.0 / (t_frames[f] - t_prev[f - start]) for f in range(start, F)])
            eng.set_pnoise(self._pn_plane, None)
        cs_steps_dev = None
        if self.csdvs_enabled:
            # emulator.py:1061-1124 inside the run: per frame the host part (step count, coefficients) as the reference computes
            # it; the stepping loop is enqueued whole, its stop rule evaluated on the device (v2e_emu_set_csdvs_run)
            pars = [self._csdvs_step_params(t_frames[f] - t_prev[f - start]) for f in range(start, F)]
            if max(q[0] for q in pars) > self.CSDVS_RUN_MAX_STEPS:
                raise ValueError("generate_events_batch with cs_lambda_pixels: %d Euler steps per frame (cs_tau_p_ms / cs_lambda_pixels) "
                                 "would all be enqueued up front; beyond %d use generate_events per frame (its loop ends as soon as "
                                 "the diffuser has settled)" % (max(q[0] for q in pars), self.CSDVS_RUN_MAX_STEPS))
            if sum(q[0] for q in pars) > self.CSDVS_RUN_MAX_TOTAL_STEPS:
                raise ValueError("generate_events_batch with cs_lambda_pixels: %d Euler steps over the run's %d frames would all be "
                                 "enqueued up front (mostly no-op launches once the diffuser has settled); beyond %d split the run or use "
                                 "generate_events per frame" % (sum(q[0] for q in pars), nrun, self.CSDVS_RUN_MAX_TOTAL_STEPS))
            cs_steps_dev = torch.zeros(nrun, dtype=torch.int32, device=eng.device)
            ns = (C.c_int * nrun)(*[q[0] for q in pars])
            ap = (C.c_double * nrun)(*[q[1] for q in pars])
            ah = (C.c_double * nrun)(*[q[2] for q in pars])
            sur, scratch, lp_new = self._cs_planes
            _capi.check(eng.lib.v2e_emu_set_csdvs_run(eng._h, scratch.data_ptr(), lp_new.data_ptr(), ap, ah, ns, nrun,
                                                      float(self.MAX_CHANGE_TO_TERMINATE_EULER_SURROUND_STEPPING),
                                                      cs_steps_dev.data_ptr()), "v2e_emu_set_csdvs_run")
        rec_claim = runs.claim_samples(self, nrun) if self.record_single_pixel_states is not None else 0
        recording = self.record_single_pixel_states is not None  # (a recorder whose series were full has ended in claim_samples)
        probe_idx = (probe_pixel_indices([self.record_single_pixel_states], H, W) if recording else []) + user_idx
        P = self._params()
        if cap is None:
            cap = default_event_capacity(nrun, H, W)
        which = runs.take_buffer_set(self, _single_buffer)
        ev = eng.event_buffer(cap, which)
        recs = eng.alloc_recs(nrun, which)
        ug = int(use_graph)
        if self._refr_mostly_on:
            ug |= _capi.RUN_ONE_FRAME_PER_LAUNCH  # the speculating chain would redo most of its launches
        if (ug & (_capi.RUN_GRAPH | _capi.RUN_PROFILE)) == 0 and (pipelined or pipelined is None) and not _single_buffer:
            ug |= _capi.RUN_PIPELINED | (_capi.RUN_FRAMES_RESIDENT if frames_resident else 0)
        probe_dev = None
        if probe_idx:
            probe_dev = eng.probe_buffer(nrun, len(probe_idx), which)
            eng.set_probes(probe_idx, probe_dev)
        eng.run(P, frames_dev[start:], t_prev, t_frames[start:], self.frame_counter, ev, recs, use_graph=ug)
        # Both chains read the frames until the run's last launch (the one on k_ahead's records takes the pixel bytes from them), and
        # k_ahead reads them on a stream of the library's own: they stay referenced until this buffer set's next run is enqueued,
        # behind this one, whether or not the caller keeps its tensor or the handle.
        self._run_frames[which] = frames_dev
        ticket = None
        if ug & _capi.RUN_PIPELINED:
            # the library may have enqueued the run in pieces on streams of its own: result() waits for them on the host; a device-side
            # event (the `done` property) is only built for a caller that asks for one
            done, ticket = None, eng.run_ticket()
        if ticket is None or ticket < 0:
            ticket = None
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(eng.device))
        pend = runs.PendingRun(
            self, counts, start, return_device, ev=ev, recs=recs, _done=done, ticket=ticket, which=which, frame0=self.frame_counter,
            dts=np.asarray(t_frames[start:]) - np.asarray(t_prev), times=t_frames[start:], cs_steps_dev=cs_steps_dev,
            probe_dev=probe_dev, probe_rec=recording, probe_claim=rec_claim,
            # (the thresholds the reference would record where it holds Python floats, emulator.py:992-995: as they are now)
            thres=(self.pos_thres if type(self.pos_thres) is float else None, self.neg_thres if type(self.neg_thres) is float else None))
        self.frame_counter += nrun
        self.t_previous = t_frames[-1]
        self._async_slots[which] = weakref.ref(pend)
        if event_files.any_open(self) or recording:
            # held strongly until its rows are in the files (its samples in single_pixel_states), in the order the runs were enqueued
            # (a handle the caller drops is written by the call that reuses its buffer set, or by cleanup())
            self._sink_runs.append(pend)
        return pend
