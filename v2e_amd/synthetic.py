"""The reference's synthetic input sources (v2e.py --synthetic_input=scripts.<name>, v2e.py:580-612) with their frames rendered
by HIP kernels straight into HBM (v2e_amd/csrc/synth.hip), and `SyntheticToEvents`, which feeds them block by block to
`EventEmulator.generate_events_batch_async`: no frame ever exists on the host.

`moving_dot`, `particles`, `gradients` and `barberpole` take the constructor arguments of the reference classes of the same names
(scripts/moving_dot.py, particles.py, gradients.py, barberpole.py: width, height, avi_path, preview, arg_list, parent_args; arg_list
holds the same command-line flags with the same defaults) and have their attributes and methods: `times`, `dt`, `t_total`,
`total_frames()`, `next_frame() -> (frame | None, time)`, `cleanup()`.  `frames_block(f0, n, out=None)` is the device-resident
interface: frames f0 .. f0 + n - 1 as one device tensor [n, H, W] and their times; any split of a clip into blocks gives the same
frames.  `next_frame()` hands out host copies of such blocks one frame at a time: there is one implementation of the pixels.

The host computes what is per frame and tiny, in the reference's own expressions (the np.arange times, theta, the shrinking
radius, Python round(), the bump position p, the particle state machine with the same np.random calls in the same order); the
kernels restate the per-pixel part in float64 in the reference's order of operations.

Where this differs from the reference, on purpose:
  * arg_list=None parses no flags (the reference then parses sys.argv, which under v2e.py is never the case);
  * avi_path / preview are accepted and skipped with one warning (cv2 is host work and not available here);
  * a `moving_dot` box that leaves the frame raises ValueError before any launch (the reference has no bounds check there: numba
    wraps or corrupts, plain Python raises IndexError or wraps negative indices);
  * `particles` with parent_args.hdr keeps its float32 frame (numpy >= 2 would promote the reference's frame to float64, because
    np.log returns a float64 scalar; numpy 1.x, which the reference was written for, keeps float32);
  * `moving_dot` with an explicit --bg (argparse then yields a float, and numpy makes the reference's frame float64) renders
    float64 frames; with the default bg the frame is uint8 as in the reference.

Left out: `single_linearly_moving_dot` is not a base_synthetic_input, so v2e.py itself refuses it (v2e.py:590), and the box of its
fixed trajectory leaves the frame at both ends; `spots` draws with scikit-image (skimage.draw), which is not available to pin a
restatement against.
"""
import argparse
import ctypes as C
import logging

import numpy as np
import torch

from . import _capi
from ._capi import check, ptr, stream_ptr
from .emulator import default_event_capacity

logger = logging.getLogger(__name__)

BACKGROUND = 127  # base_synthetic_input.BACKGROUND
_NP_DT = {_capi.DT_U8: np.uint8, _capi.DT_F32: np.float32, _capi.DT_F64: np.float64}
_TORCH_DT = {_capi.DT_U8: torch.uint8, _capi.DT_F32: torch.float32, _capi.DT_F64: torch.float64}
_warned_host_video = False


class _DeviceSource:
    """What the four sources share: the reference's frame interface on top of `frames_block`."""
    NEXT_FRAME_BLOCK = 64  # frames per device block behind next_frame()
    out_dtype = _capi.DT_U8

    def __init__(self, width, height, avi_path, preview, arg_list, parent_args, device):
        global _warned_host_video
        self.width, self.height = int(width), int(height)
        self.w, self.h = self.width, self.height
        self.avi_path, self.preview = avi_path, preview
        self.args, self.parent_args = arg_list, parent_args
        self.device = torch.device("cuda:0" if device is None else device)
        self.frame_number = 0
        self.time = 0
        self._host_block = None  # (first frame, frames on the host, times) behind next_frame()
        if (avi_path is not None or preview) and not _warned_host_video:
            logger.warning("v2e_amd.synthetic: avi_path=%r / preview=%r need OpenCV on the host: the AVI / preview of the synthetic "
                           "input is skipped, the frames are not affected", avi_path, preview)
            _warned_host_video = True

    def total_frames(self):
        """:returns: total number of frames"""
        return len(self.times)

    def cleanup(self):
        pass

    def _check_block(self, f0, n, out):
        f0, n = int(f0), int(n)
        if f0 < 0 or n <= 0 or f0 + n > len(self.times):
            raise ValueError("frames %d .. %d are not inside the clip's %d frames" % (f0, f0 + n - 1, len(self.times)))
        dt = _TORCH_DT[self.out_dtype]
        if out is None:
            out = torch.empty((n, self.h, self.w), dtype=dt, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != dt or tuple(out.shape) != (n, self.h, self.w) or not out.is_contiguous()
              or out.device.type != self.device.type or self.device.index not in (None, out.device.index)):
            raise ValueError("out must be a contiguous %s tensor [%d, %d, %d] on %s" % (dt, n, self.h, self.w, self.device))
        return f0, n, out

    def _upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def next_frame(self):
        """The next frame (a host array of its own) and its time, or (None, times[-1]) when finished."""
        k = self.frame_number
        if k >= len(self.times):
            return None, self.times[-1]
        hb = self._host_block
        if hb is None or not (hb[0] <= k < hb[0] + len(hb[1])):
            n = min(self.NEXT_FRAME_BLOCK, len(self.times) - k)
            fr, t = self.frames_block(k, n)
            hb = self._host_block = (k, fr.cpu().numpy(), t)
        self.frame_number += 1
        return hb[1][k - hb[0]].copy(), hb[2][k - hb[0]]


class _DotSource(_DeviceSource):
    """Sources drawn by fill_dot: `dot_table` is the host part, `v2e_synth_dots` the pixels."""

    def frames_block(self, f0, n, out=None):
        """Frames f0 .. f0 + n - 1 rendered on the device: (tensor [n, H, W], times[n])."""
        f0, n, out = self._check_block(f0, n, out)
        offs, xy, box = self.dot_table(f0, n)
        nd = int(offs[-1])
        # one small upload: offsets (padded to 8 bytes), centres, boxes
        no = (n + 1 + 1) // 2 * 2
        blob = np.zeros(no * 4 + nd * 16 + nd * 8 + 8, dtype=np.uint8)
        blob[:4 * (n + 1)] = offs.astype(np.int32).view(np.uint8)
        blob[no * 4:no * 4 + nd * 16] = xy.astype(np.float64).reshape(-1).view(np.uint8)
        blob[no * 4 + nd * 16:no * 4 + nd * 24] = box.astype(np.int32).reshape(-1).view(np.uint8)
        dev = self._upload(blob)
        base = dev.data_ptr()
        bg, fg, sigma, d, peak, low_cut, clip = self._dot_params()
        check(_capi.lib().v2e_synth_dots(C.c_void_p(base + no * 4), C.c_void_p(base + no * 4 + nd * 16), C.c_void_p(base), n, self.h,
                                         self.w, ptr(out), self.out_dtype, float(bg), float(fg), float(sigma), int(d), float(peak),
                                         float(low_cut), int(clip), stream_ptr(self.device)), "v2e_synth_dots")
        dev.record_stream(torch.cuda.current_stream(self.device))
        return out, self.times[f0:f0 + n]


class moving_dot(_DotSource):
    """scripts/moving_dot.py: dots on a shrinking circle."""

    def __init__(self, width=346, height=260, avi_path=None, preview=False, arg_list=None, parent_args=None, *, device=None):
        super().__init__(width, height, avi_path, preview, arg_list, parent_args, device)
        parser = argparse.ArgumentParser("moving_dot")
        parser.add_argument('--num_particles', type=int, default=5)
        parser.add_argument('--contrast', type=float, default=10)
        parser.add_argument('--bg', type=float, default=5)
        parser.add_argument('--radius', type=float, default=100)
        parser.add_argument('--cycles', type=float, default=None, help='number of cycles of moving dots')
        parser.add_argument('--dt', type=float, default=100e-6, help='time step in seconds')
        parser.add_argument('--t_total', type=float, default=None, help='specifies total time in seconds if given, other use cycles')
        args = parser.parse_args([] if arg_list is None else arg_list)
        if (args.cycles is None and args.t_total is None) or (args.cycles is not None and args.t_total is not None):
            raise Exception('specify either one of --cycles or --t_total')
        # moving_dot.py:83-116, statement for statement
        self.speed_pps = 1000
        self.dot_sigma = 1
        self.radius = args.radius
        self.dt = args.dt
        self.num_dots = args.num_particles
        self.contrast = args.contrast
        self.bg = args.bg  # (the default is the int 5: argparse converts only strings)
        self.circum = 2 * np.pi * self.radius
        self.period = self.circum / self.speed_pps
        if args.t_total is not None:
            self.t_total = args.t_total
            self.cycles = self.t_total / self.period
        else:
            self.cycles = args.cycles
            self.t_total = self.circum * self.cycles / self.speed_pps
        self.times = np.arange(0, self.t_total, self.dt)
        self.theta = 2 * np.pi * self.cycles * (self.times / self.t_total)
        self.fg = int(self.bg * self.contrast)
        self.d = int(self.dot_sigma * 3)
        self.fps = 60
        # moving_dot.py:156: bg * np.ones(uint8) is a uint8 frame for the int default, a float64 one for a float bg
        self.out_dtype = _capi.DT_U8 if isinstance(self.bg, int) else _capi.DT_F64
        if self.out_dtype == _capi.DT_U8 and not 0 <= self.bg <= 255:
            raise ValueError("bg is a grey level 0..255")

    def _dot_params(self):
        return self.bg, self.fg, self.dot_sigma, self.d, 10, .01, 1

    def dot_table(self, f0, n):
        """The dots of frames f0 .. f0 + n - 1 (moving_dot.py:155-169): (offs int32 [n + 1], centres float64 [dots, 2] x, y,
        rounded centres int32 [dots, 2] x0, y0).  A box [x0 - d, x0 + d) x [y0 - d, y0 + d) that leaves the frame raises ValueError."""
        offs, xy, box = [0], [], []
        d = self.d
        for k in range(f0, f0 + n):
            time = self.times[k]
            if self.contrast != 1:  # only fill dots if they are visible
                cycles = time / self.period
                radius = self.radius - cycles * self.d * 1.5
                for i in range(self.num_dots):
                    theta = self.theta[k] + (i / self.num_dots) * 2 * np.pi
                    x = self.w / 2 + radius * np.cos(theta)
                    y = self.h / 2 + radius * np.sin(theta)
                    x0, y0 = round(x), round(y)
                    if x0 - d < 0 or x0 + d > self.w or y0 - d < 0 or y0 + d > self.h:
                        raise ValueError("moving_dot: the box of dot %d of frame %d, centre (%d, %d) +-%d, leaves the %d x %d frame "
                                         "(the reference has no bounds check here); use a smaller --radius"
                                         % (i, k, x0, y0, d, self.w, self.h))
                    xy.append((x, y))
                    box.append((x0, y0))
            offs.append(len(xy))
        return (np.asarray(offs, np.int32), np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(box, np.int32).reshape(-1, 2))


class _Particle:
    """particles.py:118-162 with the position and velocity as two Python floats each (the same IEEE doubles as the reference's
    two-element arrays)."""
    __slots__ = ("width", "height", "x", "y", "vx", "vy", "speed", "contrast", "time", "radius")

    def __init__(self, rng, width, height, time, radius, speed_min, speed_max, start_on_edge=False):
        self.width = width
        self.height = height
        if start_on_edge:
            edge = rng.randint(0, 4)
            if edge == 0 or edge == 1:
                pos_x = rng.randint(0, width)
                pos_y = 0 if edge == 0 else height
            else:
                pos_y = rng.randint(0, height)
                pos_x = 0 if edge == 3 else width
            angle_rad = 0
            if edge == 1:
                angle_rad = rng.uniform(np.pi / 4, -.75 * np.pi)
            elif edge == 0:
                angle_rad = rng.uniform(np.pi / 4, .75 * np.pi)
            elif edge == 3:
                angle_rad = rng.uniform(-np.pi / 4, np.pi / 4)
            elif edge == 2:
                angle_rad = rng.uniform(np.pi / 4, 3 * np.pi / 2 - np.pi / 4)
        else:
            pos_x = rng.uniform(0, width)
            pos_y = rng.uniform(0, height)
        angle_rad = rng.uniform(0, 2 * np.pi)  # (particles.py:146 stands outside the else: it replaces the edge's angle too)
        self.x, self.y = float(pos_x), float(pos_y)
        self.speed = rng.uniform(speed_min, speed_max)
        self.vx, self.vy = float(self.speed * np.cos(angle_rad)), float(self.speed * np.sin(angle_rad))
        self.contrast = rng.uniform(1.19, 1.21)
        self.time = float(time)
        self.radius = radius

    def update(self, time):
        dt = time - self.time
        self.x = self.x + dt * self.vx
        self.y = self.y + dt * self.vy
        self.time = time

    def is_out_of_bounds(self):
        return self.x < 0 or self.x > self.width or self.y < 0 or self.y > self.height


class particles(_DotSource):
    """scripts/particles.py: dots on linear trajectories, replaced as they leave.  The clip carries state (the particle list and
    the random stream), so its blocks must be taken in order, each frame once: anything else raises ValueError.
    rng: an np.random.RandomState to draw from; default the global np.random module, as in the reference."""
    CONTRAST = 1.25
    TOTAL_TIME = 1
    NUM_PARTICLES = 300
    RADIUS = 1
    DT = 100e-6
    SPEED_MIN = 3
    SPEED_MAX = 100
    BACKGROUND = BACKGROUND
    out_dtype = _capi.DT_F32

    def __init__(self, width=346, height=260, avi_path=None, preview=False, arg_list=None, parent_args=None, *, device=None,
                 rng=None):
        super().__init__(width, height, avi_path, preview, arg_list, parent_args, device)
        parser = argparse.ArgumentParser("particles")
        parser.add_argument('--num_particles', type=int, default=particles.NUM_PARTICLES, help='max number of particles at one time')
        parser.add_argument('--contrast', type=float, default=particles.CONTRAST, help='constrast of each particle relative to background')
        parser.add_argument('--bg', type=float, default=particles.BACKGROUND, help='background brightness 0-255')
        parser.add_argument('--radius', type=float, default=particles.RADIUS, help='radius of each particle, px')
        parser.add_argument('--total_time', type=float, default=particles.TOTAL_TIME, help='total simulation time in seconds')
        parser.add_argument('--speed_min', type=float, default=particles.SPEED_MIN, help='min speed in px/s, uniform sampling')
        parser.add_argument('--speed_max', type=float, default=particles.SPEED_MAX, help='max speed in px/s, uniform sampling')
        parser.add_argument('--dt', type=float, default=particles.DT, help='event timestemp, seconds')
        parser.add_argument('--edge', action='store_true', help='start all particles on edge, otherwise at random location')
        args = parser.parse_args([] if arg_list is None else arg_list)
        self._rng = np.random if rng is None else rng
        # particles.py:66-93
        self.contrast = args.contrast
        self.dt = args.dt
        self.radius = args.radius
        self.speed_pps_min = args.speed_min
        self.speed_pps_max = args.speed_max
        self.num_particles = args.num_particles
        self.particle_count = 0
        self.t_total = args.total_time
        self.start_on_edge = args.edge
        self.bg = args.bg
        self.fg = self.bg * self.contrast
        if getattr(parent_args, "hdr", False):
            self.bg = np.log(self.bg)
            self.fg = np.log(self.fg)
        self.particles = []
        for i in range(self.num_particles):
            p = _Particle(self._rng, width, height, 0, self.radius, self.speed_pps_min, self.speed_pps_max, self.start_on_edge)
            self.particles.append(p)
            self.particle_count += 1
        self.times = np.arange(0, self.t_total, self.dt)
        self.time = 0
        self._state_frame = 0  # the next frame the state machine can produce

    def cleanup(self):
        logger.info(f'particles() generated {self.particle_count:,} particles in {self.time:.3f}s')

    def _dot_params(self):
        return self.bg, self.fg, self.radius, int(self.radius * 2) + 1, 2, -1.0, 0

    def _step(self):
        """particles.py:186-197 for the next frame: the positions drawn, in order.  The loop's behaviour is the reference's by
        construction, the same list operations: removing while iterating skips the particle that follows, a particle appended in
        the loop is visited in the same frame, an out-of-bounds particle is replaced and not drawn."""
        self.time = self.times[self._state_frame]
        t = float(self.time)
        drawn = []
        for p in self.particles:
            if p.is_out_of_bounds():
                self.particles.remove(p)
                newp = _Particle(self._rng, self.w, self.h, t, self.radius, self.speed_pps_min, self.speed_pps_max, self.start_on_edge)
                self.particles.append(newp)
                self.particle_count += 1
            else:
                p.update(t)
                drawn.append((p.x, p.y))
        self._state_frame += 1
        return drawn

    def dot_table(self, f0, n):
        """The dots of frames f0 .. f0 + n - 1 as `moving_dot.dot_table` gives them (x0, y0 = round(x), round(y), particles.py:225);
        advances the state, so f0 must be the frame after the last one taken."""
        if f0 != self._state_frame:
            raise ValueError("particles carries state from frame to frame: the next block must start at frame %d, not %d"
                             % (self._state_frame, f0))
        if f0 + n > len(self.times):
            raise ValueError("frames %d .. %d are not inside the clip's %d frames" % (f0, f0 + n - 1, len(self.times)))
        offs, xy, box = [0], [], []
        for _ in range(n):
            for x, y in self._step():
                x0, y0 = round(x), round(y)
                if abs(x0) > 1 << 30 or abs(y0) > 1 << 30:
                    raise ValueError("particles: a particle at (%g, %g) is beyond the kernel's integer range" % (x, y))
                xy.append((x, y))
                box.append((x0, y0))
            offs.append(len(xy))
        return (np.asarray(offs, np.int32), np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(box, np.int32).reshape(-1, 2))


class gradients(_DeviceSource):
    """scripts/gradients.py: a triangular bump and a sharp bar moving to the right."""
    CONTRAST = 2
    TOTAL_TIME = 1
    DT = 100e-6
    SPEED_PPS = 300
    BUMP_WIDTH = .5

    def __init__(self, width=346, height=260, avi_path=None, preview=False, arg_list=None, parent_args=None, *, device=None):
        super().__init__(width, height, avi_path, preview, arg_list, parent_args, device)
        parser = argparse.ArgumentParser("gradients")
        parser.add_argument('--contrast', type=float, default=gradients.CONTRAST)
        parser.add_argument('--total_time', type=float, default=gradients.TOTAL_TIME)
        parser.add_argument('--speed_pps', type=float, default=gradients.SPEED_PPS)
        parser.add_argument('--dt', type=float, default=gradients.DT)
        parser.add_argument('--bump_width', type=float, default=gradients.BUMP_WIDTH)
        args = parser.parse_args([] if arg_list is None else arg_list)
        self.contrast = args.contrast
        self.dt = args.dt
        self.bg = BACKGROUND
        self.t_total = args.total_time
        self.speed_pps = args.speed_pps
        self.bump_width = args.bump_width
        self.times = np.arange(0, self.t_total, self.dt)

    def constants(self):
        """gradients.py:121-124: low, high, diff, w2."""
        low = (self.bg * 2) / (self.contrast + 1)
        high = self.contrast * low
        diff = high - low
        w2 = (self.bump_width * self.w) / 2
        return low, high, diff, w2

    def bump_centres(self, f0, n):
        """gradients.py:125 for frames f0 .. f0 + n - 1."""
        w2 = self.constants()[3]
        return w2 + self.times[f0:f0 + n] * self.speed_pps

    def frames_block(self, f0, n, out=None):
        """Frames f0 .. f0 + n - 1 rendered on the device: (uint8 tensor [n, H, W], times[n])."""
        f0, n, out = self._check_block(f0, n, out)
        low, high, diff, w2 = self.constants()
        p = self._upload(np.asarray(self.bump_centres(f0, n), np.float64))
        check(_capi.lib().v2e_synth_gradients(ptr(p), n, self.h, self.w, ptr(out), float(low), float(high), float(-diff / w2),
                                              float(w2), stream_ptr(self.device)), "v2e_synth_gradients")
        p.record_stream(torch.cuda.current_stream(self.device))
        return out, self.times[f0:f0 + n]


class barberpole(_DeviceSource):
    """scripts/barberpole.py: the barber pole illusion."""
    CONTRAST = 1.5
    TOTAL_TIME = 1
    DT = 100e-6
    SPEED_PPS = 1000
    NUM_STRIPES = 6
    BB_WIDTH = 0.8
    BB_HEIGHT = .2
    BB_ANGLE = 30

    def __init__(self, width=346, height=260, avi_path=None, preview=False, arg_list=None, parent_args=None, *, device=None):
        super().__init__(width, height, avi_path, preview, arg_list, parent_args, device)
        parser = argparse.ArgumentParser("barberpole")
        parser.add_argument('--num_stripes', type=int, default=barberpole.NUM_STRIPES)
        parser.add_argument('--contrast', type=float, default=barberpole.CONTRAST)
        parser.add_argument('--total_time', type=float, default=barberpole.TOTAL_TIME)
        parser.add_argument('--speed_pps', type=float, default=barberpole.SPEED_PPS)
        parser.add_argument('--dt', type=float, default=barberpole.DT)
        parser.add_argument('--bb_width', type=float, default=barberpole.BB_WIDTH)
        parser.add_argument('--bb_height', type=float, default=barberpole.BB_HEIGHT)
        parser.add_argument('--bb_angle', type=float, default=barberpole.BB_ANGLE)
        args = parser.parse_args([] if arg_list is None else arg_list)
        self.contrast = args.contrast
        self.dt = args.dt
        self.bg = BACKGROUND
        self.t_total = args.total_time
        self.speed_pps = args.speed_pps
        self.num_stripes = args.num_stripes
        self.bb_width = args.bb_width
        self.bb_height = args.bb_height
        self.bb_angle = args.bb_angle
        self.times = np.arange(0, self.t_total, self.dt)
        # barberpole.py:87-92: the pole is minx < x < maxx and miny < y < maxy
        dx = (1 - self.bb_width) / 2
        self.maxx = self.w - round(self.w * dx)
        self.minx = round(self.w * dx)
        dy = (1 - self.bb_height) / 2
        self.maxy = self.h - round(self.h * dy)
        self.miny = round(self.h * dy)

    def constants(self):
        """barberpole.py:156-161: wavelength, low, diff, tan."""
        wavelength = (self.bb_width * self.w) / self.num_stripes
        low = (self.bg * 2) / (self.contrast + 1)
        diff = (self.contrast - 1) * low
        tan = np.tan((90 - self.bb_angle) * np.pi / 180)
        return wavelength, low, diff, tan

    def frames_block(self, f0, n, out=None):
        """Frames f0 .. f0 + n - 1 rendered on the device: (uint8 tensor [n, H, W], times[n])."""
        f0, n, out = self._check_block(f0, n, out)
        wavelength, low, diff, tan = self.constants()
        t = self._upload(np.asarray(self.times[f0:f0 + n], np.float64))
        check(_capi.lib().v2e_synth_barberpole(ptr(t), n, self.h, self.w, ptr(out), float(low), float(diff), float(tan),
                                               float(self.speed_pps), float(2 * np.pi), float(wavelength), int(self.minx),
                                               int(self.maxx), int(self.miny), int(self.maxy), int(self.bg), stream_ptr(self.device)),
              "v2e_synth_barberpole")
        t.record_stream(torch.cuda.current_stream(self.device))
        return out, self.times[f0:f0 + n]


class SyntheticToEvents:
    """v2e.py:580-612 device-resident: the frames of a synthetic source go to the emulator in blocks of `block_frames` without
    ever existing on the host.  Events, counts and event files are those of `emulator.generate_events(frame, t)` called per frame
    on the same frames (Philox mode).  A uint8 source takes the emulator's uint8 path, `particles` its float32 path."""

    def __init__(self, source, emulator, block_frames=256):
        if int(block_frames) < 1:
            raise ValueError("block_frames must be positive")
        self.source, self.emu, self.block_frames = source, emulator, int(block_frames)
        self._side = None  # run(): the stream the source renders on, created on first need

    def run(self, on_events=None, return_device=False, on_frames=None):
        """Returns (events, counts per frame, n_frames).  on_events(events, counts, frame0) is called once per block in frame order
        (events None for a block without events on the host); nothing is accumulated then and events is None.  With
        return_device=True the rows are device tensors: inside on_events a view of one of the emulator's two alternating event
        buffers, valid for the duration of the callback.  on_frames(frames, times, frame0) is called once per block in frame order,
        on the caller's stream before the block's run is enqueued, with the very tensor [n,H,W] the emulator is about to read (one
        of the two frame buffers), its frame times and the index of its first frame -- ThresholdSweep.add_run takes it as it is (a
        uint8 source).  The tensor is valid for the duration of the callback only: work the callback enqueues on the current
        stream reads it before the buffer is rendered into again, anything else has to copy it.  Without on_frames nothing changes.

        Two frame buffers alternate: block b + 1 is rendered on a stream of its own while the emulator runs block b.  The host waits
        for a block's render before it enqueues the block's run, so the run is enqueued with frames_resident=True (nothing on the
        caller's stream writes the frames) and its head overlaps the run before.  The render that reuses a buffer comes after the
        result() of the run that read it, and waits on the device for an event recorded behind that run's chain."""
        src, emu = self.source, self.emu
        N, B = src.total_frames(), self.block_frames
        H, W, dev = src.h, src.w, src.device
        main = torch.cuda.current_stream(dev)
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        side = self._side
        side.wait_stream(main)
        blocks = [(f0, min(B, N - f0)) for f0 in range(0, N, B)]
        with torch.cuda.stream(side):
            bufs = [torch.empty((min(B, N), H, W), dtype=_TORCH_DT[src.out_dtype], device=dev) for _ in range(min(2, len(blocks)))]
        read_done = [None, None]
        cap = default_event_capacity(min(B, N), H, W)
        runs, counts, evs = [], [], []

        def render(b):
            f0, n = blocks[b]
            with torch.cuda.stream(side):
                if read_done[b & 1] is not None:
                    side.wait_event(read_done[b & 1])
                fr, t = src.frames_block(f0, n, out=bufs[b & 1][:n])
                ready = torch.cuda.Event()
                ready.record(side)
            return fr, t, ready

        def collect():
            pend, frame0 = runs.pop(0)
            ev, cnt = pend.result()
            counts.append(np.asarray(cnt))
            if on_events is not None:
                on_events(ev, cnt, frame0)
            elif ev is not None:
                evs.append(ev.clone() if return_device else ev)

        try:
            nxt = render(0)
            for b in range(len(blocks)):
                fr, t, ready = nxt
                ready.synchronize()
                if on_frames is not None:
                    # (the buffer is rendered into again only behind read_done, which is recorded on the caller's stream below:
                    #  behind the run's chain and so behind what the callback enqueued there, which must have read the frames)
                    on_frames(fr, t, blocks[b][0])
                pend = emu.generate_events_batch_async(fr, t, return_device=return_device, use_graph=0, cap=cap, frames_resident=True)
                read_done[b & 1] = torch.cuda.Event()
                read_done[b & 1].record(main)
                runs.append((pend, blocks[b][0]))
                if len(runs) == 2:  # the run before: its frame buffer is the one the next render writes
                    collect()
                if b + 1 < len(blocks):
                    nxt = render(b + 1)
            while runs:
                collect()
        finally:
            main.wait_stream(side)
            for buf in bufs:
                buf.record_stream(main)
        counts = np.concatenate(counts)
        if on_events is not None:
            return None, counts, N
        if return_device:
            return (torch.cat(evs) if evs else torch.empty((0, 4), dtype=torch.float32, device=dev)), counts, N
        return (np.concatenate(evs) if evs else None), counts, N
