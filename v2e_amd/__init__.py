"""v2e_amd -- the v2e hot path (DVS event emulator + SuperSloMo interpolation) on MI355X.

`EventEmulator` and `SuperSloMo` keep the reference's class signatures
(v2ecore/emulator.py:86-117, v2ecore/slomo.py:44-54) so that v2e.py can use them as
drop-in replacements.  All arithmetic runs in hand-written HIP
kernels for gfx950 (v2e_amd/csrc, C ABI in include/v2e_amd.h); there is no CPU path.
"""
from .emulator import EventEmulator  # noqa: F401
from .slomo import SuperSloMo  # noqa: F401
from .renderer import EventRenderer, ExposureMode, frame_times_text, run_packets, write_frame_times  # noqa: F401
from .preproc import Stage1  # noqa: F401  (v2e.py stage 1: INTER_AREA resize + BGR2GRAY on device; parity unpinned)
from .synthetic import SyntheticToEvents, barberpole, gradients, moving_dot, particles  # noqa: F401  (--synthetic_input sources in HBM)
from .tensors import EventTensorizer, plan_windows  # noqa: F401  (count / voxel / time-surface tensors of device-resident runs)
from .sweep import ThresholdSweep, estimate_thresholds  # noqa: F401  (event counts for many thresholds in one pass over a clip)
from .denoise import DenoiseResult, DenoiseSweep, denoise_rows  # noqa: F401  (correlation-filter ROC for all (k, tau) in one pass)
from .window import WindowResult, WindowSweep  # noqa: F401  (fixed-window-filter ROC for all (L, sigma, k) in one pass)
from .dwindow import DoubleWindowResult, DoubleWindowSweep  # noqa: F401  (double-window-filter ROC, one wavefront per (L, sigma, k))
from .patches import EventPatches, frame_labels, score_roc  # noqa: F401  (per-event time-surface patches for learned denoisers)
from .mlpf import MLPFilter  # noqa: F401  (a learned patch MLP scored per row in one fused pass)
from .stats import EventStats, EventStatsResult  # noqa: F401  (a stream's rates, intervals and time-bin counts)
from .readers import EventFileReader, read_events  # noqa: F401  (AEDAT-2.0 and text event files back into device rows)
from ._capi import V2EAmdError  # noqa: F401

__all__ = ["EventEmulator", "SuperSloMo", "EventRenderer", "ExposureMode", "Stage1", "V2EAmdError", "run_packets",
           "frame_times_text", "write_frame_times", "SyntheticToEvents", "moving_dot", "particles", "gradients", "barberpole",
           "EventTensorizer", "plan_windows", "ThresholdSweep", "estimate_thresholds", "DenoiseSweep", "DenoiseResult", "denoise_rows",
           "WindowSweep", "WindowResult", "DoubleWindowSweep", "DoubleWindowResult",
           "EventPatches", "frame_labels", "score_roc", "MLPFilter", "EventStats", "EventStatsResult", "EventFileReader", "read_events"]
