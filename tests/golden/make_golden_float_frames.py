#!/usr/bin/env python
"""Reference-generated fixtures of the float-frame input classes of tests/chain_dtypes.py (same file format as make_golden.py's
philox fixtures; the reference is imported by ref_harness.py): they pin the ORACLE's float-frame branches -- the yardstick of
tests/test_chain_dtypes_gpu.py -- on frames that hold the lin / log switch at 20.0 and its neighbours, values beyond 255
(inten01 > 1, eps at its clamp), fractional values and non-uniform frame intervals.

  philox_f64frames_33x37            float64 frames (not float32 values), cutoff_hz = 300: float64 state
  philox_f32frames_f32state_33x37   float32 frames, cutoff_hz = 0: float32 state
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
import chain_dtypes as cd  # noqa: E402


def main():
    mg.logging_off()
    H, W, n = 33, 37, 20
    for name, dtype, cutoff, seed in (("philox_f64frames_33x37", np.float64, 300, 31),
                                      ("philox_f32frames_f32state_33x37", np.float32, 0, 32)):
        frames, times = cd.clip(dtype, n, H, W, seed)
        kw = dict(cd.ALL_ON, cutoff_hz=cutoff)
        # (seed 23: the largest per-pixel count of a frame -- the column that alternates 0 <-> 255 under a small threshold draw -- is
        #  49 and 55, below the emulator's default max_iters of 64 that tests/test_emulator_gpu.py runs the fixtures with)
        mg.make_philox_fixture(name, list(frames), times, kw, seed=23, store_frames=True)
        limit = os.path.getsize(os.path.join(HERE, "philox_hdr_97x131.npz"))
        assert os.path.getsize(os.path.join(HERE, name + ".npz")) <= limit


if __name__ == "__main__":
    main()
