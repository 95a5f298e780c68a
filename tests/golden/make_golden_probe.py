"""Input-only fixture for tests/test_probe_gpu.py: philox_probe_flicker_97x131.npz (frames, times, seed).

The single-pixel recorder tests probe the pixel with the most signal events and need it to fire ON and OFF.  With scidvs=True no
committed Philox fixture has such a pixel: their busiest pixels fire OFF only (checked with the oracle: philox_scidvs_97x131 and
philox_scidvs_f32_97x131 52 OFF / 0 ON; the SCIDVS parameters on the frames of the pnoise, csdvs and moving-dot fixtures likewise).
This clip has a block that flickers between the background and a brighter grey level from frame to frame over a dark gradient with seeded texture (a bright background would bury the block under the OFF events every SCIDVS pixel fires while
its high-pass settles), so the pixels of
the block see steps up and down.  No expected outputs are stored: the tests compare the device-resident recorder with the per-frame
recorder, which tests/golden/single_pixel.npz pins to the reference.

    python tests/golden/make_golden_probe.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def frames(n=12, H=97, W=131, seed=41):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 1 + (xx * 3) // W + (yy * 2) // H
    out = np.empty((n, H, W), np.uint8)
    for k in range(n):
        f = base + rng.integers(0, 2, size=(H, W))
        if k >= 2 and k % 2 == 0:  # (dark at first: a block that starts bright would open with the same OFF burst)
            f[30:61, 40:93] = 6 + rng.integers(-1, 2, size=(31, 53))
        out[k] = np.clip(f, 0, 255).astype(np.uint8)
    return out


if __name__ == "__main__":
    fr = frames()
    np.savez_compressed(os.path.join(HERE, "philox_probe_flicker_97x131.npz"), frames=fr,
                        times=np.asarray([i / 300 for i in range(len(fr))], dtype=np.float64), seed=np.int64(14))
