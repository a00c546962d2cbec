"""Writes tests/golden/denoise_signal.npz: the behaviour fixture of the noise-suppression
tests (tests/denoise_util.py).  Generated data only: 2.25 s at 16 kHz; bursts of 440 + 880 +
1320 Hz (0.5 / 0.25 / 0.125) are on during the second half of each half second up to 2.0 s,
so the first and the last quarter second hold noise only; white noise of sigma 0.05 runs
throughout.  The clean and the noise part are stored separately.

    python tests/golden/make_golden_denoise.py
"""
import os

import numpy as np

FS = 16000
N = 36000                  # 2.25 s
SIGMA = 0.05
TONES = ((440.0, 0.5), (880.0, 0.25), (1320.0, 0.125))


def make():
    rng = np.random.default_rng(20261021)
    t = np.arange(N) / FS
    on = (np.floor(t * 4.0).astype(np.int64) % 2 == 1) & (t < 2.0)      # [0.25, 0.5), [0.75, 1.0), ...
    clean = sum(a * np.sin(2.0 * np.pi * f * t) for f, a in TONES) * on
    noise = SIGMA * rng.standard_normal(N)
    return clean.astype(np.float32), noise.astype(np.float32)


if __name__ == "__main__":
    clean, noise = make()
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "denoise_signal.npz")
    np.savez_compressed(out, clean=clean, noise=noise, fs=np.array(FS, np.int64))
    print(out, os.path.getsize(out), "bytes")
