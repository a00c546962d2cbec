"""Writes tests/golden/track_signal.npz: the behaviour fixture of the pitch-tracking
tests (tests/track_util.py).  Generated data only: one second at 16 kHz of a 180 -> 220 Hz
glide whose fundamental fades at 3 Hz under a strong second harmonic, with a 1000-sample
gap of noise.  Plain YIN (pitch.h) decides many of its frames an octave off; the tracked
path must not.

    python tests/golden/make_golden_track.py
"""
import os

import numpy as np

FS = 16000.0
N = 16000
GAP = (7000, 8000)


def make():
    rng = np.random.default_rng(20261021)
    t = np.arange(N) / FS
    f = 180.0 + 40.0 * t / t[-1]
    phase = 2.0 * np.pi * np.cumsum(f) / FS
    a1 = 0.30 + 0.28 * np.cos(2.0 * np.pi * 3.0 * t)          # the fundamental fades to 0.02
    x = a1 * np.sin(phase) + 0.8 * np.sin(2.0 * phase + 0.7) + 0.004 * rng.standard_normal(N)
    x[GAP[0]:GAP[1]] = 0.5 * rng.standard_normal(GAP[1] - GAP[0])
    return x.astype(np.float32), f.astype(np.float32)


if __name__ == "__main__":
    sig, f_true = make()
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "track_signal.npz")
    np.savez_compressed(out, sig=sig, f_true=f_true, gap=np.array(GAP, np.int64))
    print(out, os.path.getsize(out), "bytes")
