#!/usr/bin/env python3
"""Writes tests/golden/pitch_signals.npz: "sig" [2][6400] float32 at 16 kHz, the
inputs of the pitch tests (tests/pitch_util.py).  Only the signals are stored --
sin differs across libm builds -- and the f64 model's outputs are computed at
test time.

  channel 0  a harmonic glide: f(t) = 90 (350 / 90)^(t / T) (1 + 0.02 sin(2 pi 5.5 t)),
             phase 2 pi cumsum(f) / fs, harmonics k = 1..4 with amplitudes 1, 0.6,
             0.35, 0.2 and phase offsets 0.7 k, times 0.3, plus 0.01 randn
  channel 1  five segments:
             [0, 1600)     0.4 (sin p + 0.5 sin 2p) at 140 Hz
             [1600, 2400)  exact zeros
             [2400, 4000)  0.2 randn
             [4000, 5600)  0.4 (sin p + 0.3 sin(2p + 1)) at 233.3 Hz, plus 0.002 randn
             [5600, 6400)  1e-3 randn

    python tests/golden/make_golden_pitch.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FS = 16000.0
N = 6400


def main():
    rng = np.random.default_rng(20261020)
    t = np.arange(N) / FS
    T = N / FS
    f = 90.0 * (350.0 / 90.0) ** (t / T) * (1.0 + 0.02 * np.sin(2 * np.pi * 5.5 * t))
    ph = 2 * np.pi * np.cumsum(f) / FS
    ch0 = 0.3 * sum(a * np.sin(k * ph + 0.7 * k) for k, a in ((1, 1.0), (2, 0.6), (3, 0.35), (4, 0.2)))
    ch0 = ch0 + 0.01 * rng.standard_normal(N)

    ch1 = np.zeros(N)
    p = 2 * np.pi * 140.0 * t[:1600]
    ch1[:1600] = 0.4 * (np.sin(p) + 0.5 * np.sin(2 * p))
    ch1[2400:4000] = 0.2 * rng.standard_normal(1600)
    p = 2 * np.pi * 233.3 * t[:1600]
    ch1[4000:5600] = 0.4 * (np.sin(p) + 0.3 * np.sin(2 * p + 1.0)) + 0.002 * rng.standard_normal(1600)
    ch1[5600:] = 1e-3 * rng.standard_normal(800)

    sig = np.stack([ch0, ch1]).astype(np.float32)
    assert np.all(sig[1, 1600:2400] == 0)
    np.savez_compressed(os.path.join(HERE, "pitch_signals.npz"), sig=sig)
    print("pitch_signals.npz", sig.shape, sig.dtype, float(np.abs(sig).max()))


if __name__ == "__main__":
    main()
