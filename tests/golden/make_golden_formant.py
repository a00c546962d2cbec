"""Writes tests/golden/formant_signal.npz: the signal of tests/formant_util.py's
make_fixture_signal (0.25 s at 16 kHz, a seeded pulse train through four
two-pole resonators) with its design.

    python tests/golden/make_golden_formant.py

  "signal"   4000 float32 samples, peak 0.5
  "design"   [4][2] float64: frequency and bandwidth in Hz of each resonator
  "fs", "f0" the sample rate and the pulse rate in Hz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import formant_util as fu  # noqa: E402

if __name__ == "__main__":
    sig = fu.make_fixture_signal()
    np.savez_compressed(os.path.join(HERE, "formant_signal.npz"), signal=sig,
                        design=np.array(fu.FIXTURE_FORMANTS, np.float64), fs=np.float64(fu.FIXTURE_FS),
                        f0=np.float64(fu.FIXTURE_F0))
    print("formant_signal.npz:", sig.shape, sig.dtype, float(np.abs(sig).max()))
