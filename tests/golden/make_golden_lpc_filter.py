"""Writes tests/golden/lpc_filter_signal.npz: the synthetic vowel of
tests/lpc_filter_util.py's make_fixture with its LPC rows and gains.

    python tests/golden/make_golden_lpc_filter.py

  "signal"  2400 float32 samples at 16 kHz, peak 0.5: a pulse train gliding from
            120 to 150 Hz plus 1 % noise through four two-pole resonators at
            700 / 1200 / 2600 / 3500 Hz for the first half and 300 / 2300 / 3000 /
            3700 Hz for the second
  "a"       [15][17] float32: the Levinson rows (f64, rounded) of its Hamming
            frames of 400 at hop 160, centred, order 16
  "gain"    [15] float32: sqrt(prediction error / 400) of each frame
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import lpc_filter_util as fu  # noqa: E402

if __name__ == "__main__":
    fix = fu.make_fixture()
    np.savez_compressed(os.path.join(HERE, "lpc_filter_signal.npz"), **fix)
    print("lpc_filter_signal.npz:", {k: (v.shape, str(v.dtype)) for k, v in fix.items()},
          float(np.abs(fix["signal"]).max()))
