#!/usr/bin/env python3
"""Record the reference resampler's outputs as tests/golden/resample_*.npz.

    python tests/golden/make_golden_resample.py /path/to/libvvresample_ref.so

The argument is a shared library holding the reference's vv_dsp_resampler_*
(its src/resample/resampler.c + interpolate.c compiled outside this repository
with the oracle's flags; the one-line command is in DESIGN.md).  Files:

  resample_<num>_<den>.npz  for every ratio of resample_util.RATIOS: the outputs
      for the first 1, 2, 15 and 6000 samples of the input, linear ("n<N>_lin")
      and sinc at 1, 4, 5, 32, 127, 128 and 200 requested taps ("n<N>_sinc<T>":
      values outside 4..128 record the clamping, 5 and 127 the odd-to-even step);
  resample_misc.npz  the seeded uniform [-1, 1) input of 6000 samples ("x"), the
      statuses and out_n of the argument cases ("arg_names", "arg_status",
      "arg_out_n"), and out_n for a list of (in_n, num, den) ("len_cases", "len_out").
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from resample_util import ResamplerApi, RATIOS, TAPS, LENGTHS, LEN_CASES, key  # noqa: E402


def main():
    ref = ResamplerApi(sys.argv[1])
    x = np.random.default_rng(20250).uniform(-1.0, 1.0, 6000).astype(np.float32)
    for num, den in RATIOS:
        arrays = {}
        for n in LENGTHS:
            for taps in [None] + TAPS:
                st, out_n, y = ref.process(x[:n], num, den, taps)
                assert st == 0, (num, den, n, taps, st)
                arrays[key(n, taps)] = y[:out_n].copy()
        np.savez_compressed(os.path.join(HERE, f"resample_{num}_{den}.npz"), **arrays)
    args = ref.argument_cases()
    names = sorted(args)
    len_out = []
    for in_n, num, den in LEN_CASES:   # linear: the length does not depend on the quality
        st, out_n, _ = ref.process(np.zeros(in_n, np.float32), num, den)
        assert st == 0
        len_out.append(out_n)
    np.savez_compressed(os.path.join(HERE, "resample_misc.npz"), x=x, arg_names=np.array(names),
                        arg_status=np.array([args[k][0] for k in names], np.int64),
                        arg_out_n=np.array([args[k][1] for k in names], np.int64),
                        len_cases=np.array(LEN_CASES, np.int64), len_out=np.array(len_out, np.int64))


if __name__ == "__main__":
    main()
