#!/usr/bin/env python3
"""Record the reference LPC's outputs as tests/golden/lpc_*.npz.

    python tests/golden/make_golden_lpc.py /path/to/liblpc_ref.so

The argument is a shared library holding the reference's vv_dsp_autocorr,
vv_dsp_levinson, vv_dsp_lpc and vv_dsp_lpspec (its src/envelope/lpc.c compiled
outside this repository with the oracle's flags; the one-line command is in
DESIGN.md).  The files and their keys are listed in tests/lpc_util.py.  The
"1 + sum" spectra are the reference called with a[1..] negated.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from lpc_util import (LpcApi, CASES, SPEC_NFFT, SPEC_GAIN, key, make_signals, case_rows, autocorr_f64,  # noqa: E402
                      lpspec_f64)


def main():
    ref = LpcApi(sys.argv[1])
    white, resonant = make_signals()
    np.savez_compressed(os.path.join(HERE, "lpc_signals.npz"), white=white, resonant=resonant)

    arrays = {}
    for n, order in CASES:
        x = case_rows(white, resonant, n)
        got = {k: [] for k in ("r_ref", "a_ref", "err_ref", "lpc_a_ref", "lpc_err_ref")}
        for row in x:
            st, r = ref.autocorr(row, order)
            assert st == 0, (n, order, st)
            st, a, err = ref.levinson(r)
            assert st == 0, (n, order, st)
            st, la, lerr = ref.lpc(row, order)
            assert st == 0, (n, order, st)
            for k, v in zip(got, (r, a, err, la, lerr)):
                got[k].append(v)
        arrays[key(n, order, "x")] = x
        arrays[key(n, order, "r_f64")] = autocorr_f64(x, order)
        for k, v in got.items():
            arrays[key(n, order, k)] = np.array(v, np.float32)
    deg = np.array([[0.0] + [0.1] * 16, [-1.0] + [0.1] * 16], np.float32)
    for r in deg:
        assert ref.levinson(r)[0] == 4
    args = ref.argument_cases()
    names = sorted(args)
    np.savez_compressed(os.path.join(HERE, "lpc_cases.npz"), deg_r=deg, arg_names=np.array(names),
                        arg_status=np.array([args[k] for k in names], np.int64), **arrays)

    # coefficient rows: order 0, order 16 from both signals, order 32 (resonant)
    coef = [np.ones(1, np.float32), arrays[key(400, 16, "lpc_a_ref")][0], arrays[key(400, 16, "lpc_a_ref")][5],
            arrays[key(1024, 32, "lpc_a_ref")][5]]
    spec = {f"a{i}": a for i, a in enumerate(coef)}
    spec["gain"] = np.array(SPEC_GAIN, np.float32)
    for nfft in SPEC_NFFT:
        for sign in (0, 1):
            mag_ref, mag_f64 = [], []
            for a, g in zip(coef, spec["gain"]):
                arg = a.copy()
                if sign:
                    arg[1:] = -arg[1:]
                st, mag = ref.lpspec(arg, float(g), nfft)
                assert st == 0
                mag_ref.append(mag)
                mag_f64.append(lpspec_f64(a, g, nfft, sign))
            spec[f"mag_ref_s{sign}_{nfft}"] = np.array(mag_ref, np.float32)
            spec[f"mag_f64_s{sign}_{nfft}"] = np.array(mag_f64, np.float64)
    np.savez_compressed(os.path.join(HERE, "lpc_spec.npz"), **spec)


if __name__ == "__main__":
    main()
