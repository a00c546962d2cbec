#!/usr/bin/env python3
"""Record the reference filter module's outputs as tests/golden/iir_*.npz and
savgol_*.npz.

    python tests/golden/make_golden_filter.py /path/to/libfilter_ref.so

The argument is a shared library holding the reference's vv_dsp_biquad_*,
vv_dsp_iir_apply, vv_dsp_savgol, vv_dsp_filter_dummy and its NaN policy (its
src/filter/iir.c, savgol.c, filter.c and src/core/nan_policy.c compiled outside
this repository with the oracle's flags; the one-line command is in DESIGN.md).
The files and their keys are listed in tests/filter_util.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from filter_util import (FilterApi, IIR_N, IIR_NAN_AT, IIR_CUTS, SAVGOL_CASES, SAVGOL_MODES,   # noqa: E402
                         SAVGOL_POLICY_CASE, OK, make_iir_signal, make_savgol_signal, make_bad_row, make_cascades,
                         cascade_model, mix_run, savgol_lengths)


def save(name, **arrays):
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)


def record_iir(ref):
    x = make_iir_signal()
    save("iir_signal", x=x, nan_at=np.array(IIR_NAN_AT))
    row = x[:IIR_N]
    nan_row = row.copy()
    nan_row[IIR_NAN_AT] = np.nan
    out, f64 = {}, {}
    for name, sos in make_cascades().items():
        st, y, z = ref.iir(sos, row)
        assert st == OK
        for cut in IIR_CUTS:                       # the same row as a stream of calls
            bq = ref.biquads(sos)
            parts = [ref.apply_structs(bq, len(sos), row[i:i + cut]) for i in range(0, IIR_N, cut)]
            assert all(p[0] == OK for p in parts) and np.array_equal(np.concatenate([p[1] for p in parts]), y)
            out[f"{name}_z_cut{cut}"] = np.array([[b.z1, b.z2] for b in bq][:len(sos)], np.float32)
        st, y_in, z_in = ref.iir(sos, row, inplace=True)
        assert st == OK and np.array_equal(y_in, y) and np.array_equal(z_in, z)
        st, y_nan, _ = ref.iir(sos, nan_row)
        assert st == OK and np.all(np.isnan(y_nan[IIR_NAN_AT:])) and np.array_equal(y_nan[:IIR_NAN_AT],
                                                                                    y[:IIR_NAN_AT])
        y64, _ = cascade_model(sos, row, dtype=np.float64)
        y32, z32 = cascade_model(sos, row)
        assert np.array_equal(y32, y) and np.array_equal(z32, z)   # the float32 model is the reference, bit for bit
        out[name + "_sos"], out[name + "_y"], out[name + "_z"], out[name + "_y_nan"] = sos, y, z, y_nan[:128]
        out[name + "_err_ref"] = np.array(np.abs(y.astype(np.float64) - y64).max() / np.abs(y64).max())
        f64[name + "_y"] = y64
        print(name, "err_ref", float(out[name + "_err_ref"]))
    out["mix_y"], out["mix_z"] = mix_run(ref, make_cascades()["b"], row)
    args = ref.iir_argument_cases()
    names = sorted(args)
    save("iir_ref", arg_names=np.array(names), arg_status=np.array([args[k] for k in names], np.int64),
         dummy=np.array(ref.lib.vv_dsp_filter_dummy()), **out)
    save("iir_f64", **f64)


def record_savgol(ref):
    x = make_savgol_signal()
    bad = make_bad_row(x)
    save("savgol_signal", x=x, bad=bad)
    coeffs = {}
    for i, (m, p, deriv, delta) in enumerate(SAVGOL_CASES):
        st, h = ref.savgol_window(m, p, deriv, delta)
        assert st == OK, (m, p, deriv, delta, st)
        coeffs[f"h{i}"] = h
    save("savgol_coeffs", **coeffs)
    for mode in SAVGOL_MODES:
        outs = {}
        for i, (m, p, deriv, delta) in enumerate(SAVGOL_CASES):
            for n in savgol_lengths(m):
                st, y = ref.savgol(x[:n], m, p, deriv, delta, mode)
                assert st == OK, (i, n, mode, st)
                outs[f"c{i}_n{n}"] = y
        save(f"savgol_mode{mode}", **outs)
    misc = {}
    m, p, deriv, delta, mode = SAVGOL_POLICY_CASE
    for policy in range(4):
        ref.set_nan_policy(policy)
        st, y = ref.savgol(bad, m, p, deriv, delta, mode)
        misc[f"policy{policy}_status"], misc[f"policy{policy}_y"] = np.array(st), y
    ref.set_nan_policy(0)
    args = ref.savgol_argument_cases()
    names = sorted(args)
    save("savgol_misc", arg_names=np.array(names), arg_status=np.array([args[k] for k in names], np.int64), **misc)


if __name__ == "__main__":
    api = FilterApi(sys.argv[1])
    record_iir(api)
    record_savgol(api)
