#!/usr/bin/env python3
"""Record the reference interpolators' outputs as tests/golden/interp_ref.npz.

    python tests/golden/make_golden_interp.py /path/to/libinterp_ref.so

The argument is a shared library holding the reference's two interpolation
functions (its src/resample/interpolate.c compiled outside this repository with
the oracle's flags; the one-line command is in DESIGN.md).  The inputs are
slices of tests/golden/lpc_signals.npz and the seeded positions of
tests/interp_util.py; only the reference's outputs are stored.  The file's keys
are listed in tests/interp_util.py.

One property is asserted here, on the CPU: the float32 model of interp_util.py
equals the reference bit for bit on every recorded finite value (and is NaN
where the reference's value is NaN).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from interp_util import InterpApi, METHODS, ROW_N, row, special_row, positions, model, bits, SPECIAL_N  # noqa: E402


def main():
    ref = InterpApi(sys.argv[1])
    arrays = {}
    total = differ = 0
    cases = [(f"n{n}", row(n), positions(n)) for n in ROW_N]
    cases += [(kind, special_row(kind), positions(SPECIAL_N)) for kind in ("inf", "nan")]
    for name, x, pos in cases:
        for method in METHODS:
            got = ref.many(method, x, pos)
            want = model(x, pos, method)
            finite = np.isfinite(got)
            total += got.size
            differ += int(np.sum(bits(got)[finite] != bits(want)[finite]))
            differ += int(np.sum(np.isnan(got) != np.isnan(want)))
            arrays[f"{name}_{method}"] = got
    print(f"float32 model vs reference: {differ} of {total} values differ")
    assert differ == 0, differ
    args = ref.argument_cases()
    names = sorted(args)
    arrays["arg_names"] = np.array(names)
    arrays["arg_status"] = np.array([args[k] for k in names], np.int64)
    path = os.path.join(HERE, "interp_ref.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
