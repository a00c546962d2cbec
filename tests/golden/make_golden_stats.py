#!/usr/bin/env python3
"""Record the reference statistics' outputs as tests/golden/stats_*.npz.

    python tests/golden/make_golden_stats.py /path/to/libstats_ref.so

The argument is a shared library holding the reference's fifteen statistics
functions (its src/core/core.c, stats.c and fp_env.c compiled outside this
repository with the oracle's flags; the one-line command is in DESIGN.md).
The inputs are slices of tests/golden/lpc_signals.npz; only the reference's
outputs are stored.  The files and their keys are listed in tests/stats_util.py.

Two properties of the fixtures are asserted here, on the CPU: every recorded
|skewness| and |excess kurtosis| of the signal slices (n >= 5) is at least
1e-3, so that 1 ulp of them is a meaningful bound, and the f64 two-pass model
of stats_util.py, rounded to float32, equals the reference bit for bit on
every recorded value of the f64 class.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from stats_util import (StatsApi, STAT_NAMES, COUNT_NAMES, F64_NAMES, ROW_N, AUTO_CASES, CROSS_CASES, EDGE_N,  # noqa: E402
                        rows, long_row, edge_rows, signals, model, autocorr_model, cross_model, f32_ulps)


def record(ref, arrays, prefix, xs, check_model):
    """the reference's value of every statistic for the rows xs -> arrays[prefix + name]"""
    got = {k: [] for k in STAT_NAMES}
    differ = 0
    for x in xs:
        res = ref.all_stats(x)
        for k in STAT_NAMES:
            got[k].append(res[k])
        if check_model:
            m = model(x)
            for k in F64_NAMES + ("mean", "crest"):
                if not np.isnan(res[k]):
                    differ += int(f32_ulps(res[k], m[k]) != 0)
    for k in STAT_NAMES:
        if k in COUNT_NAMES:
            arrays[prefix + k] = np.array([-1 if isinstance(v, np.floating) and np.isnan(v) else v for v in got[k]],
                                          np.int64)
        else:
            arrays[prefix + k] = np.array(got[k], np.float32)
    return differ


def main():
    ref = StatsApi(sys.argv[1])
    white, resonant = signals()

    arrays = {}
    differ, small = 0, np.inf
    for n in ROW_N:
        differ += record(ref, arrays, f"n{n}_", rows(n, white, resonant), True)
        if n >= 5:
            small = min(small, np.abs(arrays[f"n{n}_skewness"]).min(), np.abs(arrays[f"n{n}_kurtosis"]).min())
    differ += record(ref, arrays, "long_", [long_row(white)], True)
    small = min(small, abs(arrays["long_skewness"][0]), abs(arrays["long_kurtosis"][0]))
    print(f"f64 model vs reference: {differ} values differ; smallest |skewness|, |kurtosis| recorded: {small:.3g}")
    assert differ == 0, differ
    assert small >= 1e-3, small
    for n in EDGE_N:
        for name, x in edge_rows(n).items():
            record(ref, arrays, f"edge{n}_{name}_", [x], False)
    np.savez_compressed(os.path.join(HERE, "stats_rows.npz"), **arrays)

    corr = {}
    differ = 0
    for n, r_len in AUTO_CASES:
        for biased in (0, 1):
            st, r = ref.autocorrelation(white[:n], r_len, biased)
            assert st == 0
            differ += int(np.sum(f32_ulps(r, autocorr_model(white[:n], r_len, biased)) != 0))
            corr[f"auto_{n}_{r_len}_{biased}"] = r
    for nx, ny, r_len in CROSS_CASES:
        st, r = ref.cross_correlation(white[:nx], resonant[:ny], r_len)
        assert st == 0
        differ += int(np.sum(f32_ulps(r, cross_model(white[:nx], resonant[:ny], r_len)) != 0))
        corr[f"cross_{nx}_{ny}_{r_len}"] = r
    print(f"correlation model vs reference: {differ} values differ")
    assert differ == 0, differ
    np.savez_compressed(os.path.join(HERE, "stats_corr.npz"), **corr)

    args = ref.argument_cases()
    names = sorted(args)
    np.savez_compressed(os.path.join(HERE, "stats_args.npz"), arg_names=np.array(names),
                        arg_status=np.array([args[k] for k in names], np.int64))


if __name__ == "__main__":
    main()
