"""Shared pieces of the statistics tests: a ctypes binding of the fifteen
functions of vv_dsp/core/stats.h (the product library and, in
tests/golden/make_golden_stats.py, a compiled reference), the fixture cases,
the argument cases both are put through, and f64 models.

The signals are tests/golden/lpc_signals.npz ("white", "resonant"); only the
reference's outputs are stored.

Fixture layout (tests/golden/stats_*.npz):
  stats_rows.npz   per n of ROW_N, key "n<n>_<name>": the reference's value of
                   statistic <name> (STAT_NAMES) for the SLICES rows of rows(n),
                   float32 or int64; a size-rule failure is stored as NaN;
                   "long_<name>": the same for long_row(); "edge<n>_<case>_<name>"
                   for the rows of edge_rows(n), n in EDGE_N
  stats_corr.npz   "auto_<n>_<r_len>_<biased>" and "cross_<nx>_<ny>_<r_len>": r
  stats_args.npz   "arg_names" / "arg_status": the argument cases by name
"""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

STAT_NAMES = ("sum", "mean", "var", "rms", "min", "max", "crest", "skewness", "kurtosis", "zero_crossings", "argmin",
              "argmax")
COUNT_NAMES = ("zero_crossings", "argmin", "argmax")
EXACT_NAMES = ("min", "max", "zero_crossings", "argmin", "argmax")
F64_NAMES = ("sum", "rms", "var", "skewness", "kurtosis")       # <= 1 ulp; mean and crest derive from them
ENERGY_NAMES = ("rms", "min", "max", "crest", "zero_crossings", "argmin", "argmax")
MIN_LEN = {"var": 2, "skewness": 3, "kurtosis": 4}

ROW_N = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 400, 1024, 4096, 4097]
BATCH = 67
SLICE_STARTS = [0, 1600, 3200]      # recorded rows 0-2 white, 3-5 resonant
SLICES = 6
CHUNK = 4096                        # the kernels' chunk (vv_dsp_amd.h)
LONG_N = 3 * CHUNK + 17
AUTO_CASES = [(1, 1), (8, 12), (64, 64), (65, 17), (400, 401), (4097, 33)]
CROSS_CASES = [(1, 1, 1), (8, 5, 7), (5, 8, 8), (64, 65, 65), (400, 400, 400), (4097, 1000, 33)]
SENTINEL = np.float32(-123.0)
SENTINEL_IDX = 987654321

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)

_fp = C.POINTER(C.c_float)
_zp = C.POINTER(C.c_size_t)


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def signals():
    z = load("lpc_signals")
    return z["white"], z["resonant"]


def valid_names(n):
    return tuple(k for k in STAT_NAMES if n >= MIN_LEN.get(k, 1))


# ------------------------------------------------------------- inputs
def rows(n, white=None, resonant=None):
    """the SLICES recorded rows of length n: [SLICES][n] float32"""
    if white is None:
        white, resonant = signals()
    return np.stack([sig[s:s + n] for sig in (white, resonant) for s in SLICE_STARTS]).astype(np.float32)


def batch_rows(n, batch=None):
    """[batch][n]: the recorded rows over and over (row j is recorded row j % SLICES), so the
    reference's value of every row of a batch is known"""
    r = rows(n)
    return r[np.arange(BATCH if batch is None else batch) % SLICES]


def long_row(white=None):
    if white is None:
        white = signals()[0]
    return np.ascontiguousarray(white[:LONG_N])


def edge_rows(n):
    """name -> row of length n (n = 400 or 4097) whose result is decided at a lane,
    wave or chunk boundary, or by a special value"""
    white = signals()[0]
    base = white[100:100 + n].copy()
    e = {}
    e["const"] = np.full(n, 0.1, np.float32)
    e["zeros"] = np.zeros(n, np.float32)
    # the extreme value several times, first at index 63 / 64 boundary positions
    t = base.copy()
    t[[64, 65, 127, 128, n - 1]] = 0.75
    t[[63, 129, 256, n - 2]] = -0.75
    e["ties"] = t
    # +0 / -0: every sample is a zero, so min = max = x[0]'s bits whatever comes later
    z = np.zeros(n, np.float32)
    z[[1, 63, 64, 65, 128, n - 1]] = -0.0
    e["zeros_pm"] = z
    z2 = z.copy()
    z2[0] = -0.0
    z2[[2, 66]] = 0.0
    e["zeros_mp"] = z2
    # zeros as the extreme among positive (negative) samples: the first zero of either sign wins
    p = np.abs(base) + np.float32(0.01)
    p[[63, 64, 200]] = [-0.0, 0.0, -0.0]
    e["zero_min"] = p
    q = -p
    q[[63, 64, 200]] = [0.0, -0.0, 0.0]
    e["zero_max"] = q
    a = base.copy()
    a[0] = np.nan
    e["nan_first"] = a
    b = base.copy()
    b[[70, 128]] = np.nan
    e["nan_mid"] = b
    # alternating signs except for equal-sign pairs, so crossings fall on 63|64, 64|65 and on
    # every chunk boundary but not on 62|63 or 65|66; one +, 0, - that counts none
    s = np.where(np.arange(n) % 2 == 0, 0.25, -0.25).astype(np.float32)
    s[62] = s[63]
    s[66] = s[65]
    for c in range(CHUNK, n, CHUNK):
        s[c - 2] = s[c - 1]
    s[301] = 0.0
    s[302] = -0.25
    e["alternate"] = s
    return e


EDGE_N = (400, 4097)


# ------------------------------------------------------------- f64 models
def f32_ulps(a, b):
    """distance in float32 steps between equal-shaped float32 arrays (NaN == NaN: 0)"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def model(x):
    """name -> value of one row: sums in f64 (two passes about mean = sum / n),
    rounded to float32 once; the derived values in float32 as the reference forms
    them; the exact class by numpy on rows without NaN."""
    x = np.asarray(x, np.float32)
    n = len(x)
    xd = x.astype(np.float64)
    s = np.sum(xd)
    d = xd - s / n
    var = np.sum(d * d) / n
    res = {"sum": np.float32(s), "rms": np.float32(np.sqrt(np.sum(xd * xd) / n)), "var": np.float32(var)}
    res["mean"] = np.float32(res["sum"] / np.float32(n))
    res["skewness"] = np.float32((np.sum(d * d * d) / n) / var ** 1.5) if var > 0 else np.float32(0)
    res["kurtosis"] = np.float32((np.sum(d * d * d * d) / n) / (var * var) - 3.0) if var > 0 else np.float32(0)
    mn, mx = x.min(), x.max()
    res["min"], res["max"] = mn, mx
    peak = mx if mx > -mn else -mn
    with np.errstate(divide="ignore", invalid="ignore"):
        res["crest"] = np.float32(np.inf) if res["rms"] == 0 else np.float32(peak / res["rms"])
    res["argmin"], res["argmax"] = int(np.argmin(x)), int(np.argmax(x))
    a, b = x[:-1], x[1:]
    res["zero_crossings"] = int(np.sum(((a > 0) & (b < 0)) | ((a < 0) & (b > 0))))
    return res


def autocorr_model(x, r_len, biased):
    xd = np.asarray(x, np.float64)
    n = len(xd)
    r = np.zeros(r_len, np.float32)
    for lag in range(min(r_len, n)):
        r[lag] = np.float32(np.sum(xd[:n - lag] * xd[lag:]) / (n if biased else n - lag))
    return r


def cross_model(x, y, r_len):
    xd, yd = np.asarray(x, np.float64), np.asarray(y, np.float64)
    r = np.zeros(r_len, np.float32)
    for lag in range(r_len):
        cnt = min(len(xd), len(yd) - lag)
        if cnt > 0:
            r[lag] = np.float32(np.sum(xd[:cnt] * yd[lag:lag + cnt]) / cnt)
    return r


# ------------------------------------------------------------- the C API
REAL_FUNCS = {"sum": "vv_dsp_sum", "mean": "vv_dsp_mean", "var": "vv_dsp_var", "rms": "vv_dsp_rms",
              "min": "vv_dsp_min", "max": "vv_dsp_max", "crest": "vv_dsp_crest_factor",
              "skewness": "vv_dsp_skewness", "kurtosis": "vv_dsp_kurtosis"}
INDEX_FUNCS = {"zero_crossings": "vv_dsp_zero_crossing_rate", "argmin": "vv_dsp_argmin", "argmax": "vv_dsp_argmax"}


class StatsApi:
    """The fifteen functions of vv_dsp/core/stats.h of one shared library, host pointers."""

    def __init__(self, path_or_lib):
        L = C.CDLL(path_or_lib) if isinstance(path_or_lib, str) else path_or_lib
        for f in REAL_FUNCS.values():
            getattr(L, f).argtypes = [_fp, C.c_size_t, _fp]
        for f in INDEX_FUNCS.values():
            getattr(L, f).argtypes = [_fp, C.c_size_t, _zp]
        L.vv_dsp_peak.argtypes = [_fp, C.c_size_t, _fp, _fp]
        L.vv_dsp_autocorrelation.argtypes = [_fp, C.c_size_t, _fp, C.c_size_t, C.c_int]
        L.vv_dsp_cross_correlation.argtypes = [_fp, C.c_size_t, _fp, C.c_size_t, _fp, C.c_size_t]
        self.lib = L

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(_fp)

    def stat(self, name, x, n=None):
        """-> (status, value); the value keeps its sentinel where the call left it untouched"""
        x = np.ascontiguousarray(x, np.float32)
        n = len(x) if n is None else n
        if name in REAL_FUNCS:
            out = np.full(1, SENTINEL, np.float32)
            return getattr(self.lib, REAL_FUNCS[name])(self._p(x), n, self._p(out)), out[0]
        out = C.c_size_t(SENTINEL_IDX)
        return getattr(self.lib, INDEX_FUNCS[name])(self._p(x), n, C.byref(out)), out.value

    def peak(self, x, want_min=True, want_max=True):
        x = np.ascontiguousarray(x, np.float32)
        mn = np.full(1, SENTINEL, np.float32)
        mx = np.full(1, SENTINEL, np.float32)
        st = self.lib.vv_dsp_peak(self._p(x), len(x), self._p(mn) if want_min else None,
                                  self._p(mx) if want_max else None)
        return st, mn[0], mx[0]

    def autocorrelation(self, x, r_len, biased):
        x = np.ascontiguousarray(x, np.float32)
        r = np.full(max(r_len, 1), SENTINEL, np.float32)
        return self.lib.vv_dsp_autocorrelation(self._p(x), len(x), self._p(r), r_len, int(biased)), r[:r_len]

    def cross_correlation(self, x, y, r_len):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        r = np.full(max(r_len, 1), SENTINEL, np.float32)
        return self.lib.vv_dsp_cross_correlation(self._p(x), len(x), self._p(y), len(y), self._p(r), r_len), r[:r_len]

    def all_stats(self, x):
        """name -> the row's value through the single-value calls; NaN where the size rule fails"""
        res = {}
        for name in STAT_NAMES:
            st, v = self.stat(name, x)
            if st == ERR_SIZE and len(x) < MIN_LEN.get(name, 1):
                v = np.float32(np.nan)
            else:
                assert st == OK, (name, len(x), st)
            res[name] = v
        st, mn, mx = self.peak(x)
        assert st == OK and mn.tobytes() == np.float32(res["min"]).tobytes() \
            and mx.tobytes() == np.float32(res["max"]).tobytes()
        return res

    def argument_cases(self, device=True):
        """name -> status.  Names ending in _dev reach the computation (a device in
        the product library) and are left out with device=False."""
        L = self.lib
        x = np.linspace(-1.0, 1.0, 8).astype(np.float32)
        buf = np.zeros(16, np.float32)
        idx = C.c_size_t(0)
        xp, bp, ip = self._p(x), self._p(buf), C.byref(idx)
        res = {}
        for name, f in REAL_FUNCS.items():
            fn = getattr(L, f)
            res[name + "_null_x"] = fn(None, 8, bp)
            res[name + "_null_out"] = fn(xp, 8, None)
            res[name + "_n0"] = fn(xp, 0, bp)
            res[name + "_null_out_n1"] = fn(xp, 1, None)           # pointers come before sizes
            if name in MIN_LEN:
                res[name + "_short"] = fn(xp, MIN_LEN[name] - 1, bp)
                res[name + "_null_x_short"] = fn(None, MIN_LEN[name] - 1, bp)
        for name, f in INDEX_FUNCS.items():
            fn = getattr(L, f)
            res[name + "_null_x"] = fn(None, 8, ip)
            res[name + "_null_out"] = fn(xp, 8, None)
            res[name + "_n0"] = fn(xp, 0, ip)
        res["peak_null_x"] = L.vv_dsp_peak(None, 8, bp, bp)
        res["peak_n0"] = L.vv_dsp_peak(xp, 0, bp, bp)
        res["peak_n0_no_outputs"] = L.vv_dsp_peak(xp, 0, None, None)
        res["peak_no_outputs"] = L.vv_dsp_peak(xp, 8, None, None)
        res["auto_null_x"] = L.vv_dsp_autocorrelation(None, 8, bp, 4, 0)
        res["auto_null_r"] = L.vv_dsp_autocorrelation(xp, 8, None, 4, 0)
        res["auto_n0"] = L.vv_dsp_autocorrelation(xp, 0, bp, 4, 0)
        res["auto_rlen0"] = L.vv_dsp_autocorrelation(xp, 8, bp, 0, 0)
        res["auto_null_r_rlen0"] = L.vv_dsp_autocorrelation(xp, 8, None, 0, 0)
        res["cross_null_x"] = L.vv_dsp_cross_correlation(None, 8, xp, 8, bp, 4)
        res["cross_null_y"] = L.vv_dsp_cross_correlation(xp, 8, None, 8, bp, 4)
        res["cross_null_r"] = L.vv_dsp_cross_correlation(xp, 8, xp, 8, None, 4)
        res["cross_nx0"] = L.vv_dsp_cross_correlation(xp, 0, xp, 8, bp, 4)
        res["cross_ny0"] = L.vv_dsp_cross_correlation(xp, 8, xp, 0, bp, 4)
        res["cross_rlen0"] = L.vv_dsp_cross_correlation(xp, 8, xp, 8, bp, 0)
        res["cross_ny0_rlen0"] = L.vv_dsp_cross_correlation(xp, 8, xp, 0, bp, 0)
        if device:
            for name in STAT_NAMES:
                res[name + "_ok_dev"] = self.stat(name, x)[0]
            res["var_n2_dev"] = self.stat("var", x[:2])[0]
            res["skewness_n3_dev"] = self.stat("skewness", x[:3])[0]
            res["kurtosis_n4_dev"] = self.stat("kurtosis", x[:4])[0]
            res["peak_min_only_dev"] = self.peak(x, True, False)[0]
            res["peak_max_only_dev"] = self.peak(x, False, True)[0]
            res["auto_beyond_n_dev"] = self.autocorrelation(x, 12, 0)[0]
            res["cross_ok_dev"] = self.cross_correlation(x, x[:5], 7)[0]
        return res
