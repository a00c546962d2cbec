"""Shared pieces of the spectral shape tests: a ctypes binding of
vv_dsp/features/spectral_shape.h, the f64 model of its definition (plain numpy,
math.fsum sums, flatness from f64 logs), the seeded case table, and the helpers
that say when an exact-class value is undecidable.

Comparison rule.  The kernel adds the same f64 terms as the model in another
order, which moves a sum of K non-negative terms by at most K 2^-53 relative.  So
every f64-class output is the model's float or its neighbour (<= 1 ulp); skewness,
whose signed terms can cancel, passes at <= 1 ulp or <= 1e-9 absolute.  peak_bin
compares floats, no sums: it is equal unless the row holds a NaN (the rule then
depends on where the NaN stands, which the model follows too, so a NaN row is
only flagged, never skipped silently).  The roll-off bin k rests on two
comparisons, C_(k-1) < T and C_k >= T; it is undecidable when |C - T| <= K 2^-50 S0
at either.  Two comparisons cannot change the answer and are left out: at k ==
k_min there is no bin before, and at k == k_max the definition returns k_max
whether or not C_(k_max) reaches T (rolloff = 1 makes T = S0 = C_(k_max), a gap of
exactly 0 that decides nothing).
"""
import ctypes as C
import math

import numpy as np

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
FS = 16000.0
FLOOR = 1e-10
NAMES = ("energy", "centroid", "spread", "skewness", "kurtosis", "flatness", "rolloff", "flux", "crest", "peak_bin")
F64_CLASS = ("energy", "centroid", "spread", "skewness", "kurtosis", "flatness", "flux", "crest")
SENTINEL = np.float32(-123.0)
SENTINEL_BIN = 987654321


class Params(C.Structure):
    """vv_dsp_spectral_shape_params"""
    _fields_ = [("n_fft", C.c_size_t), ("sample_rate", C.c_float), ("magnitude", C.c_int), ("k_min", C.c_size_t),
                ("k_max", C.c_size_t), ("rolloff", C.c_float), ("floor", C.c_float)]


class Values(C.Structure):
    """vv_dsp_spectral_shape_values"""
    _fields_ = [(n, C.c_float) for n in NAMES[:9]] + [("peak_bin", C.c_uint32)]


def params(n_fft, magnitude=0, band=None, rolloff=0.85, floor=FLOOR, fs=FS):
    k_min, k_max = band if band is not None else (0, n_fft // 2)
    return Params(n_fft, fs, magnitude, k_min, k_max, rolloff, floor)


class ShapeApi:
    """vv_dsp_spectral_shape (one row in host memory) of the product library"""

    def __init__(self, path):
        self.lib = L = C.CDLL(path)
        L.vv_dsp_spectral_shape.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(Values)]
        L.vv_dsp_amd_last_error.restype = C.c_char_p

    def row(self, row, prm, prev=None, null_row=False, null_out=False):
        """(status, Values): the struct starts as sentinels, so an untouched one shows"""
        v = Values(*([SENTINEL] * 9), SENTINEL_BIN)
        row = np.ascontiguousarray(row, np.float32)
        prev = None if prev is None else np.ascontiguousarray(prev, np.float32)
        st = self.lib.vv_dsp_spectral_shape(None if null_row else row.ctypes.data,
                                            None if prev is None else prev.ctypes.data,
                                            None if prm is None else C.byref(prm), None if null_out else C.byref(v))
        return st, v


def untouched(v):
    return all(getattr(v, n) == SENTINEL for n in NAMES[:9]) and v.peak_bin == SENTINEL_BIN


# ------------------------------------------------------------- the model
def weights(p, magnitude):
    """float32 weights of float32 powers: sqrtf (numpy's is correctly rounded) with
    `magnitude`; a negative weight counts as a NaN"""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        w = np.sqrt(p) if magnitude else p.copy()
    w[w < 0] = np.nan
    return w


def _fsum(v):
    v = np.asarray(v, np.float64)
    return math.fsum(v.tolist()) if np.all(np.isfinite(v)) else float(np.sum(v))


def model_row(p, q, prm):
    """the definition on one row p (and its predecessor q, or None) in f64: a dict of the
    ten outputs as they are stored (float32 / int), the f64-class values before their
    rounding (`<name>_f64`) and what the decisions rested on"""
    nfft, fs = int(prm.n_fft), float(np.float32(prm.sample_rate))
    k0, k1 = int(prm.k_min), int(prm.k_max)
    K, B = nfft // 2 + 1, k1 - k0 + 1
    w32 = weights(p, prm.magnitude)[k0:k1 + 1]
    w = w32.astype(np.float64)
    k = np.arange(k0, k1 + 1, dtype=np.float64)
    S0 = _fsum(w)
    out = {"energy": S0}
    with np.errstate(all="ignore"):
        c = _fsum(k * w) / S0 if S0 != 0 else 0.0
        out["centroid"] = 0.0 if S0 == 0 else c * fs / nfft
        d = k - c
        m2, m3, m4 = _fsum(d ** 2 * w), _fsum(d ** 3 * w), _fsum(d ** 4 * w)
        var = m2 / S0 if S0 != 0 else 0.0
        sd = math.sqrt(var) if var >= 0 else float("nan")
        out["spread"] = 0.0 if S0 == 0 else sd * fs / nfft
        flat = S0 == 0 or m2 == 0
        out["skewness"] = 0.0 if flat else (m3 / S0) / sd ** 3
        out["kurtosis"] = 0.0 if flat else (m4 / S0) / sd ** 4
        # the bound of the module docstring on what another order moves the skewness by
        out["skew_bound"] = 0.0 if flat or not np.isfinite(S0) else K * 2.0 ** -53 * _fsum(np.abs(d) ** 3 * w) / (S0 * sd ** 3)
        fl32 = np.float32(prm.floor)
        wp = np.where(w32 < fl32, fl32, w32).astype(np.float64)      # a NaN stays
        out["flatness"] = math.exp(_fsum(np.log(wp)) / B) / (_fsum(wp) / B) if np.all(np.isfinite(wp)) else float("nan")
        if q is None:
            out["flux"] = 0.0
        else:
            dq = w - weights(q, prm.magnitude)[k0:k1 + 1].astype(np.float64)
            out["flux"] = math.sqrt(_fsum(dq * dq)) if np.all(np.isfinite(dq)) else float("nan")
        # exact class: the running maximum starts at w[k_min]; a later NaN never replaces it
        if np.isnan(w32[0]):
            peak = 0
        else:
            peak = int(np.argmax(np.where(np.isnan(w32), -np.inf, w32)))
        out["peak_bin"] = k0 + peak
        out["crest"] = 0.0 if S0 == 0 else float(w[peak]) / (S0 / B)
        Cs = np.cumsum(w)
        T = float(np.float32(prm.rolloff)) * S0
        hit = np.nonzero(Cs >= T)[0]
        kr = int(hit[0]) if hit.size else B - 1
        out["rolloff_bin"] = k0 + kr
        out["rolloff"] = (k0 + kr) * fs / nfft
        tol = K * 2.0 ** -50 * S0
        doubt = False
        if np.isfinite(S0) and S0 != 0:
            doubt = (kr > 0 and abs(Cs[kr - 1] - T) <= tol) or (kr < B - 1 and abs(Cs[kr] - T) <= tol)
        out["rolloff_undecidable"] = bool(doubt)
        out["peak_undecidable"] = bool(np.any(np.isnan(w32)))
    for n in F64_CLASS + ("rolloff",):
        out[n + "_f64"] = np.float64(out[n])      # before the one rounding to float
        out[n] = np.float32(out[n])
    return out


def model_rows(rows, prm, rows_per_group=0):
    """the model on rows [r][>= K] float32 -> {name: array [r]}"""
    rows = np.asarray(rows, np.float32)
    K = int(prm.n_fft) // 2 + 1
    rpg = rows_per_group if rows_per_group else max(len(rows), 1)
    res = [model_row(rows[r, :K], None if r % rpg == 0 else rows[r - 1, :K], prm) for r in range(len(rows))]
    return {n: np.array([x[n] for x in res]) for n in (res[0] if res else {})}


def f32_ulps(a, b):
    """distance in float32 steps; NaN against NaN is 0, NaN against a number is huge"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    both = np.isnan(a) & np.isnan(b)
    one = np.isnan(a) ^ np.isnan(b)
    return np.where(both, 0, np.where(one, 1 << 40, d))


def compare(got, want):
    """Asserts the comparison rule of the module docstring on {name: array} of one call
    against model_rows' result; returns {name: (exact, one_ulp)} counts of the f64 class."""
    assert not np.any(want["rolloff_undecidable"]) and not np.any(want["peak_undecidable"])
    assert np.array_equal(np.asarray(got["peak_bin"]).astype(np.int64), want["peak_bin"]), "peak_bin"
    assert np.array_equal(np.asarray(got["rolloff"], np.float32), want["rolloff"]), "rolloff"
    counts = {}
    for n in F64_CLASS:
        u = f32_ulps(got[n], want[n])
        ok = u <= 1
        if n == "skewness":
            ok |= np.abs(np.asarray(got[n], np.float64) - want[n].astype(np.float64)) <= 1e-9
        assert np.all(ok), (n, np.asarray(got[n])[~ok], want[n][~ok])
        counts[n] = (int(np.sum(u == 0)), int(np.sum(u == 1)))
    return counts


# ------------------------------------------------------------- the cases
def case_rows(n_fft, rows, seed):
    """seeded power rows [rows][K] float32: squared noise under a sloping envelope, every
    bin positive, the rows independent (so flux is far from 0)"""
    K = n_fft // 2 + 1
    rng = np.random.default_rng(seed)
    env = 1.0 / (1.0 + np.arange(K) / max(K / 8.0, 1.0)) ** 2
    x = (np.abs(rng.standard_normal((rows, K))) + 0.05) ** 2 * env * rng.uniform(0.5, 2.0, (rows, 1))
    return x.astype(np.float32)


def band_of(kind, n_fft):
    K = n_fft // 2 + 1
    return {"all": (0, K - 1), "lo1": (1, K - 1), "hi2": (0, max(K - 2, 0)), "one": (K // 2, K // 2)}[kind]


# (n_fft, rows, pitch - K or an absolute pitch >= K + 2, base offset in floats, band, magnitude, rolloff, seed).
# K = 2, 3, 64, 65, 66, 129, 257, 513, 8193: one bin per lane and fewer, the step from t = 1 to t = 3
# bins per lane, registers (t <= 9) and LDS (t = 129); pitches K (packed; 16-byte loads only where K
# is a multiple of 4), K + 1 and an offset base (4-byte loads), 544 for n_fft 1024 (16-byte loads).
CASES = [
    (2, 1, 0, 0, "all", 0, 0.85, 101), (2, 7, 1, 0, "one", 1, 0.5, 102),
    (4, 2, 0, 0, "all", 1, 1.0, 103), (4, 7, 1, 1, "lo1", 0, 0.85, 104),
    (126, 1, 0, 0, "all", 0, 0.5, 105), (126, 7, 0, 0, "hi2", 1, 0.85, 106), (126, 2, 1, 0, "lo1", 0, 1.0, 107),
    (128, 7, 0, 0, "all", 0, 0.85, 108), (128, 2, 1, 1, "one", 0, 0.5, 109), (128, 1, 3, 0, "hi2", 1, 1.0, 110),
    (130, 7, 0, 0, "all", 1, 0.85, 111), (130, 2, 2, 0, "lo1", 0, 0.5, 112), (130, 1, 1, 1, "hi2", 1, 1.0, 129),
    (256, 7, 0, 0, "all", 0, 1.0, 113), (256, 1, 1, 0, "hi2", 1, 0.85, 114), (256, 2, 3, 1, "lo1", 1, 0.5, 115),
    (512, 7, 0, 0, "all", 1, 0.5, 116), (512, 2, 1, 0, "one", 0, 0.85, 117), (512, 1, 3, 0, "lo1", 0, 1.0, 118),
    (1024, 7, 0, 0, "all", 0, 0.85, 119), (1024, 7, 544, 0, "all", 1, 0.5, 120), (1024, 2, 1, 0, "hi2", 0, 1.0, 121),
    (1024, 1, 544, 1, "lo1", 1, 0.85, 122), (1024, 7, 544, 0, "one", 0, 0.85, 123), (1024, 2, 544, 0, "hi2", 1, 1.0, 124),
    (16384, 7, 0, 0, "all", 0, 0.85, 125), (16384, 2, 1, 0, "lo1", 1, 0.5, 126), (16384, 1, 3, 0, "hi2", 0, 1.0, 127),
    (16384, 2, 0, 1, "one", 1, 0.85, 128),
]
CASE_IDS = [f"{c[0]}-r{c[1]}-p{c[2]}-o{c[3]}-{c[4]}-{'mag' if c[5] else 'pow'}-{c[6]:g}" for c in CASES]


def case_pitch(case):
    K = case[0] // 2 + 1
    return case[2] if case[2] >= K + 2 else K + case[2]


def case_params(case):
    return params(case[0], case[5], band_of(case[4], case[0]), case[6])


_models = {}


def case_model(i):
    """(rows, model) of CASES[i], computed once and shared; nobody writes to either"""
    if i not in _models:
        case = CASES[i]
        rows = case_rows(case[0], case[1], case[7])
        rows.setflags(write=False)
        _models[i] = (rows, model_rows(rows, case_params(case)))
    return _models[i]
