"""Shared pieces of the interpolation tests: a ctypes binding of the two functions
of vv_dsp/resample/interpolate.h (the product library and, in
tests/golden/make_golden_interp.py, a compiled reference), the seeded position
sets, the recorded rows and the NumPy float32 model of both methods.

The signals are slices of tests/golden/lpc_signals.npz; only the reference's
outputs are stored.

Fixture layout (tests/golden/interp_ref.npz):
  "n<n>_<method>"   the reference's value at every position of positions(n) on
                    row(n), n in ROW_N, method in METHODS
  "inf_<method>", "nan_<method>"
                    the same for special_row("inf") / special_row("nan")
                    (SPECIAL_N samples, one of them Inf / NaN)
  "arg_names" / "arg_status"
                    the argument cases of the two scalar functions by name
"""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

LINEAR, CUBIC = 0, 1
METHODS = ("linear", "cubic")
FUNCS = {"linear": "vv_dsp_interpolate_linear_real", "cubic": "vv_dsp_interpolate_cubic_real"}

ROW_N = [1, 2, 3, 4, 5, 257, 4099]
FULL_MAX = 257          # rows up to here record every integer position; longer ones those near the ends
SPECIAL_N = 257
SPECIAL_AT = 100        # index of the Inf / NaN sample
N_RANDOM = 2000
SENTINEL = np.float32(-123.0)

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)

_fp = C.POINTER(C.c_float)
F32 = np.float32


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def signals():
    z = load("lpc_signals")
    return z["white"], z["resonant"]


# ------------------------------------------------------------- inputs
def row(n):
    """the recorded row of length n: white and resonant slices in turn"""
    white, resonant = signals()
    k = ROW_N.index(n)
    sig = (white, resonant)[k % 2]
    return np.ascontiguousarray(sig[300 * k:300 * k + n], np.float32)


def special_row(kind):
    x = signals()[0][1000:1000 + SPECIAL_N].astype(np.float32)
    x[SPECIAL_AT] = np.inf if kind == "inf" else np.nan
    return x


def positions(n):
    """The recorded positions of a row of n samples (float32, no NaN): every integer
    from -2 to n + 1 (rows longer than FULL_MAX: those within 4 of either end), the
    half-integers between them, the floats next to each integer on both sides,
    +-0, +-Inf, +-1e30, and N_RANDOM uniform positions in [-2, n + 1]."""
    if n <= FULL_MAX:
        ints = np.arange(-2, n + 2)
    else:
        ints = np.concatenate([np.arange(-2, 5), np.arange(n - 5, n + 2)])
    fi = ints.astype(np.float32)
    below = np.nextafter(fi, F32(-np.inf))
    above = np.nextafter(fi, F32(np.inf))
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e30, -1e30], np.float32)
    rng = np.random.default_rng(20260 + n)
    rand = rng.uniform(-2.0, n + 1.0, N_RANDOM).astype(np.float32)
    return np.concatenate([fi, fi + F32(0.5), below, above, special, rand]).astype(np.float32)


def warp_positions(n, m, kind, seed=0):
    """m float32 positions on a row of n samples: "warp" a monotone ramp with a slow
    vibrato, "reverse" a ramp from beyond the end down to before the start, "const"
    one fractional position m times, "random" uniform over [-2, n + 1]"""
    k = np.arange(m, dtype=np.float64)
    if kind == "warp":
        p = k * ((n - 1) / max(m - 1, 1)) + 1.7 * np.sin(k * 0.013)
    elif kind == "reverse":
        p = (n + 0.5) - k * ((n + 2.0) / max(m - 1, 1))
    elif kind == "const":
        p = np.full(m, min(n - 1, 2) * 0.37 + (n > 3) * 1.0)
    elif kind == "random":
        p = np.random.default_rng(777 + seed).uniform(-2.0, n + 1.0, m)
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


def uniform_positions(start, step, m):
    """(float)(start + (double)k * step), product and sum rounded separately (NumPy f64)"""
    return (np.float64(start) + np.arange(m, dtype=np.float64) * np.float64(step)).astype(np.float32)


# ------------------------------------------------------------- the float32 model
def model(x, pos, method):
    """interpolate.c:4-64 per position in float32, every product and sum rounded on its
    own (NumPy float32 arithmetic does); a NaN position gives NaN"""
    x = np.asarray(x, np.float32)
    pos = np.asarray(pos, np.float32)
    n = len(x)
    cubic = method in (CUBIC, "cubic")
    out = np.empty(len(pos), np.float32)
    if cubic and n < 2:
        out[:] = x[0]
        return out
    max_index = F32(n - 1)
    lo = pos <= 0
    hi = ~lo & (pos >= max_index)
    nan = np.isnan(pos)
    inside = ~(lo | hi | nan)
    out[lo] = x[0]
    out[hi] = x[n - 1]
    out[nan] = np.nan
    p = pos[inside]
    i = np.floor(p).astype(np.int64)
    t = p - i.astype(np.float32)
    assert t.dtype == np.float32
    i2 = np.minimum(i + 1, n - 1)
    with np.errstate(all="ignore"):
        if not cubic:
            out[inside] = (F32(1) - t) * x[i] + t * x[i2]
            return out
        p0, p1, p2, p3 = x[np.maximum(i - 1, 0)], x[i], x[i2], x[np.minimum(i + 2, n - 1)]
        m1 = F32(0.5) * (p2 - p0)
        m2 = F32(0.5) * (p3 - p1)
        t2 = t * t
        t3 = t2 * t
        h00 = F32(2) * t3 - F32(3) * t2 + F32(1)
        h10 = t3 - F32(2) * t2 + t
        h01 = -F32(2) * t3 + F32(3) * t2
        h11 = t3 - t2
        res = h00 * p1 + h10 * m1 + h01 * p2 + h11 * m2
    assert res.dtype == np.float32
    out[inside] = res
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b, nan_equal=False):
    """bit for bit; nan_equal: any NaN equals any NaN"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    eq = bits(a) == bits(b)
    if nan_equal:
        eq |= np.isnan(a) & np.isnan(b)
    return bool(np.all(eq))


# ------------------------------------------------------------- the C API
class InterpApi:
    """The two functions of vv_dsp/resample/interpolate.h of one shared library, host pointers."""

    def __init__(self, path_or_lib):
        L = C.CDLL(path_or_lib) if isinstance(path_or_lib, str) else path_or_lib
        for f in FUNCS.values():
            getattr(L, f).argtypes = [_fp, C.c_size_t, C.c_float, _fp]
            getattr(L, f).restype = C.c_int
        self.lib = L

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(_fp)

    def one(self, method, x, pos, n=None):
        """-> (status, value); the value keeps its sentinel where the call left it untouched"""
        x = np.ascontiguousarray(x, np.float32)
        out = np.full(1, SENTINEL, np.float32)
        st = getattr(self.lib, FUNCS[method])(self._p(x), len(x) if n is None else n, C.c_float(float(pos)),
                                              self._p(out))
        return st, out[0]

    def many(self, method, x, pos):
        x = np.ascontiguousarray(x, np.float32)
        fn = getattr(self.lib, FUNCS[method])
        out = np.full(len(pos), SENTINEL, np.float32)
        xp, n = self._p(x), len(x)
        for k, p in enumerate(pos):
            st = fn(xp, n, C.c_float(float(p)), out[k:].ctypes.data_as(_fp))
            assert st == OK, (method, n, float(p), st)
        return out

    def argument_cases(self, device=True):
        """name -> status.  Names ending in _dev reach the computation (a device in
        the product library) and are left out with device=False."""
        x = np.linspace(-1.0, 1.0, 8).astype(np.float32)
        out = np.zeros(1, np.float32)
        xp, op = self._p(x), self._p(out)
        res = {}
        for method, f in FUNCS.items():
            fn = getattr(self.lib, f)
            res[method + "_null_x"] = fn(None, 8, 1.5, op)
            res[method + "_null_out"] = fn(xp, 8, 1.5, None)
            res[method + "_n0"] = fn(xp, 0, 1.5, op)
            res[method + "_null_x_n0"] = fn(None, 0, 1.5, op)          # pointers come before sizes
            res[method + "_null_out_n0"] = fn(xp, 0, 1.5, None)
            if device:
                res[method + "_ok_dev"] = fn(xp, 8, 1.5, op)
                res[method + "_n1_dev"] = fn(xp, 1, 0.5, op)
                res[method + "_beyond_dev"] = fn(xp, 8, 1e30, op)
        return res
