"""Shared pieces of the filter-module tests (biquad IIR, Savitzky-Golay): a ctypes
binding of vv_dsp_biquad_* / vv_dsp_iir_apply / vv_dsp_savgol (the product
library and, in tests/golden/make_golden_filter.py, a compiled reference), the
cascades and cases of the fixtures, the argument cases both are put through,
and models of the cascade: float32 with the reference's operation order
(bit-exact, checked against the fixture in tests/test_filter_host.py) and f64.

Fixture layout (tests/golden/):
  iir_signal.npz   "x": 6600 float32 samples of noise, peak 0.5 (the fixture row
                   is x[:6000]); "nan_at": index of the NaN in the NaN row
  iir_ref.npz      per cascade c in "abcd": "<c>_sos" [stages][5] b0 b1 b2 a1 a2,
                   "<c>_y" / "<c>_z" the reference's output and final states
                   [stages][2] from zero state, "<c>_z_cut<k>" the final states of
                   the same row streamed in calls of k samples (the outputs were
                   bit-identical to "<c>_y" when recorded, as was the in-place
                   call), "<c>_y_nan" the first 128 outputs of the NaN row (all
                   later ones were NaN), "<c>_err_ref" = max|y_ref - y_f64| /
                   max|y_f64|; "mix_y" / "mix_z": biquad_process interleaved with
                   iir_apply (mix_run); "arg_names" / "arg_status"; "dummy"
  iir_f64.npz      "<c>_y": the f64 model's outputs
  savgol_signal.npz "x": 4100 float32 samples; "bad": the NaN / Inf row of 300
  savgol_coeffs.npz "h<i>": the reference's window of SAVGOL_CASES[i]
  savgol_mode<m>.npz "c<i>_n<N>": the reference's output of case i on x[:N]
  savgol_misc.npz  "policy<p>_status" / "policy<p>_y": the NaN-policy cases;
                   "arg_names" / "arg_status"
"""
import ctypes as C
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
SENTINEL = np.float32(-123.0)

IIR_N = 6000
IIR_SIGNAL_N = 6600
IIR_NAN_AT = 100
IIR_CUTS = [1, 7, 64, 1000]
IIR_CASCADES = "abcd"

# (window_length, polyorder, deriv, delta)
SAVGOL_CASES = [(1, 0, 0, 1.0), (3, 1, 0, 1.0), (5, 2, 0, 1.0), (5, 2, 1, 0.5), (11, 3, 2, 0.01), (51, 4, 0, 1.0),
                (257, 5, 0, 1.0), (257, 15, 3, 2.0), (9, 8, 8, 1.0)]
SAVGOL_MODES = [0, 1, 2, 3]          # reflect, constant, nearest, wrap
SAVGOL_SIGNAL_N = 4100
SAVGOL_POLICY_CASE = (11, 3, 0, 1.0, 0)   # window, polyorder, deriv, delta, mode of the NaN-policy rows

_fp = C.POINTER(C.c_float)


def savgol_lengths(m):
    """the row lengths of a case: m, m + 1 (where the reflect and wrap rules bite), 300, 4100"""
    return sorted({n for n in (m, m + 1, 300, SAVGOL_SIGNAL_N) if n >= m})


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------- inputs
def make_iir_signal(seed=7341):
    w = np.random.default_rng(seed).standard_normal(IIR_SIGNAL_N)
    return (0.5 * w / np.abs(w).max()).astype(np.float32)


def make_savgol_signal(seed=9127):
    """noise on a slow sine, so that smoothing and derivatives both have something to show"""
    rng = np.random.default_rng(seed)
    t = np.arange(SAVGOL_SIGNAL_N)
    return (0.4 * np.sin(2.0 * np.pi * t / 180.0) + 0.1 * rng.standard_normal(SAVGOL_SIGNAL_N)).astype(np.float32)


def make_bad_row(x):
    """300 samples with a NaN, a +Inf and a -Inf"""
    bad = x[:300].copy()
    bad[50] = np.nan
    bad[120] = np.inf
    bad[200] = -np.inf
    return bad


def _pole_pair(r, hz, fs=16000.0):
    th = 2.0 * math.pi * hz / fs
    return -2.0 * r * math.cos(th), r * r


def make_cascades():
    """name -> sos [stages][5] float32 (b0 b1 b2 a1 a2)"""
    a = []
    for r, hz in ((0.80, 1000.0), (0.86, 1200.0), (0.92, 1400.0), (0.98, 1600.0)):
        a1, a2 = _pole_pair(r, hz)
        g = (1.0 + a1 + a2) / 4.0                     # unit gain at DC, zeros at z = -1
        a.append([g, 2.0 * g, g, a1, a2])
    a1, a2 = _pole_pair(0.999, 440.0)
    g = (1.0 - 0.999 * 0.999) / 2.0
    b = [[g, 0.0, -g, a1, a2]]
    c = [[1.0, -1.0, 0.0, -0.995, 0.0]]                # first-order DC blocker
    d = []
    for hz, db, q in ((500.0, 6.0, 2.0), (3000.0, -4.0, 1.0)):   # peaking equalisers
        amp = 10.0 ** (db / 40.0)
        w0 = 2.0 * math.pi * hz / 16000.0
        al = math.sin(w0) / (2.0 * q)
        a0 = 1.0 + al / amp
        d.append([(1.0 + al * amp) / a0, -2.0 * math.cos(w0) / a0, (1.0 - al * amp) / a0, -2.0 * math.cos(w0) / a0,
                  (1.0 - al / amp) / a0])
    return {k: np.array(v, np.float32) for k, v in zip(IIR_CASCADES, (a, b, c, d))}


# ------------------------------------------------------------- models
def cascade_model(sos, x, state=None, dtype=np.float32):
    """Direct Form II Transposed per stage over rows x (..., n), every operation
    rounded to `dtype` in the reference's order (iir.c:23-25): float32 is
    bit-exact to it, float64 is the exact-arithmetic yardstick.  state
    (..., stages, 2) or None -> (y, final state)."""
    sos = np.asarray(sos, np.float32).astype(dtype)
    x = np.asarray(x).astype(dtype)
    lead = x.shape[:-1]
    z = np.zeros(lead + (len(sos), 2), dtype) if state is None else np.array(state, dtype)
    y = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(x.shape[-1]):
            v = x[..., i]
            for s, (b0, b1, b2, a1, a2) in enumerate(sos):
                out = b0 * v + z[..., s, 0]
                z[..., s, 0] = (b1 * v - a1 * out) + z[..., s, 1]
                z[..., s, 1] = b2 * v - a2 * out
                v = out
            y[..., i] = v
    return y, z


def savgol_pad(x, half, mode):
    """rows x (..., n) with `half` samples added on either side by the reference's
    rules (savgol.c:164-203): REFLECT mirrors about the edge sample without
    repeating it, CONSTANT and NEAREST repeat the edge sample, WRAP continues
    circularly on the right and with x[(n - (i mod n) - 1) mod n] on the left"""
    n = x.shape[-1]
    i = np.arange(half)
    if mode == 0:
        left, right = np.minimum(i + 1, n - 1), (n - 2 - i if n >= 2 else np.full(half, n - 1))
    elif mode == 3:
        left, right = (n - (i % n) - 1) % n, i % n
    else:
        left, right = np.zeros(half, np.int64), np.full(half, n - 1)
    return np.concatenate([x[..., left[::-1]], x, x[..., right]], axis=-1)


def savgol_model(x, h, mode):
    """the reference's convolution (savgol.c:205-217) on rows x (..., n): f64
    products (exact) added in window order, rounded once -- bit-exact to it"""
    m = len(h)
    xp = savgol_pad(np.asarray(x, np.float32), m // 2, mode).astype(np.float64)
    n = x.shape[-1]
    acc = np.zeros(x.shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(m):
            acc = acc + np.float64(h[k]) * xp[..., k:k + n]
        return acc.astype(np.float32)


def mix_run(api, sos, x):
    """vv_dsp_biquad_process interleaved with vv_dsp_iir_apply on one stage:
    3 single samples, a block of 50, 2 single samples -> (outputs[55], state[2])"""
    bq = api.biquads(sos[:1])
    out = [api.process(bq, x[i]) for i in range(3)]
    st, y = api.apply_structs(bq, 1, x[3:53])
    assert st == OK, st
    out += list(y)
    out += [api.process(bq, x[53 + i]) for i in range(2)]
    return np.array(out, np.float32), np.array([bq[0].z1, bq[0].z2], np.float32)


# ------------------------------------------------------------- the C API
class Biquad(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("a1", "a2", "b0", "b1", "b2", "z1", "z2")]


class FilterApi:
    """vv_dsp_biquad_*, vv_dsp_iir_apply, vv_dsp_savgol and the NaN policy of one
    shared library, host pointers."""

    def __init__(self, path_or_lib):
        L = C.CDLL(path_or_lib) if isinstance(path_or_lib, str) else path_or_lib
        L.vv_dsp_biquad_init.argtypes = [C.c_void_p] + [C.c_float] * 5
        L.vv_dsp_biquad_reset.argtypes = [C.c_void_p]
        L.vv_dsp_biquad_reset.restype = None
        L.vv_dsp_biquad_process.argtypes = [C.c_void_p, C.c_float]
        L.vv_dsp_biquad_process.restype = C.c_float
        L.vv_dsp_iir_apply.argtypes = [C.c_void_p, C.c_size_t, _fp, _fp, C.c_size_t]
        L.vv_dsp_savgol.argtypes = [_fp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _fp]
        L.vv_dsp_set_nan_policy.argtypes = [C.c_int]
        L.vv_dsp_set_nan_policy.restype = None
        self.lib = L

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(_fp)

    def biquads(self, sos, state=None):
        arr = (Biquad * max(len(sos), 1))()
        for s, (b0, b1, b2, a1, a2) in enumerate(np.asarray(sos, np.float32)):
            assert self.lib.vv_dsp_biquad_init(C.byref(arr[s]), b0, b1, b2, a1, a2) == OK
            if state is not None:
                arr[s].z1, arr[s].z2 = float(state[s][0]), float(state[s][1])
        return arr

    def apply_structs(self, bq, stages, x, inplace=False):
        x = np.ascontiguousarray(x, np.float32)
        y = x.copy() if inplace else np.full(max(len(x), 1), SENTINEL, np.float32)
        st = self.lib.vv_dsp_iir_apply(C.byref(bq) if bq is not None else None, stages, self._p(y if inplace else x),
                                       self._p(y), len(x))
        return st, y[:len(x)]

    def iir(self, sos, x, state=None, inplace=False):
        """-> (status, y, final state [stages][2])"""
        bq = self.biquads(sos, state)
        st, y = self.apply_structs(bq, len(sos), x, inplace)
        return st, y, np.array([[bq[s].z1, bq[s].z2] for s in range(len(sos))], np.float32).reshape(len(sos), 2)

    def process(self, bq, x):
        return np.float32(self.lib.vv_dsp_biquad_process(C.byref(bq), float(x)))

    def savgol(self, x, m, p, deriv, delta, mode):
        x = np.ascontiguousarray(x, np.float32)
        y = np.full(max(len(x), 1), SENTINEL, np.float32)
        return self.lib.vv_dsp_savgol(self._p(x), len(x), m, p, deriv, delta, mode, self._p(y)), y[:len(x)]

    def savgol_window(self, m, p, deriv, delta):
        """the window a library convolves with, read off its response to a unit
        sample in the middle of a row of 3 m (each output is one exact product)"""
        n, c, half = 3 * m, (3 * m) // 2, m // 2
        x = np.zeros(n, np.float32)
        x[c] = 1.0
        st, y = self.savgol(x, m, p, deriv, delta, 1)
        return st, y[c + half - np.arange(m)]

    def set_nan_policy(self, policy):
        self.lib.vv_dsp_set_nan_policy(policy)

    def iir_argument_cases(self, device=True):
        """name -> status.  Names ending in _dev reach the computation (a device in
        the product library) and are left out with device=False."""
        L = self.lib
        x = np.linspace(-1.0, 1.0, 8).astype(np.float32)
        y = np.zeros(8, np.float32)
        bq = self.biquads(make_cascades()["c"])
        xp, yp = self._p(x), self._p(y)
        res = {
            "init_null": L.vv_dsp_biquad_init(None, 1.0, 0.0, 0.0, 0.0, 0.0),
            "init_ok": L.vv_dsp_biquad_init(C.byref(bq[0]), 1.0, -1.0, 0.0, -0.995, 0.0),
            "apply_null_in": L.vv_dsp_iir_apply(C.byref(bq), 1, None, yp, 8),
            "apply_null_out": L.vv_dsp_iir_apply(C.byref(bq), 1, xp, None, 8),
            "apply_null_biquads": L.vv_dsp_iir_apply(None, 1, xp, yp, 8),
            "apply_null_in_n0": L.vv_dsp_iir_apply(C.byref(bq), 1, None, yp, 0),     # pointers come first
            "apply_null_biquads_stages0_n0": L.vv_dsp_iir_apply(None, 0, xp, yp, 0),
            "apply_n0": L.vv_dsp_iir_apply(C.byref(bq), 1, xp, yp, 0),
        }
        if device:
            res["apply_ok_dev"] = L.vv_dsp_iir_apply(C.byref(bq), 1, xp, yp, 8)
            res["apply_stages0_dev"] = L.vv_dsp_iir_apply(None, 0, xp, yp, 8)
        return res

    def savgol_argument_cases(self, device=True):
        L = self.lib
        x = np.linspace(-1.0, 1.0, 300).astype(np.float32)
        y = np.zeros(300, np.float32)
        xp, yp = self._p(x), self._p(y)
        res = {
            "null_in": L.vv_dsp_savgol(None, 300, 5, 2, 0, 1.0, 0, yp),
            "null_out": L.vv_dsp_savgol(xp, 300, 5, 2, 0, 1.0, 0, None),
            "null_in_n0": L.vv_dsp_savgol(None, 0, 5, 2, 0, 1.0, 0, yp),            # pointers come first
            "n0": L.vv_dsp_savgol(xp, 0, 5, 2, 0, 1.0, 0, yp),
            "n0_even_window": L.vv_dsp_savgol(xp, 0, 4, 2, 0, 1.0, 0, yp),          # the size comes first
            "window_even": L.vv_dsp_savgol(xp, 300, 6, 2, 0, 1.0, 0, yp),
            "window_zero": L.vv_dsp_savgol(xp, 300, 0, 2, 0, 1.0, 0, yp),
            "window_negative": L.vv_dsp_savgol(xp, 300, -3, 2, 0, 1.0, 0, yp),
            "polyorder_negative": L.vv_dsp_savgol(xp, 300, 5, -1, 0, 1.0, 0, yp),
            "deriv_negative": L.vv_dsp_savgol(xp, 300, 5, 2, -1, 1.0, 0, yp),
            "deriv_gt_polyorder": L.vv_dsp_savgol(xp, 300, 5, 2, 3, 1.0, 0, yp),
            "window_gt_n": L.vv_dsp_savgol(xp, 7, 9, 2, 0, 1.0, 0, yp),
            "window_gt_n_deriv_gt_polyorder": L.vv_dsp_savgol(xp, 7, 9, 2, 3, 1.0, 0, yp),   # range before size
            "delta_zero_deriv1": L.vv_dsp_savgol(xp, 300, 5, 2, 1, 0.0, 0, yp),
            "delta_negative_deriv1": L.vv_dsp_savgol(xp, 300, 5, 2, 1, -1.0, 0, yp),
            "delta_nan_deriv1": L.vv_dsp_savgol(xp, 300, 5, 2, 1, float("nan"), 0, yp),
            "window_gt_n_delta_zero": L.vv_dsp_savgol(xp, 3, 5, 2, 1, 0.0, 0, yp),  # size before delta
            "polyorder_16": L.vv_dsp_savgol(xp, 300, 33, 16, 0, 1.0, 0, yp),
            "polyorder_16_deriv2": L.vv_dsp_savgol(xp, 300, 33, 16, 2, 1.0, 0, yp),
            "window_259": L.vv_dsp_savgol(xp, 300, 259, 3, 0, 1.0, 0, yp),
        }
        if device:
            res["delta_zero_deriv0_dev"] = L.vv_dsp_savgol(xp, 300, 5, 2, 0, 0.0, 0, yp)   # delta unused
            res["ok_dev"] = L.vv_dsp_savgol(xp, 300, 5, 2, 1, 0.5, 3, yp)
            res["window_eq_n_dev"] = L.vv_dsp_savgol(xp, 9, 9, 2, 0, 1.0, 0, yp)
        return res
