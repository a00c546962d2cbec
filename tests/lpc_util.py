"""Shared pieces of the LPC tests: a ctypes binding of vv_dsp_autocorr /
_levinson / _lpc / _lpspec (the product library and, in
tests/golden/make_golden_lpc.py, a compiled reference), the fixture cases,
the argument cases both are put through, and f64 models of the sums.

Fixture layout (tests/golden/lpc_*.npz):
  lpc_signals.npz  "white", "resonant": 16000 float32 samples, peak 0.5
  lpc_cases.npz    per case (n, order), key prefix c<n>_<order>_: "x" the 10 rows
                   (5 slices of each signal every 1600 samples, white first, times
                   a Hamming window), "r_ref", "r_f64", "a_ref" / "err_ref" (the
                   reference's levinson on r_ref), "lpc_a_ref" / "lpc_err_ref";
                   "deg_r": Levinson rows with r[0] = 0 and r[0] < 0;
                   "arg_names" / "arg_status": the argument cases by name
  lpc_spec.npz     "a<i>": coefficient row i, "gain": one gain per row, and per
                   nfft "mag_ref_s<sign>_<nfft>" / "mag_f64_s<sign>_<nfft>" [rows][nfft]
"""
import ctypes as C
import math
import os

import numpy as np

from frames_util import hamming

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

CASES = [(1, 0), (2, 1), (33, 32), (64, 1), (65, 16), (320, 12), (400, 16), (1024, 32), (600, 128), (4100, 40)]
GENERIC_CASES = [(600, 128), (4100, 40)]       # beyond the wave kernel's order / length
ROW_STARTS = [0, 1600, 3200, 4800, 6400]       # per signal: rows 0-4 white, 5-9 resonant
WHITE_ROWS = slice(0, 5)
SPEC_NFFT = [1, 2, 64, 400, 512, 2048]
SPEC_GAIN = [1.0, 0.37, 1.0, 1.0]              # one non-unit gain
SENTINEL = np.float32(-123.0)

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)

_fp = C.POINTER(C.c_float)


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def key(n, order, what):
    return f"c{n}_{order}_{what}"


# ------------------------------------------------------------- inputs
def make_signals(seed=20260):
    """white Gaussian noise, and the same noise through a 4-pole resonator (poles of
    radius 0.9 at 700 and 2300 Hz of 16 kHz); both scaled to peak 0.5, float32"""
    w = np.random.default_rng(seed).standard_normal(16000)
    den = np.array([1.0])
    for f in (700.0, 2300.0):
        th = 2.0 * math.pi * f / 16000.0
        den = np.convolve(den, [1.0, -2.0 * 0.9 * math.cos(th), 0.81])
    y = np.zeros(len(w))
    for i in range(len(w)):
        acc = w[i]
        for j in range(1, 5):
            if i - j >= 0:
                acc -= den[j] * y[i - j]
        y[i] = acc
    return ((0.5 * w / np.abs(w).max()).astype(np.float32), (0.5 * y / np.abs(y).max()).astype(np.float32))


def case_rows(white, resonant, n):
    w = hamming(n)
    return np.stack([sig[s:s + n] * w for sig in (white, resonant) for s in ROW_STARTS]).astype(np.float32)


# ------------------------------------------------------------- f64 models
def autocorr_f64(x, order):
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    return np.stack([np.sum(x[..., :n - k] * x[..., k:], axis=-1) for k in range(order + 1)], axis=-1)


def lpspec_f64(a, gain, nfft, plus):
    """gain / |1 -+ sum a[m] e^(-j 2 pi m k / nfft)| with the residue (m k) mod nfft exact"""
    a = np.asarray(a, np.float64)
    k = np.arange(nfft, dtype=np.int64)
    re = np.ones(nfft)
    im = np.zeros(nfft)
    for m in range(1, len(a)):
        ang = 2.0 * np.pi * ((m * k) % nfft).astype(np.float64) / nfft
        am = a[m] if plus else -a[m]
        re = re + am * np.cos(ang)
        im = im + am * np.sin(ang)
    den = np.sqrt(re * re + im * im)
    return np.where(den > 0, float(gain) / np.where(den > 0, den, 1.0), 0.0)


# ------------------------------------------------------------- the C API
class LpcApi:
    """vv_dsp_autocorr / _levinson / _lpc / _lpspec of one shared library, host pointers."""

    def __init__(self, path_or_lib):
        L = C.CDLL(path_or_lib) if isinstance(path_or_lib, str) else path_or_lib
        L.vv_dsp_autocorr.argtypes = [_fp, C.c_size_t, C.c_size_t, _fp]
        L.vv_dsp_levinson.argtypes = [_fp, C.c_size_t, _fp, _fp]
        L.vv_dsp_lpc.argtypes = [_fp, C.c_size_t, C.c_size_t, _fp, _fp]
        L.vv_dsp_lpspec.argtypes = [_fp, C.c_size_t, C.c_float, C.c_size_t, _fp]
        self.lib = L

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(_fp)

    def autocorr(self, x, order):
        x = np.ascontiguousarray(x, np.float32)
        r = np.full(order + 1, SENTINEL, np.float32)
        return self.lib.vv_dsp_autocorr(self._p(x), len(x), order, self._p(r)), r

    def levinson(self, r):
        """-> (status, a, err); a and err keep SENTINEL where the call left them untouched"""
        r = np.ascontiguousarray(r, np.float32)
        a = np.full(len(r), SENTINEL, np.float32)
        err = np.full(1, SENTINEL, np.float32)
        return self.lib.vv_dsp_levinson(self._p(r), len(r) - 1, self._p(a), self._p(err)), a, err[0]

    def lpc(self, x, order):
        x = np.ascontiguousarray(x, np.float32)
        a = np.full(order + 1, SENTINEL, np.float32)
        err = np.full(1, SENTINEL, np.float32)
        return self.lib.vv_dsp_lpc(self._p(x), len(x), order, self._p(a), self._p(err)), a, err[0]

    def lpspec(self, a, gain, nfft):
        a = np.ascontiguousarray(a, np.float32)
        mag = np.full(max(nfft, 1), SENTINEL, np.float32)
        return self.lib.vv_dsp_lpspec(self._p(a), len(a) - 1, gain, nfft, self._p(mag)), mag[:nfft]

    def argument_cases(self, device=True):
        """name -> status.  Names ending in _dev reach the computation (a device in
        the product library) and are left out with device=False."""
        L = self.lib
        x = np.linspace(-1.0, 1.0, 8).astype(np.float32)
        buf = np.zeros(8, np.float32)
        one = np.zeros(1, np.float32)
        xp, bp, op = self._p(x), self._p(buf), self._p(one)
        res = {
            "autocorr_null_x": L.vv_dsp_autocorr(None, 8, 2, bp),
            "autocorr_null_r": L.vv_dsp_autocorr(xp, 8, 2, None),
            "autocorr_null_x_n0": L.vv_dsp_autocorr(None, 0, 0, bp),      # pointers come first
            "autocorr_order_eq_n": L.vv_dsp_autocorr(xp, 4, 4, bp),
            "autocorr_n0": L.vv_dsp_autocorr(xp, 0, 0, bp),
            "levinson_null_r": L.vv_dsp_levinson(None, 2, bp, op),
            "levinson_null_a": L.vv_dsp_levinson(xp, 2, None, op),
            "levinson_null_err": L.vv_dsp_levinson(xp, 2, bp, None),
            "levinson_r0_zero": self.levinson(np.array([0.0, 0.5, 0.25], np.float32))[0],
            "levinson_r0_negative": self.levinson(np.array([-1.0, 0.5, 0.25], np.float32))[0],
            "lpc_null_x": L.vv_dsp_lpc(None, 8, 2, bp, op),
            "lpc_null_a": L.vv_dsp_lpc(xp, 8, 2, None, op),
            "lpc_null_err": L.vv_dsp_lpc(xp, 8, 2, bp, None),
            "lpc_null_x_order_eq_n": L.vv_dsp_lpc(None, 4, 4, bp, op),    # pointers come first
            "lpc_order_eq_n": L.vv_dsp_lpc(xp, 4, 4, bp, op),
            "lpc_n0": L.vv_dsp_lpc(xp, 0, 0, bp, op),
            "lpspec_null_a": L.vv_dsp_lpspec(None, 2, 1.0, 8, bp),
            "lpspec_null_mag": L.vv_dsp_lpspec(xp, 2, 1.0, 8, None),
            "lpspec_nfft0": self.lpspec(x[:3], 1.0, 0)[0],
        }
        if device:
            res["autocorr_ok_dev"] = self.autocorr(x, 2)[0]
            res["levinson_order0_dev"] = self.levinson(np.array([2.0], np.float32))[0]
            res["levinson_nan_r0_dev"] = self.levinson(np.array([np.nan, 0.5], np.float32))[0]
            res["lpc_silent_dev"] = self.lpc(np.zeros(8, np.float32), 2)[0]   # r[0] = 0 found on the way
            res["lpc_ok_dev"] = self.lpc(x, 2)[0]
            res["lpspec_order0_dev"] = self.lpspec(np.ones(1, np.float32), 1.0, 4)[0]
        return res
