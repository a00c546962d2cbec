"""Shared pieces of the resampler tests: a ctypes binding of the
vv_dsp_resampler_* C API (the product library and, in
tests/golden/make_golden_resample.py, a compiled reference), the argument
cases both are put through, and a NumPy model of the arithmetic.

The model (used where no fixture could hold the output):
  linear -- pos = (float)((double)k / ratio), the end cases, f32 floor, and
            (1 - t) a + t b with every operation rounded to f32;
  sinc   -- the polyphase table in f64 (sinc rounded to f32 before the Hann
            product, rows divided by their sum, rounded to f32 once), the
            reference's f64 centre floor((double)k / ratio), the row
            rint(frac P), and an f32 running sum over the taps; where the
            quotient fell below an integer (row P) the output is evaluated
            with the reference's own per-output f64 formula (model_exact).
"""
import ctypes as C
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

RATIOS = [(1, 3), (3, 1), (2, 6), (1, 1), (160, 441), (160, 147), (80, 147), (147, 480), (7, 5)]
TAPS = [1, 4, 5, 32, 127, 128, 200]
LENGTHS = [1, 2, 15, 6000]
LEN_CASES = [(1, 160, 441), (2, 160, 441), (2, 3, 1), (1, 3, 1), (15, 7, 5), (6000, 160, 441), (6000, 80, 147),
             (100000, 44100, 48001), (2 ** 24 + 1, 1, 3), (2 ** 24 + 1, 160, 147)]
SENTINEL = 77   # *out_n before a call: shows whether the call wrote it

_fp = C.POINTER(C.c_float)
_szp = C.POINTER(C.c_size_t)


def fixture(num, den):
    with np.load(os.path.join(GOLDEN, f"resample_{num}_{den}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def fixture_misc():
    with np.load(os.path.join(GOLDEN, "resample_misc.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def key(n, taps):
    """Fixture key: taps None = linear."""
    return f"n{n}_lin" if taps is None else f"n{n}_sinc{taps}"


class ResamplerApi:
    """vv_dsp_resampler_* of one shared library, host pointers."""

    def __init__(self, path_or_lib):
        L = C.CDLL(path_or_lib) if isinstance(path_or_lib, str) else path_or_lib
        L.vv_dsp_resampler_create.argtypes = [C.c_uint, C.c_uint]
        L.vv_dsp_resampler_create.restype = C.c_void_p
        L.vv_dsp_resampler_destroy.argtypes = [C.c_void_p]
        L.vv_dsp_resampler_destroy.restype = None
        L.vv_dsp_resampler_set_ratio.argtypes = [C.c_void_p, C.c_uint, C.c_uint]
        L.vv_dsp_resampler_set_quality.argtypes = [C.c_void_p, C.c_int, C.c_uint]
        L.vv_dsp_resampler_process_real.argtypes = [C.c_void_p, _fp, C.c_size_t, _fp, C.c_size_t, _szp]
        self.lib = L

    def process(self, x, num, den, taps=None, cap=None):
        """-> (status, out_n, y[:out_n]); taps None = linear.  cap: out_cap (default: enough)."""
        L = self.lib
        x = np.ascontiguousarray(x, np.float32)
        rs = L.vv_dsp_resampler_create(num, den)
        assert rs
        try:
            if taps is not None:
                assert L.vv_dsp_resampler_set_quality(rs, 1, taps) == 0
            room = int(math.floor(max(len(x) - 1, 0) * (num / den))) + 2 if cap is None else cap
            y = np.full(max(room, 1), np.float32(-123.0), np.float32)
            out_n = C.c_size_t(SENTINEL)
            st = L.vv_dsp_resampler_process_real(rs, x.ctypes.data_as(_fp), len(x), y.ctypes.data_as(_fp), room,
                                                 C.byref(out_n))
            return st, out_n.value, y
        finally:
            L.vv_dsp_resampler_destroy(rs)

    def argument_cases(self):
        """name -> (status, out_n) of the argument checks of resampler.c:16-76, none of
        which reaches the processing loop."""
        L = self.lib
        res = {}
        for name, (a, b) in (("create_num0", (0, 1)), ("create_den0", (1, 0)), ("create_ok", (3, 2))):
            rs = L.vv_dsp_resampler_create(a, b)
            res[name] = (0 if rs else 1, 0)   # 1: NULL
            if rs:
                L.vv_dsp_resampler_destroy(rs)
        L.vv_dsp_resampler_destroy(None)
        rs = L.vv_dsp_resampler_create(1, 3)
        x = np.zeros(16, np.float32)
        y = np.zeros(16, np.float32)
        xp, yp = x.ctypes.data_as(_fp), y.ctypes.data_as(_fp)
        res["set_ratio_null"] = (L.vv_dsp_resampler_set_ratio(None, 1, 2), 0)
        res["set_ratio_num0"] = (L.vv_dsp_resampler_set_ratio(rs, 0, 2), 0)
        res["set_ratio_den0"] = (L.vv_dsp_resampler_set_ratio(rs, 2, 0), 0)
        res["set_ratio_ok"] = (L.vv_dsp_resampler_set_ratio(rs, 1, 3), 0)
        res["set_quality_null"] = (L.vv_dsp_resampler_set_quality(None, 1, 32), 0)
        res["set_quality_taps0"] = (L.vv_dsp_resampler_set_quality(rs, 1, 0), 0)
        res["set_quality_taps1000"] = (L.vv_dsp_resampler_set_quality(rs, 0, 1000), 0)

        def proc(name, rs_, xin, n, yout, cap, with_out_n=True):
            out_n = C.c_size_t(SENTINEL)
            st = L.vv_dsp_resampler_process_real(rs_, xin, n, yout, cap, C.byref(out_n) if with_out_n else None)
            res[name] = (st, out_n.value)

        proc("process_null_rs", None, xp, 16, yp, 16)
        proc("process_null_in", rs, None, 16, yp, 16)
        proc("process_null_out", rs, xp, 16, None, 16)
        proc("process_null_out_n", rs, xp, 16, yp, 16, with_out_n=False)
        proc("process_null_in_empty", rs, None, 0, yp, 16)     # null pointers come before in_n == 0
        proc("process_empty", rs, xp, 0, yp, 0)                # in_n == 0: *out_n = 0, OK
        proc("process_cap_short", rs, xp, 16, yp, 5)           # 16 samples at 1/3 -> 6 outputs
        proc("process_cap_zero", rs, xp, 16, yp, 0)
        L.vv_dsp_resampler_destroy(rs)
        return res


# ---------------------------------------------------------------- the model
def effective_taps(taps):
    taps = min(max(int(taps), 4), 128)
    return taps + (taps & 1)


def model_table(num, den, taps):
    """(P + 1, taps_eff) float32 and the same in float64."""
    taps = effective_taps(taps)
    P = num // math.gcd(num, den)
    cutoff = min(1.0, num / den)
    half = taps // 2
    frac = np.append(np.arange(P, dtype=np.float64) / P, 1.0)
    m = np.arange(taps)
    t = (m - half).astype(np.float64)[None, :] - frac[:, None]
    v = t * cutoff
    pix = math.pi * v
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(v == 0.0, 1.0, np.sin(pix) / pix).astype(np.float32).astype(np.float64)
    w = 0.5 - 0.5 * np.cos((2.0 * math.pi * m) / (taps - 1))
    weight = s * w[None, :]
    wsum = np.zeros(P + 1)
    for j in range(taps):   # the reference's summation order
        wsum = wsum + weight[:, j]
    t64 = weight / wsum[:, None]
    return t64.astype(np.float32), t64


def output_length(n, num, den):
    return 0 if n == 0 else int(math.floor((n - 1) * (num / den))) + 1


def model_centres(num, den, ks):
    """The reference's centre and table row for outputs ks (int64 arrays)."""
    ratio = num / den
    P = num // math.gcd(num, den)
    in_pos = np.asarray(ks, np.float64) / ratio
    centre = np.floor(in_pos)
    row = np.rint((in_pos - centre) * P).astype(np.int64)
    return centre.astype(np.int64), row


def model_sinc(x, num, den, taps, ks=None):
    """Outputs ks (default: all) of the sinc path, f32 table and f32 running sum."""
    x = np.asarray(x, np.float32)
    n = len(x)
    if ks is None:
        ks = np.arange(output_length(n, num, den), dtype=np.int64)
    W, _ = model_table(num, den, taps)
    T = W.shape[1]
    centre, row = model_centres(num, den, ks)
    acc = np.zeros(len(ks), np.float32)
    for m in range(T):
        idx = np.clip(centre + (m - T // 2), 0, n - 1)
        acc = acc + x[idx] * W[row, m]
    low = np.flatnonzero(row == W.shape[0] - 1)
    if len(low):
        acc[low] = model_exact(x, num, den, T, np.asarray(ks)[low])
    return acc


def model_exact(x, num, den, taps, ks):
    """The reference's own per-output evaluation (resampler.c:95-118) in f64.  Used
    where its quotient fell below an integer (fraction ~ 1 - eps): with 4 taps
    and cutoff 1 the Hann window zeroes the one tap whose sinc does not vanish
    there, and the result hangs on eps, which no table row can hold."""
    x = np.asarray(x, np.float32)
    n = len(x)
    ratio = num / den
    cutoff = min(1.0, ratio)
    half = taps // 2
    in_pos = np.asarray(ks, np.float64) / ratio
    centre = np.floor(in_pos).astype(np.int64)
    acc = np.zeros(len(in_pos))
    wsum = np.zeros(len(in_pos))
    for m in range(taps):
        idx = centre + (m - half)
        v = (idx.astype(np.float64) - in_pos) * cutoff
        pix = math.pi * v
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(v == 0.0, 1.0, np.sin(pix) / pix).astype(np.float32).astype(np.float64)
        weight = s * (0.5 - 0.5 * math.cos((2.0 * math.pi * m) / (taps - 1)))
        acc = acc + x[np.clip(idx, 0, n - 1)].astype(np.float64) * weight
        wsum = wsum + weight
    return np.where(wsum != 0.0, acc / np.where(wsum != 0.0, wsum, 1.0), acc).astype(np.float32)


def model_linear(x, num, den, chunk=1 << 22):
    x = np.asarray(x, np.float32)
    n = len(x)
    out_n = output_length(n, num, den)
    ratio = num / den
    y = np.empty(out_n, np.float32)
    max_index = np.float32(n - 1)
    one = np.float32(1.0)
    for k0 in range(0, out_n, chunk):
        k = np.arange(k0, min(k0 + chunk, out_n), dtype=np.float64)
        pos = (k / ratio).astype(np.float32)
        i = np.clip(np.floor(pos), 0, max(n - 2, 0)).astype(np.int64)
        t = pos - i.astype(np.float32)
        a = x[i]
        b = x[np.minimum(i + 1, n - 1)]
        v = (one - t) * a + t * b
        v = np.where(pos <= 0, x[0], v)
        v = np.where(pos >= max_index, x[n - 1], v)
        y[k0:k0 + len(k)] = v
    return y


def within_harness(got, want, rtol=5e-5, atol=5e-5):
    """tests/conftest.py::tolerances as assert_allclose applies it; returns max |diff|."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    d = np.abs(got - want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = d > atol + rtol * np.abs(want)
    assert not bad.any(), (int(bad.sum()), float(d.max()), np.flatnonzero(bad)[:8])
    return float(d.max()) if d.size else 0.0
