"""What the phase vocoder tests share: the f64 numpy model of
include/vv_dsp/spectral/phase_vocoder.h (its positions, its values and the order of
its phase sum, whose segment length is read from the header), the plain wrapped
recurrence it is checked against, the comparison rule, the case table and a ctypes
view of the one-call host form.

The rule: a component passes when |got - model| <= 2^-23 m_j, one float ulp of the
f64 magnitude m_j.  The f64 libm and any reordering reach the phase at the 1e-12 rad
level over a few hundred rows, five orders below float's half ulp, so the two sides
can differ only where a rounding boundary is crossed, which costs at most one ulp of
m_j.  m_j == 0 must give exact zeros; where the model is NaN the result is NaN."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
HEADER = os.path.join(ROOT, "include", "vv_dsp", "spectral", "phase_vocoder.h")


def header_constant(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    assert m, name
    return m.group(1)


S = int(header_constant("VV_DSP_PVOC_SEGMENT"))
MAX_FFT = int(header_constant("VV_DSP_PVOC_MAX_FFT"))
NORM_FLOOR = np.float32(header_constant("VV_DSP_PVOC_NORM_FLOOR").rstrip("f"))
RATES = (1.0, 0.5, 0.8, 1.5, 2.0, 1.0 / 3.0)


# ------------------------------------------------------------- positions
def uniform_positions(start, step, m):
    """p_j = start + (double)j * step, the product and the sum rounded separately"""
    return np.float64(start) + np.arange(m, dtype=np.float64) * np.float64(step)


def curve_positions(pos, T):
    """p_j = (double)pos[j] clamped into [0, T], a NaN to 0"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    p = np.where(p >= 0.0, p, 0.0)
    return np.minimum(p, np.float64(T))


def stretch_rows(T, rate):
    """the number of j >= 0 with (double)j * rate < (double)T"""
    m = 0
    while np.float64(m) * np.float64(rate) < np.float64(T):
        m += 1
    return m


# ------------------------------------------------------------- the model
def _planes(D, n_fft):
    """f64 magnitude and phase of bins 0..n_fft/2 of rows D (T, n_fft), with rows T and
    T + 1 (all zero) appended"""
    K = n_fft // 2 + 1
    T = D.shape[0]
    re = np.zeros((T + 2, K))
    im = np.zeros((T + 2, K))
    re[:T] = D[:, :K].real.astype(np.float64)
    im[:T] = D[:, :K].imag.astype(np.float64)
    with np.errstate(all="ignore"):
        mag = np.sqrt(re * re + im * im)
        th = np.arctan2(im, re)
    th[(re == 0) & (im == 0)] = 0.0                      # signed zeros give no +-pi
    bad = ~(np.isfinite(re) & np.isfinite(im))           # neither atan2 nor sqrt of an infinity is a NaN
    th[bad] = np.nan
    mag[bad] = np.nan
    return mag, th


def model(D, n_fft, p, S=S):
    """D (T, n_fft) complex64, p the f64 positions (already inside [0, T]) -> dict:
    out (m, n_fft) complex64 the rows, z (m, K) complex128 the values before rounding,
    mj (m, K) the f64 magnitudes."""
    D = np.asarray(D)
    T, K = D.shape[0], n_fft // 2 + 1
    p = np.asarray(p, np.float64)
    m = len(p)
    assert m == 0 or (p.min() >= 0 and p.max() <= T)
    mag, th = _planes(D, n_fft)
    fl = np.floor(p)
    t0 = fl.astype(np.int64)
    a = (p - fl)[:, None]
    with np.errstate(all="ignore"):
        mj = (1.0 - a) * mag[t0] + a * mag[t0 + 1]
        d = th[t0 + 1] - th[t0]
        A = np.zeros((m, K))
        base = np.zeros(K)
        for j0 in range(0, m, S):
            part = np.zeros(K)
            for j in range(j0, min(m, j0 + S)):
                A[j] = base + part
                part = part + d[j]
            base = base + part
        phi = (th[t0[0]] if m else 0.0) + A
        z = np.empty((m, K), np.complex128)          # the two components apart: no complex product
        z.real = mj * np.cos(phi)
        z.imag = mj * np.sin(phi)
        re32 = z.real.astype(np.float32)
        im32 = z.imag.astype(np.float32)
    zero = (mj == 0) & ~np.isnan(phi)
    re32[zero] = 0.0
    im32[zero] = 0.0
    out = np.zeros((m, n_fft), np.complex64)
    out[:, :K].real = re32
    out[:, :K].imag = im32
    for k in range(1, K):
        if 2 * k < n_fft:
            out[:, n_fft - k] = np.conj(out[:, k])
    return {"out": out, "z": z, "mj": mj}


def recurrence(D, n_fft, hop, p):
    """the usual phase vocoder: the accumulated phase advances by w_k hop plus the
    deviation from it wrapped into [-pi, pi) -> (m, K) complex128"""
    K = n_fft // 2 + 1
    mag, th = _planes(np.asarray(D), n_fft)
    w = 2.0 * np.pi * np.arange(K) * hop / n_fft
    acc = th[int(np.floor(p[0]))].copy()
    z = np.zeros((len(p), K), np.complex128)
    for j, pj in enumerate(p):
        t0 = int(np.floor(pj))
        a = pj - t0
        z[j] = ((1.0 - a) * mag[t0] + a * mag[t0 + 1]) * np.exp(1j * acc)
        dev = th[t0 + 1] - th[t0] - w
        dev = dev - 2.0 * np.pi * np.round(dev / (2.0 * np.pi))
        acc = acc + w + dev
    return z


# ------------------------------------------------------------- the rule
def _mag_full(mj, n_fft):
    """m_j of every bin of a full row: bin n_fft - k has bin k's"""
    K = mj.shape[1]
    full = np.zeros((mj.shape[0], n_fft))
    full[:, :K] = mj
    for k in range(1, K):
        if 2 * k < n_fft:
            full[:, n_fft - k] = mj[:, k]
    return full


def compare(got, mdl, n_fft):
    """got (m, n_fft) complex64 against model() -> (exact, one_ulp, bad) component counts;
    bad counts the components outside the rule"""
    want = mdl["out"]
    assert got.shape == want.shape, (got.shape, want.shape)
    lim = _mag_full(mdl["mj"], n_fft) * 2.0 ** -23
    exact = one = bad = 0
    for g, w in ((got.real, want.real), (got.imag, want.imag)):
        nan = np.isnan(w)
        same = (g == w) & ~nan
        with np.errstate(invalid="ignore"):
            near = ~same & ~nan & (np.abs(g.astype(np.float64) - w.astype(np.float64)) <= lim) & (lim > 0)
        okn = nan & np.isnan(g)
        exact += int(same.sum()) + int(okn.sum())
        one += int(near.sum())
        bad += int((~same & ~near & ~okn).sum())
    return exact, one, bad


def check(got, mdl, n_fft, what=""):
    exact, one, bad = compare(got, mdl, n_fft)
    print(f"pvoc {what}: {exact} exact, {one} within one ulp of m_j, {bad} outside")
    assert bad == 0, (what, exact, one, bad)
    return exact, one


# ------------------------------------------------------------- inputs
def noise_rows(T, n_fft, seed, nch=None):
    """seeded complex64 rows (T, n_fft) or (nch, T, n_fft); every bin is set (the upper
    half is never read and need not be the lower half's mirror)"""
    rng = np.random.default_rng(seed)
    shape = (T, n_fft) if nch is None else (nch, T, n_fft)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


# (n_fft, T, kind, arg, m): kind "u": arg = (start, step); "c": arg = name of a curve.
# Every rate at every row length, m at S - 1, S, S + 1 and 2 S + 1, T from 1 to 160,
# a non-zero start, a last position exactly T, and the three curves.
def _cases():
    cases = []
    for n_fft in (64, 400, 1024, 2):
        for i, rate in enumerate(RATES):
            m = (S - 1, S, S + 1, 2 * S + 1, S + 1, 2 * S + 1)[i]
            T = int(np.ceil((m - 1) * rate)) + 1 + (i % 2)        # the last position stays below T
            cases.append((n_fft, T, "u", (0.0, rate), m))
    cases += [
        (64, 1, "u", (0.0, 0.25), 4), (64, 1, "u", (0.0, 0.5), 3),      # T = 1; the last position is T
        (400, 2, "u", (0.0, 1.0), 3),                                   # the last position is T: a zero row
        (64, 160, "u", (2.5, 1.25), 2 * S + 1), (1024, 40, "u", (3.0, 0.5), 2 * S + 1),   # a non-zero start
        (400, 80, "u", (0.0, 1.0), 81),                                 # rows 0..T, the last one zero
        (64, 50, "c", "clamped", 2 * S + 1), (400, 30, "c", "nan", S + 1), (1024, 40, "c", "backwards", 2 * S + 1),
        (2, 20, "c", "backwards", S),
    ]
    return cases


CASES = _cases()
CASE_IDS = [f"n{c[0]}-T{c[1]}-{c[2]}{c[3] if c[2] == 'c' else '%g_%g' % c[3]}-m{c[4]}" for c in CASES]


def curve(name, T, m, seed=5):
    rng = np.random.default_rng(seed)
    if name == "clamped":          # runs from below 0 to above T
        return np.linspace(-3.0, T + 3.0, m).astype(np.float32)
    if name == "nan":
        pos = np.sort(rng.uniform(0, T, m)).astype(np.float32)
        pos[m // 2] = np.nan
        return pos
    if name == "backwards":
        return np.linspace(T - 0.25, 0.125, m).astype(np.float32)
    raise KeyError(name)


def case_positions(case):
    """(pos float32 or None, p f64) of a case"""
    n_fft, T, kind, arg, m = case
    if kind == "u":
        return None, uniform_positions(arg[0], arg[1], m)
    pos = curve(arg, T, m)
    return pos, curve_positions(pos, T)


# ------------------------------------------------------------- the host form
class PvocApi:
    """vv_dsp_phase_vocoder (one channel in host memory) of the product library"""

    def __init__(self, path):
        self.lib = L = C.CDLL(path)
        L.vv_dsp_phase_vocoder.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.c_size_t,
                                           C.c_void_p]
        L.vv_dsp_amd_last_error.restype = C.c_char_p
        L.vvhip_available.restype = C.c_int

    def run(self, spec, n_fft, start, step, m, T=None, null_in=False, null_out=False):
        """-> (status, out (m, n_fft) complex64 pre-filled with a canary)"""
        spec = np.ascontiguousarray(spec, np.complex64)
        out = np.full((m, n_fft), CANARY, np.complex64)
        st = self.lib.vv_dsp_phase_vocoder(None if null_in else spec.ctypes.data, spec.shape[0] if T is None else T,
                                           n_fft, start, step, m, None if null_out else out.ctypes.data)
        return st, out


CANARY = np.complex64(-7.25 + 3.5j)


def untouched(a):
    return bool(np.all(a == CANARY))
