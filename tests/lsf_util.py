"""Shared pieces of the LSF and formant tests: the numpy model of
include/vv_dsp/envelope/lsf.h in two forms (row by row, and vectorised over
rows of one order), the case table both test sets run, and a ctypes binding of
the host-row calls.

Every model operation is one IEEE f64 operation in the header's order, so the
GPU kernels can be held to it bit for bit wherever no math-library function
(acos) stands between.  The grid constant CG is read from the header.
"""
import ctypes as C
import os
import re

import numpy as np

import lpc_util
from frames_util import hamming

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vv_dsp", "envelope", "lsf.h")

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
STABLE, COMPLETE = 1, 2
G = 256
BISECTIONS = 32
ORDERS = (1, 2, 3, 8, 15, 16, 31, 32)
QNAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def header_cg():
    with open(HEADER) as f:
        m = re.search(r"#define\s+VV_DSP_LSF_CG\s+(\S+)", f.read())
    return float.fromhex(m.group(1))


def grid():
    cg = np.float64(header_cg())
    x = np.empty(G + 1, np.float64)
    x[0] = 1.0
    x[1] = cg
    for i in range(2, G):
        x[i] = (2.0 * cg) * x[i - 1] - x[i - 2]
    x[G] = -1.0
    return x


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


# ------------------------------------------------------------- the case table
def levinson_f64(r, order):
    a = np.zeros(order + 1)
    a[0] = 1.0
    e = r[0]
    for m in range(1, order + 1):
        k = -(r[m] + np.dot(a[1:m], r[m - 1:0:-1])) / e
        a[1:m] = a[1:m] + k * a[m - 1:0:-1]
        a[m] = k
        e *= 1.0 - k * k
    return a


_signals = None


def signal_rows(order, starts=(0, 3200, 6400)):
    """Levinson rows (f64, rounded to float) of Hamming frames of 400 of the LPC fixture"""
    global _signals
    if _signals is None:
        _signals = lpc_util.load("lpc_signals")
    w = hamming(400).astype(np.float64)
    rows = {}
    for name in ("white", "resonant"):
        for s in starts:
            x = _signals[name][s:s + 400].astype(np.float64) * w
            rows[f"{name}{s}"] = levinson_f64(lpc_util.autocorr_f64(x, order), order).astype(np.float32)
    return rows


def cases(order):
    """name -> float32 row a[order + 1]; ORDINARY names the rows that have an independent truth"""
    rows = signal_rows(order)
    base = rows["resonant0"]
    p = order
    if p >= 2:
        # neighbouring LSFs 1e-3 rad apart: a pair in an otherwise even spread
        w = np.pi * np.arange(1, p + 1) / (p + 1)
        w[p // 2] = w[p // 2 - 1] + 1e-3
        rows["twotone"] = lsf_to_lpc_row(w.astype(np.float32))
    unit = np.zeros(p + 1, np.float32)
    unit[0] = 1.0
    rows["unit"] = unit
    rows["outside"] = (base.astype(np.float64) * 1.2 ** np.arange(p + 1)).astype(np.float32)
    last0 = base.copy()
    last0[p] = 0.0
    rows["lastzero"] = last0
    dbl = unit.copy()   # (1 - z^-1/2)^2: a double root, and a (p-2)-fold root at 0
    dbl[1:min(p, 2) + 1] = [-1.0, 0.25][:min(p, 2)]
    rows["double"] = dbl
    nan = base.copy()
    nan[(p + 1) // 2] = np.nan
    rows["nan"] = nan
    inf = base.copy()
    inf[1] = np.inf
    rows["inf"] = inf
    return rows


def ordinary(name):
    return name.startswith(("white", "resonant", "twotone"))


def header_hex(name):
    with open(HEADER) as f:
        m = re.search(r"#define\s+" + name + r"\s+(\S+)", f.read())
    return float.fromhex(m.group(1))


def cos_def(w):
    """the header's cosine of float64 values, by arithmetic alone (any shape)"""
    hi, lo = np.float64(header_hex("VV_DSP_LSF_PIO2_HI")), np.float64(header_hex("VV_DSP_LSF_PIO2_LO"))
    C = [np.float64(1.0)]
    for i in range(1, 12):
        C.append(-C[i - 1] / np.float64((2 * i) * (2 * i + 1)))
    w = np.asarray(w, np.float64)
    with np.errstate(all="ignore"):
        t = (w - hi) - lo
        s = t * t
        q = np.full_like(t, C[11])
        for i in range(10, -1, -1):
            q = q * s + C[i]
        return -(t * q)


# ------------------------------------------------------------- row-wise model
def clenshaw(c, x):
    x2 = 2.0 * x
    b1 = np.float64(0.0)
    b2 = np.float64(0.0)
    for n in range(len(c) - 1, 0, -1):
        b = (x2 * b1 - b2) + c[n]
        b2 = b1
        b1 = b
    return (x * b1 - b2) + c[0]


def step_down_row(a):
    p = len(a) - 1
    c = np.asarray(a, np.float64).copy()
    rc = np.full(p, QNAN32, np.float32)
    with np.errstate(all="ignore"):
        for m in range(p, 0, -1):
            k = c[m]
            rc[m - 1] = QNAN32 if k != k else np.float32(k)
            if not abs(k) < 1.0:
                return rc, False
            den = 1.0 - k * k
            new = c.copy()
            for i in range(1, m):
                new[i] = (c[i] - k * c[m - i]) / den
            c = new
    return rc, True


def series_row(a):
    """the two Chebyshev series c1, c2 of a row"""
    p = len(a) - 1
    ad = np.zeros(p + 2, np.float64)
    ad[0] = 1.0
    ad[1:p + 1] = np.asarray(a[1:], np.float64)
    with np.errstate(all="ignore"):
        P = [ad[k] + ad[p + 1 - k] for k in range(p + 2)]
        Q = [ad[k] - ad[p + 1 - k] for k in range(p + 2)]
        M1, M2 = (p + 1) // 2, p // 2
        f1, f2 = [], []
        if p % 2 == 0:
            for k in range(M1 + 1):
                f1.append(P[k] - f1[k - 1] if k else P[k])
                f2.append(Q[k] + f2[k - 1] if k else Q[k])
        else:
            f1 = P[:M1 + 1]
            for k in range(M2 + 1):
                f2.append(Q[k] + f2[k - 2] if k >= 2 else Q[k])
        out = []
        for f, M in ((f1, M1), (f2, M2)):
            out.append(np.array([f[M]] + [2.0 * f[M - n] for n in range(1, M + 1)], np.float64))
    return out


def scan_row(c, x):
    """the bisected roots of one series in cell order, and |S| at the bracket ends"""
    with np.errstate(all="ignore"):
        neg = [bool(clenshaw(c, xi) < 0.0) for xi in x]
        roots, ends = [], []
        for i in range(G):
            if neg[i] != neg[i + 1]:
                lo, hi = x[i], x[i + 1]
                ends += [abs(clenshaw(c, lo)), abs(clenshaw(c, hi))]
                for _ in range(BISECTIONS):
                    mid = 0.5 * (lo + hi)
                    if bool(clenshaw(c, mid) < 0.0) == neg[i]:
                        lo = mid
                    else:
                        hi = mid
                roots.append(0.5 * (lo + hi))
    return roots, ends


def lpc_to_lsf_row(a, x=None, info=None):
    """-> lsf[p] float32, rc[p] float32, flags; info (a dict) receives the f64 roots and |S| at the
    bracket ends"""
    x = grid() if x is None else x
    p = len(a) - 1
    rc, stable = step_down_row(a)
    c1, c2 = series_row(a)
    u, e1 = scan_row(c1, x)
    v, e2 = scan_row(c2, x)
    M1, M2 = (p + 1) // 2, p // 2
    complete = len(u) == M1 and len(v) == M2
    if complete:
        complete = all(u[k] > v[k] for k in range(M2)) and all(v[k] > u[k + 1] for k in range(M1 - 1) if k < M2)
    lsf = np.full(p, QNAN32, np.float32)
    if complete:
        lsf[0::2] = np.arccos(np.array(u, np.float64)).astype(np.float32)
        lsf[1::2] = np.arccos(np.array(v, np.float64)).astype(np.float32)
    if info is not None:
        info.update(u=u, v=v, ends=e1 + e2, complete=complete)
    return lsf, rc, (STABLE if stable else 0) | (COMPLETE if complete else 0)


def lsf_to_lpc_row(lsf):
    p = len(lsf)
    with np.errstate(all="ignore"):
        ck = [cos_def(np.float64(v)) for v in np.asarray(lsf, np.float32)]   # one value at a time
        F = [np.zeros(p + 2, np.float64), np.zeros(p + 2, np.float64)]
        F[0][0] = F[1][0] = 1.0
        for k in range(p):
            old = F[k & 1]
            new = np.empty_like(old)
            tc = 2.0 * ck[k]
            for i in range(p + 2):
                o1 = old[i - 1] if i >= 1 else np.float64(0.0)
                o2 = old[i - 2] if i >= 2 else np.float64(0.0)
                new[i] = (old[i] - tc * o1) + o2
            F[k & 1] = new
        a = np.empty(p + 1, np.float32)
        a[0] = 1.0
        for m in range(1, p + 1):
            f1m1 = F[0][m - 1]
            f2m1 = F[1][m - 1]
            f2m2 = F[1][m - 2] if m >= 2 else np.float64(0.0)
            P = F[0][m] if p & 1 else F[0][m] + f1m1
            Q = F[1][m] - f2m2 if p & 1 else F[1][m] - f2m1
            h = 0.5 * (P + Q)
            a[m] = QNAN32 if h != h else np.float32(h)
    return a


# ------------------------------------------------------------- vectorised model
def clenshaw_vec(c, x):
    """c [B, M+1], x [B, ...] -> S of x's shape"""
    ex = (slice(None),) + (None,) * (x.ndim - 1)
    x2 = 2.0 * x
    b1 = np.zeros_like(x)
    b2 = np.zeros_like(x)
    for n in range(c.shape[1] - 1, 0, -1):
        b = (x2 * b1 - b2) + c[:, n][ex]
        b2 = b1
        b1 = b
    return (x * b1 - b2) + c[:, 0][ex]


def step_down_vec(a):
    B, w = a.shape
    p = w - 1
    c = a.astype(np.float64)
    rc = np.full((B, p), QNAN32, np.float32)
    live = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for m in range(p, 0, -1):
            k = c[:, m]
            rc[live, m - 1] = np.where(k != k, QNAN32, k.astype(np.float32))[live]
            live = live & (np.abs(k) < 1.0)
            den = 1.0 - k * k
            new = c.copy()
            new[:, 1:m] = (c[:, 1:m] - k[:, None] * c[:, m - 1:0:-1]) / den[:, None]
            c = np.where(live[:, None], new, c)
    return rc, live


def series_vec(a):
    B, w = a.shape
    p = w - 1
    ad = np.zeros((B, p + 2), np.float64)
    ad[:, 0] = 1.0
    ad[:, 1:p + 1] = a[:, 1:].astype(np.float64)
    M1, M2 = (p + 1) // 2, p // 2
    with np.errstate(all="ignore"):
        P = ad + ad[:, ::-1]
        Q = ad - ad[:, ::-1]
        f1 = np.empty((B, M1 + 1))
        f2 = np.empty((B, M2 + 1))
        if p % 2 == 0:
            for k in range(M1 + 1):
                f1[:, k] = P[:, k] - f1[:, k - 1] if k else P[:, k]
                f2[:, k] = Q[:, k] + f2[:, k - 1] if k else Q[:, k]
        else:
            f1[:] = P[:, :M1 + 1]
            for k in range(M2 + 1):
                f2[:, k] = Q[:, k] + f2[:, k - 2] if k >= 2 else Q[:, k]
        out = []
        for f, M in ((f1, M1), (f2, M2)):
            c = 2.0 * f[:, ::-1]
            c[:, 0] = f[:, M]
            out.append(c)
    return out


def scan_vec(c, M, x):
    """-> ok [B] (exactly M brackets), roots [B, M] (rows not ok: zeros)"""
    B = c.shape[0]
    with np.errstate(all="ignore"):
        neg = clenshaw_vec(c, np.broadcast_to(x, (B, G + 1)).copy()) < 0.0
        br = neg[:, :-1] != neg[:, 1:]
        ok = br.sum(axis=1) == M
        roots = np.zeros((B, M), np.float64)
        if M and ok.any():
            cells = np.nonzero(br[ok])[1].reshape(-1, M)
            lo, hi = x[cells], x[cells + 1]
            nlo = np.take_along_axis(neg[ok], cells, axis=1)
            cc = c[ok]
            for _ in range(BISECTIONS):
                mid = 0.5 * (lo + hi)
                same = (clenshaw_vec(cc, mid) < 0.0) == nlo
                lo = np.where(same, mid, lo)
                hi = np.where(same, hi, mid)
            roots[ok] = 0.5 * (lo + hi)
    return ok, roots


def lpc_to_lsf_vec(a, x=None):
    """rows a [B, p+1] float32 of one order -> lsf [B, p], rc [B, p], flags [B] int32"""
    x = grid() if x is None else x
    a = np.asarray(a, np.float32)
    B, w = a.shape
    p = w - 1
    rc, stable = step_down_vec(a)
    c1, c2 = series_vec(a)
    M1, M2 = (p + 1) // 2, p // 2
    ok1, u = scan_vec(c1, M1, x)
    ok2, v = scan_vec(c2, M2, x)
    complete = ok1 & ok2
    if M2:
        complete &= np.all(u[:, :M2] > v, axis=1)
        n = min(M1 - 1, M2)
        complete &= np.all(v[:, :n] > u[:, 1:n + 1], axis=1)
    lsf = np.full((B, p), QNAN32, np.float32)
    with np.errstate(all="ignore"):
        lu = np.arccos(u).astype(np.float32)
        lv = np.arccos(v).astype(np.float32)
    lsf[:, 0::2] = np.where(complete[:, None], lu, QNAN32)
    lsf[:, 1::2] = np.where(complete[:, None], lv, QNAN32)
    return lsf, rc, (stable * STABLE + complete * COMPLETE).astype(np.int32)


def lsf_to_lpc_vec(lsf):
    lsf = np.asarray(lsf, np.float32)
    B, p = lsf.shape
    with np.errstate(all="ignore"):
        ck = cos_def(lsf.astype(np.float64))
        F = [np.zeros((B, p + 2)), np.zeros((B, p + 2))]
        F[0][:, 0] = F[1][:, 0] = 1.0

        def sh(f, d):
            out = np.zeros_like(f)
            out[:, d:] = f[:, :-d]
            return out
        for k in range(p):
            old = F[k & 1]
            tc = (2.0 * ck[:, k])[:, None]
            F[k & 1] = (old - tc * sh(old, 1)) + sh(old, 2)
        P = F[0] if p & 1 else F[0] + sh(F[0], 1)
        Q = F[1] - sh(F[1], 2) if p & 1 else F[1] - sh(F[1], 1)
        h = (0.5 * (P + Q))[:, :p + 1]
        a = np.where(h != h, QNAN32, h.astype(np.float32))
    a[:, 0] = 1.0
    return a


# ------------------------------------------------------------- the C API
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
SENT = np.float32(-123.0)


class LsfApi:
    """vv_dsp_lpc_to_lsf / vv_dsp_lsf_to_lpc of the product library, host pointers."""

    def __init__(self, path):
        L = C.CDLL(path)
        L.vv_dsp_lpc_to_lsf.argtypes = [_fp, C.c_size_t, _fp, _fp, _ip]
        L.vv_dsp_lsf_to_lpc.argtypes = [_fp, C.c_size_t, _fp]
        L.vv_dsp_lpc_to_lsf_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        L.vv_dsp_lsf_to_lpc_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.vv_dsp_lsf_frames_device.argtypes = [C.c_void_p] + [C.c_size_t] * 5 + [C.c_int, C.c_void_p, C.c_size_t] + \
            [C.c_void_p] * 5
        L.vv_dsp_amd_last_error.restype = C.c_char_p
        self.lib = L

    def lpc_to_lsf(self, a, order=None, want=("lsf", "rc", "flags")):
        a = np.ascontiguousarray(a, np.float32)
        order = len(a) - 1 if order is None else order
        lsf = np.full(max(order, 1), SENT, np.float32)
        rc = np.full(max(order, 1), SENT, np.float32)
        flags = np.full(1, -77, np.int32)
        st = self.lib.vv_dsp_lpc_to_lsf(a.ctypes.data_as(_fp), order,
                                        lsf.ctypes.data_as(_fp) if "lsf" in want else None,
                                        rc.ctypes.data_as(_fp) if "rc" in want else None,
                                        flags.ctypes.data_as(_ip) if "flags" in want else None)
        return st, lsf, rc, flags

    def lsf_to_lpc(self, lsf, order=None):
        lsf = np.ascontiguousarray(lsf, np.float32)
        order = len(lsf) if order is None else order
        a = np.full(max(order, 0) + 1, SENT, np.float32)
        return self.lib.vv_dsp_lsf_to_lpc(lsf.ctypes.data_as(_fp), order, a.ctypes.data_as(_fp)), a


# ------------------------------------------------------------- comparisons of the GPU tests
def assert_bits(got, want, what):
    gb, wb = bits(np.asarray(got)), bits(np.asarray(want).astype(np.asarray(got).dtype))
    assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
    assert np.array_equal(gb, wb), (what, np.argwhere(gb != wb)[:6].tolist())


def assert_adjacent(got, want, what):
    """float32 arrays equal or adjacent floats; NaNs in the same places and the quiet NaN bit for
    bit.  -> (number of exact values, number one ulp off)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN places", np.argwhere(gn != wn)[:6].tolist())
    assert np.all(bits(got)[gn] == 0x7FC00000) and np.all(bits(want)[wn] == 0x7FC00000), (what, "NaN bits")

    def ordered(x):   # floats as integers in value order
        i = bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    d = np.abs(ordered(got[~gn]) - ordered(want[~gn]))
    assert np.all(d <= 1), (what, int(d.max()), np.argwhere(d > 1)[:6].tolist())
    return int(np.sum(d == 0)), int(np.sum(d == 1))
