"""Shared pieces of the formant tests: the numpy model of
include/vv_dsp/features/formant.h in two forms (row by row, and vectorised over
rows of one order), the design of the formant fixture and a ctypes binding of
the host calls.

Every model operation is one IEEE f64 operation in the header's order; the
start points are read from the library (vv_dsp_formant_start_points), so the
model and the kernels cannot differ by a math library's last bit there.  atan2
and log stand between the roots and freq / bw.
"""
import ctypes as C
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
CONVERGED = 1
MAX_ITER = 48
TWO_PI = 6.283185307179586
QNAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
QNAN64 = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]

# the fixture: a pulse train through four two-pole resonators (Hz, Hz)
FIXTURE_FS = 16000
FIXTURE_F0 = 125.0
FIXTURE_FORMANTS = ((700.0, 80.0), (1220.0, 90.0), (2600.0, 120.0), (3500.0, 150.0))


class FormantParams(C.Structure):
    _fields_ = [("sample_rate", C.c_float), ("f_min", C.c_float), ("f_max", C.c_float), ("bw_max", C.c_float),
                ("n_formants", C.c_uint32)]


class FormantOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("freq", "bw", "count", "flags", "roots")]


def default_params(fs=16000.0, **kw):
    fs = np.float32(fs)
    p = FormantParams(fs, 50.0, np.float32(fs / np.float32(2.0)) - np.float32(50.0), 600.0, 5)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def load_fixture():
    with np.load(os.path.join(GOLDEN, "formant_signal.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def make_fixture_signal(seed=20261):
    """0.25 s at 16 kHz: a pulse train at FIXTURE_F0 with seeded amplitude jitter and a little
    seeded noise, through the cascade of FIXTURE_FORMANTS' two-pole resonators; peak 0.5, float32"""
    n = FIXTURE_FS // 4
    rng = np.random.default_rng(seed)
    x = 1e-3 * rng.standard_normal(n)
    period = int(round(FIXTURE_FS / FIXTURE_F0))
    x[::period] += 1.0 + 0.1 * rng.standard_normal(len(x[::period]))
    y = x
    for f, bw in FIXTURE_FORMANTS:
        r = math.exp(-math.pi * bw / FIXTURE_FS)
        c1, c2 = -2.0 * r * math.cos(2.0 * math.pi * f / FIXTURE_FS), r * r
        out = np.zeros(n)
        for i in range(n):
            out[i] = y[i] - c1 * (out[i - 1] if i >= 1 else 0.0) - c2 * (out[i - 2] if i >= 2 else 0.0)
        y = out
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


# ------------------------------------------------------------- complex arithmetic in real operations
def cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def cdiv(xr, xi, ur, ui):
    n = ur * ur + ui * ui
    return (xr * ur + xi * ui) / n, (xi * ur - xr * ui) / n


# ------------------------------------------------------------- row-wise model
def aberth_row(a, start, info=None):
    """a[p+1] float32, start [p, 2] -> roots [p, 2] f64, converged; info receives the iteration count"""
    p = len(a) - 1
    ad = np.asarray(a, np.float64)
    z = np.array(start, np.float64).copy()
    one, zero = np.float64(1.0), np.float64(0.0)
    if not np.any(ad[1:] != 0.0):
        if info is not None:
            info["iters"] = 0
        return z, True
    with np.errstate(all="ignore"):
        for it in range(MAX_ITER):
            new = z.copy()
            small, bad = True, False
            for i in range(p):
                zr, zi = z[i]
                br, bi, dr, di = one, zero, zero, zero
                for m in range(1, p + 1):
                    tr, ti = cmul(dr, di, zr, zi)
                    dr, di = tr + br, ti + bi
                    br, bi = cmul(br, bi, zr, zi)
                    br = br + ad[m]
                wr, wi = cdiv(br, bi, dr, di)
                sr, si = zero, zero
                for j in range(p):
                    if j != i:
                        rr, ri = cdiv(one, zero, zr - z[j][0], zi - z[j][1])
                        sr, si = sr + rr, si + ri
                tr, ti = cmul(wr, wi, sr, si)
                er, ei = cdiv(wr, wi, one - tr, -ti)
                new[i] = (zr - er, zi - ei)
                bad = bad or not (np.isfinite(er) and np.isfinite(ei))
                small = small and bool(er * er + ei * ei < 1e-26)
            z = new
            if info is not None:
                info["iters"] = it + 1
            if bad:
                return np.full((p, 2), QNAN64), False
            if small:
                return z, True
    return z, False


def candidates_row(z, converged, silent, prm):
    """-> freq[n], bw[n] float32, count; plus the f64 candidates kept (f, bw, im) for the decidability test"""
    nf = prm.n_formants
    freq = np.full(nf, QNAN32, np.float32)
    bw = np.full(nf, QNAN32, np.float32)
    kept = []
    if converged and not silent:
        with np.errstate(all="ignore"):
            c = np.float64(prm.sample_rate) / TWO_PI
            for i, (re, im) in enumerate(z):
                if im > 0.0:
                    f = np.arctan2(im, re) * c
                    b = -(np.log(re * re + im * im) * c)
                    if f >= np.float64(prm.f_min) and f <= np.float64(prm.f_max) and b > 0.0 and \
                            b <= np.float64(prm.bw_max):
                        kept.append((f, i, b, im))
    kept.sort(key=lambda t: (t[0], t[1]))
    count = min(len(kept), nf)
    for k in range(count):
        freq[k] = np.float32(kept[k][0])
        bw[k] = np.float32(kept[k][2])
    return freq, bw, count, kept


def formants_row(a, start, prm, info=None):
    """-> dict freq, bw, count, flags, roots of one row"""
    silent = not np.any(np.asarray(a[1:], np.float64) != 0.0)
    z, conv = aberth_row(a, start, info)
    freq, bw, count, kept = candidates_row(z, conv, silent, prm)
    if info is not None:
        info["kept"] = kept
    return {"freq": freq, "bw": bw, "count": np.int32(count), "flags": np.int32(CONVERGED if conv else 0), "roots": z}


# ------------------------------------------------------------- vectorised model
def aberth_vec(a, start):
    """a [B, p+1] float32 -> roots [B, p, 2], converged [B], iterations [B]"""
    a = np.asarray(a, np.float32)
    B, w = a.shape
    p = w - 1
    ad = a.astype(np.float64)
    zr = np.broadcast_to(np.asarray(start, np.float64)[:, 0], (B, p)).copy()
    zi = np.broadcast_to(np.asarray(start, np.float64)[:, 1], (B, p)).copy()
    silent = ~np.any(ad[:, 1:] != 0.0, axis=1)
    done = silent.copy()
    conv = silent.copy()
    failed = np.zeros(B, bool)
    iters = np.zeros(B, np.int64)
    idx = np.arange(p)
    with np.errstate(all="ignore"):
        for it in range(MAX_ITER):
            if done.all():
                break
            br, bi = np.ones((B, p)), np.zeros((B, p))
            dr, di = np.zeros((B, p)), np.zeros((B, p))
            for m in range(1, p + 1):
                tr, ti = cmul(dr, di, zr, zi)
                dr, di = tr + br, ti + bi
                br, bi = cmul(br, bi, zr, zi)
                br = br + ad[:, m][:, None]
            wr, wi = cdiv(br, bi, dr, di)
            sr, si = np.zeros((B, p)), np.zeros((B, p))
            for j in range(p):
                rr, ri = cdiv(1.0, 0.0, zr - zr[:, j][:, None], zi - zi[:, j][:, None])
                keep = (idx != j)[None, :]
                sr = np.where(keep, sr + rr, sr)
                si = np.where(keep, si + ri, si)
            tr, ti = cmul(wr, wi, sr, si)
            er, ei = cdiv(wr, wi, 1.0 - tr, -ti)
            bad = np.any(~(np.isfinite(er) & np.isfinite(ei)), axis=1)
            small = np.all(er * er + ei * ei < 1e-26, axis=1)
            run = ~done
            zr = np.where(run[:, None], zr - er, zr)
            zi = np.where(run[:, None], zi - ei, zi)
            iters += run
            failed |= run & bad
            conv |= run & ~bad & small
            done |= run & (bad | small)
    roots = np.stack([zr, zi], axis=-1)
    roots[failed] = QNAN64
    return roots, conv, iters


def formants_vec(a, start, prm):
    a = np.asarray(a, np.float32)
    B, w = a.shape
    p = w - 1
    nf = prm.n_formants
    roots, conv, iters = aberth_vec(a, start)
    silent = ~np.any(a[:, 1:].astype(np.float64) != 0.0, axis=1)
    re, im = roots[..., 0], roots[..., 1]
    with np.errstate(all="ignore"):
        c = np.float64(prm.sample_rate) / TWO_PI
        f = np.arctan2(im, re) * c
        b = -(np.log(re * re + im * im) * c)
        kept = (conv & ~silent)[:, None] & (im > 0.0) & (f >= np.float64(prm.f_min)) & (f <= np.float64(prm.f_max)) & \
            (b > 0.0) & (b <= np.float64(prm.bw_max))
    key = np.where(kept, f, np.inf)
    order = np.argsort(key, axis=1, kind="stable")
    nk = kept.sum(axis=1)
    count = np.minimum(nk, nf).astype(np.int32)
    freq = np.full((B, nf), QNAN32, np.float32)
    bw = np.full((B, nf), QNAN32, np.float32)
    for k in range(min(nf, p)):
        sel = k < count
        src = order[:, k]
        freq[sel, k] = f[np.arange(B), src][sel].astype(np.float32)
        bw[sel, k] = b[np.arange(B), src][sel].astype(np.float32)
    return {"freq": freq, "bw": bw, "count": count, "flags": (conv * CONVERGED).astype(np.int32), "roots": roots,
            "iters": iters}


# ------------------------------------------------------------- the C API
_fp = C.POINTER(C.c_float)


class FormantApi:
    def __init__(self, path):
        L = C.CDLL(path)
        L.vv_dsp_formant_params_default.argtypes = [C.c_float, C.POINTER(FormantParams)]
        L.vv_dsp_formant_start_points.argtypes = [C.c_size_t, C.c_void_p]
        L.vv_dsp_lpc_formants.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(FormantParams), C.POINTER(FormantOut)]
        L.vv_dsp_lpc_formants_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 C.POINTER(FormantParams), C.POINTER(FormantOut), C.c_void_p]
        L.vv_dsp_formants_frames_device.argtypes = [C.c_void_p] + [C.c_size_t] * 5 + \
            [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(FormantParams), C.POINTER(FormantOut), C.c_void_p]
        L.vv_dsp_amd_last_error.restype = C.c_char_p
        self.lib = L

    def start_points(self, order):
        out = np.full((max(order, 1), 2), -123.0, np.float64)
        st = self.lib.vv_dsp_formant_start_points(order, out.ctypes.data)
        return st, out

    def start(self, order):
        st, out = self.start_points(order)
        assert st == OK
        return out

    def formants(self, a, prm, order=None, want=("freq", "bw", "count", "flags", "roots")):
        """one host row -> status, dict of arrays (sentinels where not written)"""
        a = np.ascontiguousarray(a, np.float32)
        order = len(a) - 1 if order is None else order
        nf = prm.n_formants if 1 <= prm.n_formants <= 16 else 16
        res = {"freq": np.full(nf, -123.0, np.float32), "bw": np.full(nf, -123.0, np.float32),
               "count": np.full(1, -77, np.int32), "flags": np.full(1, -77, np.int32),
               "roots": np.full((min(max(order, 1), 64), 2), -123.0, np.float64)}
        out = FormantOut(*[res[n].ctypes.data if n in want else None for n in ("freq", "bw", "count", "flags", "roots")])
        return self.lib.vv_dsp_lpc_formants(a.ctypes.data, order, C.byref(prm), C.byref(out)), res
