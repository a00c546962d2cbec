"""Shared pieces of the pitch tests: a ctypes binding of vv_dsp/features/pitch.h,
the f64 model of its definition (plain numpy, any summation order), the frame
builder of vv_dsp_fetch_frames_device (zero padding / reflection / window), the
decision margin of a frame, and the cases.

The signals are tests/golden/pitch_signals.npz ("sig" [2][6400] float32 at
16 kHz, tests/golden/make_golden_pitch.py); only the signals are stored, the
model's outputs are computed at test time.

Decision margin.  The model's decisions are comparisons of f64 values that
another summation order moves by about W 2^-53 relative.  The margin of a frame
is the smallest relative gap one of its decisions rested on: |d'(tau) - thr| / thr
over the lags scanned, the gaps between neighbours on the descent, at its end and
around the chosen lag (they select the parabolic refinement), and for unvoiced
frames the gap between the two smallest values (exact ties at 1.0, which the
c == 0 rule produces, count as decided).  A frame with margin < MARGIN is
undecidable: two correct implementations may decide it differently, so lag, f0
and aperiodicity are not compared on it.
"""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
FS = 16000.0
MARGIN = 1e-9
SENTINEL = np.float32(-123.0)
SENTINEL_LAG = 987654321
BATCH = 67

# (frame, hop, fmin, fmax, center, window, threshold) -> (tau_min, tau_max, W): the smallest
# shapes that put a lag or a term count on a lane or wave boundary
CASES = [
    ((130, 40, 254.0, 2000.0, 0, None, 0.15), (8, 63, 67)),
    ((130, 40, 250.0, 2000.0, 0, None, 0.15), (8, 64, 66)),
    ((130, 40, 247.0, 2000.0, 0, None, 0.15), (8, 65, 65)),
    ((65, 40, 250.0, 2000.0, 0, None, 0.15), (8, 64, 1)),
    ((257, 64, 125.0, 1000.0, 1, None, 0.2), (16, 128, 129)),
    ((400, 160, 80.0, 400.0, 0, None, 0.15), (40, 200, 200)),
    ((400, 160, 80.0, 400.0, 1, "hann", 0.15), (40, 200, 200)),
    ((400, 500, 80.0, 400.0, 0, None, 0.1), (40, 200, 200)),          # hop > frame
    ((1024, 256, 60.0, 500.0, 0, None, 0.15), (32, 267, 757)),
]
CASE_IDS = [f"{c[0][0]}-{c[0][1]}-{c[0][2]:g}-{c[0][3]:g}-{'c' if c[0][4] else 'n'}-{c[0][5] or 'box'}" for c in CASES]

_fp = C.POINTER(C.c_float)
_zp = C.POINTER(C.c_size_t)


class Params(C.Structure):
    """vv_dsp_pitch_params"""
    _fields_ = [("sample_rate", C.c_float), ("fmin", C.c_float), ("fmax", C.c_float), ("threshold", C.c_float)]


def params(fmin, fmax, threshold, fs=FS):
    return Params(fs, fmin, fmax, threshold)


def signals():
    with np.load(os.path.join(GOLDEN, "pitch_signals.npz"), allow_pickle=False) as z:
        return z["sig"]


def hann(n):
    """vv_dsp_window_hann's table in float32 (symmetric)"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))).astype(np.float32)


def window_of(name, n):
    return None if name is None else hann(n)


# ------------------------------------------------------------- frames
def num_frames(n, frame, hop, center):
    if center:
        return (n + hop - 1) // hop
    return 0 if n < frame else 1 + (n - frame) // hop


def reflect(idx, n):
    """frame_src.hpp / framing.c:21-56"""
    if idx < 0:
        a = -idx - 1
        if a >= n:
            a %= 2 * n
            if a >= n:
                a = 2 * n - 1 - a
        return a
    if idx >= n:
        r = n - 1 - (idx - n)
        if r < 0:
            r = -r - 1
            if r >= n:
                r %= 2 * n
                if r >= n:
                    r = 2 * n - 1 - r
        return min(max(r, 0), n - 1)
    return idx


def frames_of(x, frame, hop, center, window):
    """[frames][frame] float32: vv_dsp_fetch_frames_device's rows of one channel"""
    x = np.asarray(x, np.float32)
    n = len(x)
    fr = num_frames(n, frame, hop, center)
    out = np.zeros((fr, frame), np.float32)
    for f in range(fr):
        start = f * hop - (frame // 2 if center else 0)
        if center:
            out[f] = x[[reflect(start + i, n) for i in range(frame)]]
        else:
            hi = min(n, start + frame)
            out[f, :hi - start] = x[start:hi]
    if window is not None:
        out = out * np.asarray(window, np.float32)       # one rounded float32 multiply
    return out


# ------------------------------------------------------------- the f64 model
def lag_range(fs, fmin, fmax, n):
    fs, lo, hi = (np.float64(np.float32(v)) for v in (fs, fmin, fmax))
    tau_min = max(2, int(np.floor(fs / hi)))
    tau_max = int(np.ceil(fs / lo))
    return tau_min, tau_max, n - tau_max


def cmnd_rows(rows, tau_max, sequential=False):
    """rows [F][n] float32 -> (d' [F][tau_max + 1] f64, c(tau_max) [F])"""
    x = np.asarray(rows, np.float32).astype(np.float64)
    F, n = x.shape
    W = n - tau_max
    d = np.empty((F, tau_max + 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for tau in range(tau_max + 1):
            df = x[:, :W] - x[:, tau:tau + W]
            sq = df * df
            d[:, tau] = np.cumsum(sq, axis=1)[:, -1] if sequential else np.sum(sq, axis=1)
        c = np.cumsum(d[:, 1:], axis=1)                   # ascending k
        q = np.ones((F, tau_max + 1))
        taus = np.arange(1, tau_max + 1, dtype=np.float64)
        with np.errstate(divide="ignore"):
            q[:, 1:] = np.where(c == 0.0, 1.0, d[:, 1:] * taus / c)
    return q, c[:, -1]


def _gap(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


def decide(q, total, fs, tau_min, tau_max, threshold):
    """one frame: (f0 float32, aperiodicity float32, lag, margin)"""
    fs = np.float64(np.float32(fs))
    thr = np.float64(np.float32(threshold))
    if not np.isfinite(total):
        return np.float32(0), np.float32(np.nan), 0, np.inf
    margin = np.inf
    tau = -1
    for t in range(tau_min, tau_max + 1):
        margin = min(margin, abs(q[t] - thr) / thr)
        if q[t] < thr:
            tau = t
            break
    if tau >= 0:
        while tau + 1 <= tau_max:
            margin = min(margin, _gap(q[tau + 1], q[tau]))
            if not q[tau + 1] < q[tau]:
                break
            tau += 1
        b = q[tau]
        off = 0.0
        if tau - 1 >= 1 and tau + 1 <= tau_max:
            a, c = q[tau - 1], q[tau + 1]
            margin = min(margin, _gap(a, b), _gap(c, b))
            den = (a - 2.0 * b) + c
            if a >= b and c >= b and den > 0.0:
                off = (a - c) / (2.0 * den)
        return np.float32(fs / (np.float64(tau) + off)), np.float32(b), tau, margin
    seg = q[tau_min:tau_max + 1]
    lag = tau_min + int(np.argmin(seg))                   # the first minimum
    two = np.sort(seg)[:2]
    if not (two[0] == 1.0 and two[1] == 1.0):
        margin = min(margin, _gap(two[0], two[1]))
    return np.float32(0), np.float32(q[lag]), lag, margin


def model_rows(rows, fmin, fmax, threshold, fs=FS, sequential=False):
    """rows [F][n] float32 -> dict: f0, aperiodicity float32 [F], lag int64 [F], cmnd float32
    [F][tau_max + 1], margin f64 [F]"""
    rows = np.asarray(rows, np.float32)
    tau_min, tau_max, W = lag_range(fs, fmin, fmax, rows.shape[1])
    assert W >= 1 and tau_min < tau_max
    q, total = cmnd_rows(rows, tau_max, sequential)
    res = [decide(q[f], total[f], fs, tau_min, tau_max, threshold) for f in range(len(rows))]
    return {"f0": np.array([r[0] for r in res], np.float32),
            "aperiodicity": np.array([r[1] for r in res], np.float32),
            "lag": np.array([r[2] for r in res], np.int64),
            "cmnd": q.astype(np.float32),
            "margin": np.array([r[3] for r in res], np.float64)}


def case_rows(case):
    """the frames of both fixture channels for a case: [2][frames][frame] float32"""
    frame, hop, _, _, center, win, _ = case
    w = window_of(win, frame)
    return np.stack([frames_of(ch, frame, hop, center, w) for ch in signals()])


_MODEL_CACHE = {}


def case_model(i):
    """the model over both channels of case i, computed once per process: name -> [2][frames]..."""
    if i not in _MODEL_CACHE:
        case = CASES[i][0]
        rows = case_rows(case)
        m = model_rows(rows.reshape(-1, rows.shape[2]), case[2], case[3], case[6])
        _MODEL_CACHE[i] = {k: v.reshape(rows.shape[:2] + v.shape[1:]) for k, v in m.items()}
    return _MODEL_CACHE[i]


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


def square_wave(n, period):
    return np.where(np.arange(n) % period < period // 2, 0.5, -0.5).astype(np.float32)


def tone(f, phase, n, rng, fs=FS):
    """three harmonics (1, 0.5, 0.25) of f plus 0.01 randn, float32"""
    t = np.arange(n) / fs
    x = sum(a * np.sin(2 * np.pi * k * f * t + k * phase) for k, a in ((1, 1.0), (2, 0.5), (3, 0.25)))
    return (x + 0.01 * rng.standard_normal(n)).astype(np.float32)


# ------------------------------------------------------------- the C API
class PitchApi:
    """vv_dsp_pitch_lag_range and vv_dsp_pitch_yin of one shared library, host pointers."""

    def __init__(self, path_or_lib):
        L = C.CDLL(path_or_lib) if isinstance(path_or_lib, str) else path_or_lib
        L.vv_dsp_pitch_lag_range.argtypes = [C.POINTER(Params), C.c_size_t, _zp, _zp, _zp]
        L.vv_dsp_pitch_yin.argtypes = [_fp, C.c_size_t, C.POINTER(Params), _fp, _fp]
        L.vv_dsp_amd_last_error.restype = C.c_char_p
        self.lib = L

    def lag_range(self, p, frame_len):
        """-> (status, tau_min, tau_max, W); the outputs keep their sentinel where untouched"""
        out = [C.c_size_t(SENTINEL_LAG) for _ in range(3)]
        st = self.lib.vv_dsp_pitch_lag_range(C.byref(p) if p is not None else None, frame_len,
                                             *(C.byref(o) for o in out))
        return (st,) + tuple(o.value for o in out)

    def yin(self, x, p, n=None, null_x=False):
        """-> (status, f0, aperiodicity)"""
        x = np.ascontiguousarray(x, np.float32)
        res = np.full(2, SENTINEL, np.float32)
        st = self.lib.vv_dsp_pitch_yin(None if null_x else x.ctypes.data_as(_fp), len(x) if n is None else n,
                                       C.byref(p) if p is not None else None, res[0:].ctypes.data_as(_fp),
                                       res[1:].ctypes.data_as(_fp))
        return st, res[0], res[1]
