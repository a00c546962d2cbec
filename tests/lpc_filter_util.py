"""Shared pieces of the LPC filter tests: the numpy model of
include/vv_dsp/envelope/lpc_filter.h in two forms (sample by sample; and a
vectorised residual with a synthesis done as the GPU's three chunk passes), the
case table both test sets run, and a ctypes binding of the host-row calls.

Every model operation is one IEEE f64 operation in the header's order, so the
residual and the exact synthesis can be held to it bit for bit.  The rows of
every case come from the fixture or from Levinson on frames of a signal (stable
by construction); random pole rows are not used.
"""
import ctypes as C
import functools
import os

import numpy as np

import lpc_util
from frames_util import hamming
from lsf_util import levinson_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
MAX_ORDER = 32
EXACT_MAX = 8192
QNAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]

FS = 16000
FIX_N = 2400
FIX_FRAME, FIX_HOP, FIX_ORDER = 400, 160, 16
FIX_ROWS = 15   # ceil(2400 / 160)
FORMANTS = ((700.0, 1200.0, 2600.0, 3500.0), (300.0, 2300.0, 3000.0, 3700.0))
BANDWIDTHS = (80.0, 100.0, 140.0, 180.0)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


# ------------------------------------------------------------- the fixture
def make_vowel(seed=20261):
    """2400 samples at 16 kHz: a pulse train gliding from 120 to 150 Hz plus 1 % noise through four
    two-pole resonators, whose frequencies switch at the middle; float32, peak 0.5"""
    rng = np.random.default_rng(seed)
    f0 = np.linspace(120.0, 150.0, FIX_N)
    phase = np.cumsum(f0 / FS)
    src = np.zeros(FIX_N)
    src[1:][np.floor(phase[1:]) > np.floor(phase[:-1])] = 1.0
    src[0] = 1.0
    src += 0.01 * rng.standard_normal(FIX_N)
    y = src
    for i, bw in enumerate(BANDWIDTHS):
        out = np.zeros(FIX_N)
        r = np.exp(-np.pi * bw / FS)
        y1 = y2 = 0.0
        for t in range(FIX_N):
            f = FORMANTS[0 if t < FIX_N // 2 else 1][i]
            v = y[t] + 2.0 * r * np.cos(2.0 * np.pi * f / FS) * y1 - r * r * y2
            out[t] = v
            y2, y1 = y1, v
        y = out
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


def reflect_frames(x, frame_len, hop):
    """the library's centred frames of x (center = 1): ceil(n / hop) of them, reflected at the ends"""
    n = len(x)
    frames = (n + hop - 1) // hop
    idx = np.arange(frame_len)[None, :] + hop * np.arange(frames)[:, None] - frame_len // 2
    idx = np.abs(idx)
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)
    return x[idx]


def levinson_rows(x, order, frame_len=FIX_FRAME, hop=FIX_HOP):
    """Hamming, centred Levinson rows of x in f64 -> (a [frames, order + 1] float32, err [frames] f64)"""
    fr = reflect_frames(np.asarray(x, np.float64), frame_len, hop) * hamming(frame_len).astype(np.float64)
    r = lpc_util.autocorr_f64(fr, order)
    a = np.stack([levinson_f64(r[i], order) for i in range(len(r))])
    err = np.array([r[i, 0] + np.dot(a[i, 1:], r[i, 1:]) for i in range(len(r))])
    return a.astype(np.float32), err


def make_fixture():
    sig = make_vowel()
    a, err = levinson_rows(sig, FIX_ORDER)
    gain = np.sqrt(np.maximum(err, 1e-12) / FIX_FRAME).astype(np.float32)
    return {"signal": sig, "a": a, "gain": gain}


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(GOLDEN, "lpc_filter_signal.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------- the model
def row_index(n, seg_len, offset, frames):
    t = np.arange(n, dtype=np.int64) + int(offset)
    return np.clip(t // int(seg_len), 0, frames - 1)


def to_float(acc):
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.asarray(acc, np.float64).astype(np.float32)
    out[np.isnan(acc)] = QNAN32
    return out


def _planes(x, a, gain, state):
    """x [nch, n]; a [nch or 1, frames, p + 1]; gain [nch or 1, frames] or None; state [nch, p] or None"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    a = np.asarray(a, np.float32)
    a = a[None] if a.ndim == 2 else a
    nch, p = x.shape[0], a.shape[2] - 1
    A = np.broadcast_to(a.astype(np.float64), (nch,) + a.shape[1:])
    G = None
    if gain is not None:
        g = np.asarray(gain, np.float32)
        G = np.broadcast_to((g[None] if g.ndim == 1 else g).astype(np.float64), (nch, a.shape[1]))
    S = np.zeros((nch, p)) if state is None else np.array(state, np.float64).reshape(nch, p)
    return x, A, G, S, nch, p


def _state_out(hist, p):
    """hist [nch, p + n], oldest first -> the last p values, newest first"""
    return hist[:, ::-1][:, :p].copy()


def residual_seq(x, a, seg_len, offset=0, gain=None, state=None):
    """the header, sample by sample -> (e float32 [nch, n], state out [nch, p])"""
    x, A, G, S, nch, p = _planes(x, a, gain, state)
    n = x.shape[1]
    f = row_index(n, seg_len, offset, A.shape[1])
    X = np.concatenate([S[:, ::-1], x.astype(np.float64)], axis=1)
    e = np.empty((nch, n), np.float64)
    with np.errstate(all="ignore"):
        for c in range(nch):
            for t in range(n):
                acc = X[c, p + t]
                for k in range(1, p + 1):
                    acc = acc + A[c, f[t], k] * X[c, p + t - k]
                if G is not None:
                    acc = acc / G[c, f[t]]
                e[c, t] = acc
    return to_float(e), _state_out(X, p)


def residual_vec(x, a, seg_len, offset=0, gain=None, state=None):
    """the same operations on whole rows at once"""
    x, A, G, S, nch, p = _planes(x, a, gain, state)
    n = x.shape[1]
    f = row_index(n, seg_len, offset, A.shape[1])
    X = np.concatenate([S[:, ::-1], x.astype(np.float64)], axis=1)
    ch = np.arange(nch)[:, None]
    with np.errstate(all="ignore"):
        acc = X[:, p:].copy()
        for k in range(1, p + 1):
            acc = acc + A[ch, f[None, :], k] * X[:, p - k:p - k + n]
        if G is not None:
            acc = acc / G[ch, f[None, :]]
    return to_float(acc), _state_out(X, p)


def synth_seq(e, a, seg_len, offset=0, gain=None, state=None):
    """the header's recursion, sequential in t (channels side by side)
    -> (y float32 [nch, n], Y f64 [nch, n], state out [nch, p])"""
    e, A, G, S, nch, p = _planes(e, a, gain, state)
    n = e.shape[1]
    f = row_index(n, seg_len, offset, A.shape[1])
    Y = np.concatenate([S[:, ::-1], np.zeros((nch, n))], axis=1)
    e64 = e.astype(np.float64)
    with np.errstate(all="ignore"):
        for t in range(n):
            acc = e64[:, t] if G is None else G[:, f[t]] * e64[:, t]
            at = A[:, f[t], :]
            for k in range(1, p + 1):
                acc = acc - at[:, k] * Y[:, p + t - k]
            Y[:, p + t] = acc
    return to_float(Y[:, p:]), Y[:, p:].copy(), _state_out(Y, p)


def synth_chunked(e, a, seg_len, offset, gain, state, L):
    """the GPU's three passes in numpy: per chunk the zero-state end values and the p x p
    transition from unit states; a scan over the chunks; every chunk walked again from its state"""
    e, A, G, S, nch, p = _planes(e, a, gain, state)
    n = e.shape[1]
    y = np.empty((nch, n), np.float32)
    Y = np.empty((nch, n))
    Sout = np.empty((nch, p))
    starts = list(range(0, n, L))
    for c in range(nch):
        ac = A[c].astype(np.float32)
        gc = None if G is None else G[c].astype(np.float32)
        s = S[c].copy()
        states = []
        for t0 in starts:
            m = min(L, n - t0)
            lanes = np.zeros((p + 1, m), np.float32)
            lanes[p] = e[c, t0:t0 + m]
            unit = np.concatenate([np.eye(p), np.zeros((1, p))])
            _, _, end = synth_seq(lanes, ac, seg_len, offset + t0, gc, unit)
            states.append(s)
            with np.errstate(all="ignore"):
                s = end[:p].T @ s + end[p]
        for t0, s in zip(starts, states):
            m = min(L, n - t0)
            y[c, t0:t0 + m], Y[c, t0:t0 + m], Sout[c] = synth_seq(e[c, t0:t0 + m], ac, seg_len, offset + t0, gc, s)
    return y, Y, Sout


def half_ulp32(v):
    """half a float32 ulp at |v| (f64 array): the rounding bound of (float)v"""
    _, ex = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.ldexp(1.0, np.maximum(ex - 25, -150))


# ------------------------------------------------------------- the case table
def channel_signal(c, n=FIX_N):
    """channel 0 is the fixture's vowel; the others are the vowel, delayed and scaled, plus noise"""
    sig = fixture()["signal"].astype(np.float64)
    if c == 0:
        return sig[:n].astype(np.float32)
    rng = np.random.default_rng(500 + c)
    x = (0.4 + 0.05 * (c % 9)) * np.roll(sig, 37 * c) + 0.02 * rng.standard_normal(FIX_N)
    return x[:n].astype(np.float32)


@functools.lru_cache(maxsize=None)
def channel_rows(c, order):
    """(a [15, order + 1] float32, gain [15] float32) of channel c"""
    if c == 0 and order == FIX_ORDER:
        return fixture()["a"], fixture()["gain"]
    a, err = levinson_rows(channel_signal(c), order)
    return a, np.sqrt(np.maximum(err, 1e-12) / FIX_FRAME).astype(np.float32)


def _case(name, order, seg_len, n, offset, frames, nch, gain, state, shared, pad):
    return dict(name=name, order=order, seg_len=seg_len, n=n, offset=offset, frames=frames, nch=nch, gain=gain,
                state=state, shared=shared, pad=pad)


def make_cases():
    """Every order with every seg_len; the other parameters cycle so that each value meets each
    order or seg_len at least once: n in {1, order - 1, 2 seg_len + 3, 2400}; offset 0, seg_len / 2,
    negative, past the last row; 1 / 3 / 15 rows (fewer and more than the signal needs); 1, 3, 65
    channels; gain, state, shared rows and padded strides on and off."""
    cases = []
    i = 0
    for order in (1, 2, 10, 16, 31, 32):
        for seg_len in (1, 7, 160):
            n = (1, max(order - 1, 1), 2 * seg_len + 3, FIX_N)[(i + i // 4) % 4]
            frames = (1, 3, FIX_ROWS)[(i + i // 3) % 3]
            offset = (0, seg_len // 2, -(seg_len + 3), frames * seg_len + 5)[(i // 2 + i // 8) % 4]
            nch = (1, 3, 65)[(i + 1) % 3] if n <= 400 or order < 31 else (1, 3)[i % 2]
            cases.append(_case(f"o{order}s{seg_len}", order, seg_len, n, offset, frames, nch, gain=i % 2 == 0,
                               state=i % 3 != 0, shared=i % 4 == 1, pad=i % 5 < 2))
            i += 1
    # the fixture as it is meant: its own rows at hop 160, the nearest centre governing
    cases.append(_case("vowel", FIX_ORDER, FIX_HOP, FIX_N, FIX_HOP // 2, FIX_ROWS, 1, True, False, False, False))
    cases.append(_case("vowel65", FIX_ORDER, FIX_HOP, FIX_N, FIX_HOP // 2, FIX_ROWS, 65, False, True, False, True))
    cases.append(_case("order32long", 32, 7, FIX_N, 3, FIX_ROWS, 3, True, True, True, False))
    cases.append(_case("order31long", 31, 160, FIX_N, -50, FIX_ROWS, 65, False, True, False, False))
    return cases


CASES = make_cases()
CASE_IDS = [c["name"] for c in CASES]
# the chunked synthesis: the fixture, chunks below the order and aligned to neither seg_len nor n
CHUNKS = (5, 64, 100)
CHUNK_CASES = [_case("chunk_vowel", FIX_ORDER, FIX_HOP, FIX_N, FIX_HOP // 2, FIX_ROWS, 1, True, True, False, False),
               _case("chunk_seg7", FIX_ORDER, 7, FIX_N, -20, FIX_ROWS, 2, False, False, False, True),
               _case("chunk_vowel3", FIX_ORDER, FIX_HOP, FIX_N, FIX_HOP // 2, FIX_ROWS, 3, True, True, False, True)]
CHUNK_IDS = [c["name"] for c in CHUNK_CASES]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = {c["name"]: c for c in CASES + CHUNK_CASES}[name]
    p, nch, n, frames = case["order"], case["nch"], case["n"], case["frames"]
    rng = np.random.default_rng(77 + 13 * p + n)
    x = np.stack([channel_signal(c, n) for c in range(nch)])
    na = 1 if case["shared"] else nch
    a = np.stack([channel_rows(c, p)[0][:frames] for c in range(na)])
    g = np.stack([channel_rows(c, p)[1][:frames] for c in range(na)]) if case["gain"] else None
    s = (0.01 * rng.standard_normal((nch, p))) if case["state"] else None
    exc = (0.05 * rng.standard_normal((nch, n))).astype(np.float32)
    exc[:, ::113] += 0.5   # pulses
    return dict(case=case, x=x, exc=exc, a=a, gain=g, state=s)


@functools.lru_cache(maxsize=None)
def expected(name):
    """inputs and the model's outputs of a case: res = (e, state), syn = (y, Y, state)"""
    d = dict(_inputs(name))
    c = d["case"]
    d["res"] = residual_vec(d["x"], d["a"], c["seg_len"], c["offset"], d["gain"], d["state"])
    d["syn"] = synth_seq(d["exc"], d["a"], c["seg_len"], c["offset"], d["gain"], d["state"])
    return d


@functools.lru_cache(maxsize=None)
def chunk_expected(name, L):
    """the chunked model form of a chunk case and its relative distance D from the sequential
    form: max |Y_chunked - Y| and max |state_chunked - state| over max |Y|, in f64"""
    d = expected(name)
    c = d["case"]
    y, Y, S = synth_chunked(d["exc"], d["a"], c["seg_len"], c["offset"], d["gain"], d["state"], L)
    ys, Ys, Ss = d["syn"]
    peak = np.abs(Ys).max()
    D = max(np.abs(Y - Ys).max(), np.abs(S - Ss).max()) / peak
    return dict(y=y, Y=Y, state=S, D=float(D), differ=int(np.sum(bits(y) != bits(ys))))


# ------------------------------------------------------------- the C API
_fp = C.POINTER(C.c_float)
_dp = C.POINTER(C.c_double)
SENT = np.float32(-123.0)


class LpcFilterApi:
    """vv_dsp_lpc_residual / vv_dsp_lpc_synth of the product library, host pointers."""

    def __init__(self, path):
        L = C.CDLL(path)
        for f in ("residual", "synth"):
            getattr(L, f"vv_dsp_lpc_{f}").argtypes = [_fp, C.c_size_t, _fp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                      C.c_longlong, _fp, _dp, _fp]
            getattr(L, f"vv_dsp_lpc_{f}_device").argtypes = \
                [C.c_void_p] + [C.c_size_t] * 3 + [C.c_void_p] + [C.c_size_t] * 4 + [C.c_void_p] + \
                [C.c_size_t] * 2 + [C.c_longlong, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.vv_dsp_lpc_residual_frames_device.argtypes = \
            [C.c_void_p] + [C.c_size_t] * 5 + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.vv_dsp_amd_last_error.restype = C.c_char_p
        self.lib = L

    def run(self, which, x, a, seg_len, offset=0, gain=None, state=None, order=None, frames=None, n=None):
        """-> (status, out [n] (SENT where untouched), state out or None)"""
        x = np.ascontiguousarray(x, np.float32)
        a = np.ascontiguousarray(a, np.float32)
        a2 = a.reshape(-1, a.shape[-1])
        order = a2.shape[1] - 1 if order is None else order
        frames = a2.shape[0] if frames is None else frames
        n = len(x) if n is None else n
        out = np.full(max(len(x), 1), SENT, np.float32)
        g = None if gain is None else np.ascontiguousarray(gain, np.float32)
        s = None if state is None else np.array(state, np.float64)
        st = getattr(self.lib, f"vv_dsp_lpc_{which}")(
            x.ctypes.data_as(_fp), n, a2.ctypes.data_as(_fp), order, frames, seg_len, offset,
            None if g is None else g.ctypes.data_as(_fp), None if s is None else s.ctypes.data_as(_dp),
            out.ctypes.data_as(_fp))
        return st, out[:len(x)], s


def assert_bits(got, want, what):
    gb, wb = bits(np.asarray(got)), bits(np.asarray(want).astype(np.asarray(got).dtype))
    assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
    assert np.array_equal(gb, wb), (what, int(np.sum(gb != wb)), np.argwhere(gb != wb)[:6].tolist())
