"""Shared pieces of the pitch-tracking tests: the f64 model of
include/vv_dsp/features/pitch_track.h in two forms (vectorised over the states,
and a deliberately naive scalar one that clips the band instead of padding it
and keeps plain Python floats), the synthetic curve cases, the behaviour
fixture and a ctypes binding of the host entry points.

The definition has no sum whose order is free: every value is an f64 add, one
multiply or one divide, and every decision a strict comparison in a stated
order.  The model is therefore the truth bit for bit, ties included; the tests
compare with array_equal (NaN == NaN for the aperiodicity plane).
"""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = range(7)
MAX_STEP, MAX_STATES, BLOCK = 126, 4096, 64     # the header's limits; L of the backtrace for S + 1 <= 960
DEFAULT_COSTS = (4.0, 0.5, 0.3, 0.35, 8)        # lambda, jump, switch, unvoiced, max_step


class TrackParams(C.Structure):
    """vv_dsp_pitch_track_params"""
    _fields_ = [("sample_rate", C.c_float), ("tau_min", C.c_uint32), ("tau_max", C.c_uint32), ("lambda_", C.c_float),
                ("jump_cost", C.c_float), ("switch_cost", C.c_float), ("unvoiced_cost", C.c_float),
                ("max_step", C.c_uint32)]


class TrackOut(C.Structure):
    """vv_dsp_pitch_track_out"""
    _fields_ = [("lag", C.c_void_p), ("f0", C.c_void_p), ("aperiodicity", C.c_void_p), ("cost", C.c_void_p)]


def tparams(tau_min, tau_max, lam=4.0, jump=0.5, switch=0.3, unvoiced=0.35, max_step=8, fs=16000.0):
    return TrackParams(fs, tau_min, tau_max, lam, jump, switch, unvoiced, max_step)


def bad_range_fields():
    """name -> the fields (in order) of parameters that are OUT_OF_RANGE"""
    inf, nan = float("inf"), float("nan")
    good = [16000.0, 20, 84, 4.0, 0.5, 0.3, 0.35, 8]
    res = {"tau_min_zero": [16000.0, 0, 50] + good[3:], "tau_min_equals_tau_max": [16000.0, 50, 50] + good[3:],
           "tau_min_above_tau_max": [16000.0, 51, 50] + good[3:]}
    for i, field in ((3, "lambda"), (4, "jump"), (5, "switch"), (6, "unvoiced")):
        for name, v in (("negative", -0.5), ("inf", inf), ("nan", nan)):
            res[f"{field}_{name}"] = good[:i] + [v] + good[i + 1:]
    for name, v in (("zero", 0.0), ("negative", -1.0), ("inf", inf), ("nan", nan)):
        res[f"sample_rate_{name}"] = [v] + good[1:]
    return {k: tuple(v) for k, v in res.items()}


def _costs(p):
    """the parameters as the definition uses them: float32 fields converted to double once"""
    f = lambda v: float(np.float64(np.float32(v)))  # noqa: E731
    return (f(p.sample_rate), int(p.tau_min), int(p.tau_max), f(p.lambda_), f(p.jump_cost), f(p.switch_cost),
            f(p.unvoiced_cost), int(p.max_step))


# ------------------------------------------------------------- outputs shared by both forms
def _outputs(q, path, fs, tau_min, tau_max):
    F = len(path)
    lag = np.array(path, np.uint32)
    f0 = np.zeros(F, np.float32)
    ap = np.empty(F, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(F):
            tau = int(path[t])
            if tau:
                b = np.float64(q[t, tau])
                off = np.float64(0.0)
                if tau - 1 >= 1 and tau + 1 <= tau_max:
                    a, c = np.float64(q[t, tau - 1]), np.float64(q[t, tau + 1])
                    den = (a - 2.0 * b) + c
                    if a >= b and c >= b and den > 0.0:
                        off = (a - c) / (2.0 * den)
                f0[t] = np.float32(np.float64(fs) / (np.float64(tau) + off))
                ap[t] = q[t, tau]
            else:
                seg = q[t, tau_min:tau_max + 1]
                vals = seg[~np.isnan(seg)]
                ap[t] = vals[np.argmin(vals)] if len(vals) else np.float32(np.nan)   # the first minimum
    return lag, f0, ap


# ------------------------------------------------------------- the model, vectorised over states
def model(q, p):
    """q [F][>= tau_max + 1] float32, p TrackParams -> dict lag uint32 [F], f0, aperiodicity
    float32 [F], cost float64"""
    q = np.asarray(q, np.float32)
    fs, tau_min, tau_max, lam, jump, sw, uc, B = _costs(p)
    F, S = q.shape[0], tau_max - tau_min + 1
    taus = np.arange(tau_min, tau_max + 1, dtype=np.float64)
    r = np.float64(lam) / taus
    steps = range(-min(B, S - 1), min(B, S - 1) + 1)
    pen = {k: np.float64(abs(k)) * r for k in steps}                 # fl(|k| r(tau)), rounded before the add
    with np.errstate(invalid="ignore", over="ignore"):
        obs = q[:, tau_min:tau_max + 1].astype(np.float64)
        obs = np.where(np.isnan(obs), np.inf, obs)
        D = obs[0].copy()
        DU = np.float64(uc)
        pred = np.zeros((F, S + 1), np.int64)
        sstar = np.zeros(F, np.int64)
        for t in range(1, F):
            s = int(np.argmin(D))                                    # the lowest lag of the minimum
            sstar[t] = s
            best = np.full(S, DU + sw)
            code = np.zeros(S, np.int64)
            cj = D[s] + jump
            if cj < best[0]:                                         # the same comparison for every state
                best[:] = cj
                code[:] = 1
            padded = np.full(S + 2 * B, np.inf)
            padded[B:B + S] = D                                      # +inf beyond the range: never strictly smaller
            for k in steps:
                c = padded[B + k:B + k + S] + pen[k]
                m = c < best
                best = np.where(m, c, best)
                code = np.where(m, 2 + k + B, code)
            pred[t, :S] = code
            bu, cu = DU, 0
            cs = D[s] + sw
            if cs < bu:
                bu, cu = cs, 1
            pred[t, S] = cu
            D = best + obs[t]
            DU = bu + uc
        s = int(np.argmin(D))
        state, cost = (s, D[s]) if D[s] < DU else (S, DU)
    path = [0] * F
    for t in range(F - 1, -1, -1):
        path[t] = 0 if state == S else tau_min + state
        if t > 0:
            c = int(pred[t, state])
            state = S if c == 0 else int(sstar[t]) if c == 1 else state + (c - 2) - B
    lag, f0, ap = _outputs(q, path, fs, tau_min, tau_max)
    return {"lag": lag, "f0": f0, "aperiodicity": ap, "cost": np.float64(cost)}


# ------------------------------------------------------------- the naive scalar form
def model_naive(q, p):
    """the header read line by line: Python floats (IEEE doubles, one rounding per
    operation), the band clipped to the lag range, predecessors kept as states"""
    q = np.asarray(q, np.float32)
    fs, tau_min, tau_max, lam, jump, sw, uc, B = _costs(p)
    F = q.shape[0]
    lags = list(range(tau_min, tau_max + 1))
    inf = float("inf")

    def O(t, tau):
        v = float(q[t, tau])
        return inf if v != v else v

    D = {tau: O(0, tau) for tau in lags}
    DU = uc
    back = []                                                         # per step: {state: predecessor}, "U" = unvoiced
    for t in range(1, F):
        sbest = lags[0]
        for tau in lags:
            if D[tau] < D[sbest]:
                sbest = tau
        nd, bk = {}, {}
        for tau in lags:
            best, who = DU + sw, "U"
            c = D[sbest] + jump
            if c < best:
                best, who = c, sbest
            rr = lam / float(tau)
            for tp in range(max(tau_min, tau - B), min(tau_max, tau + B) + 1):
                pnl = float(abs(tau - tp)) * rr
                c = D[tp] + pnl
                if c < best:
                    best, who = c, tp
            nd[tau] = best + O(t, tau)
            bk[tau] = who
        best, who = DU, "U"
        c = D[sbest] + sw
        if c < best:
            best, who = c, sbest
        bk["U"] = who
        D, DU = nd, best + uc
        back.append(bk)
    state, cost = "U", DU
    sbest = lags[0]
    for tau in lags:
        if D[tau] < D[sbest]:
            sbest = tau
    if D[sbest] < DU:
        state, cost = sbest, D[sbest]
    path = [0] * F
    for t in range(F - 1, -1, -1):
        path[t] = 0 if state == "U" else state
        if t > 0:
            state = back[t - 1][state]
    lag, f0, ap = _outputs(q, path, fs, tau_min, tau_max)
    return {"lag": lag, "f0": f0, "aperiodicity": ap, "cost": np.float64(cost)}


def same(a, b):
    """bit-for-bit agreement of two results (NaN aperiodicity equal to NaN)"""
    return (np.array_equal(a["lag"], b["lag"]) and
            np.array_equal(np.asarray(a["f0"], np.float32).view(np.uint32), np.asarray(b["f0"], np.float32).view(np.uint32))
            and np.array_equal(a["aperiodicity"], b["aperiodicity"], equal_nan=True) and
            np.float64(a["cost"]).view(np.uint64) == np.float64(b["cost"]).view(np.uint64))


# ------------------------------------------------------------- synthetic curves
def curves(F, tau_min, tau_max, seed, kind="contour"):
    """[F][tau_max + 1] float32, seeded, independent of the YIN kernel.
    contour: noise in [0.3, 1.3) with a dip near a wandering lag, a second dip at twice
      that lag (or half), and stretches with no dip (unvoiced);
    ties: multiples of 1/8 in [0, 1] (with lambda and tau powers of two the penalties are exact);
    nan: contour with rows of all NaN, rows with some NaN and +inf values;
    zero: all zero."""
    rng = np.random.default_rng(seed)
    W = tau_max + 1
    if kind == "zero":
        return np.zeros((F, W), np.float32)
    if kind == "ties":
        return (rng.integers(0, 9, (F, W)) / 8.0).astype(np.float32)
    q = (0.3 + rng.random((F, W))).astype(np.float32)
    S = tau_max - tau_min + 1
    centre = tau_min + S * (0.3 + 0.1 * np.sin(np.arange(F) / 7.0 + seed))
    for t in range(F):
        if (t // 9) % 4 == 3:
            continue                                                 # no dip: unvoiced stretch
        c = int(centre[t])
        for lag, depth in ((c, 0.25 if (t // 5) % 3 else 0.02), (2 * c, 0.03), (c // 2, 0.2)):
            for d in (-1, 0, 1):
                if tau_min <= lag + d <= tau_max:
                    q[t, lag + d] = np.float32(depth + 0.1 * abs(d) + 0.02 * rng.random())
    if kind == "nan":
        for t in range(F):
            if t % 7 == 3:
                q[t, :] = np.nan
            elif t % 7 == 5:
                q[t, rng.integers(0, W, max(1, W // 3))] = np.nan
            elif t % 7 == 6:
                q[t, rng.integers(0, W, max(1, W // 4))] = np.inf
    return q


# (name, S, F, max_step, kind, costs or None): every case the GPU test runs against the model
# and the CPU test runs through both forms of the model.  tau_min = 20 unless the kind says
# otherwise.  S: a lane, a wave and the one-wave / workgroup switch (256) on either side;
# F: 1, 2, 3 and the backtrace block L = 64 at L - 1, L, L + 1, 2 L + 1; max_step 0, 1, 8 and >= S
# (the band clipped at both ends).  The naive form costs F S min(2 B + 1, S) steps of Python: the
# long and wide cases keep max_step small.
def _cases():
    cs = []
    for S in (63, 64, 65, 129, 257, 300):
        cs.append((f"S{S}", S, 70, 8, "contour", None))
    for F in (1, 2, 3, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
        cs.append((f"F{F}", 65, F, 8, "contour", None))
    cs.append(("F650", 63, 650, 1, "contour", None))
    for B in (0, 1, 8, 70, MAX_STEP):
        cs.append((f"B{B}", 65, 40, B, "contour", None))
    cs.append(("B126-S300", 300, 12, MAX_STEP, "contour", None))
    for B in (1, 8, 64):
        cs.append((f"ties-B{B}", 65, 50, B, "ties", (8.0, 0.5, 0.25, 0.375)))
    cs.append(("ties-S300", 300, 20, 8, "ties", (8.0, 0.5, 0.25, 0.375)))
    cs.append(("ties-lambda0", 65, 50, 8, "ties", (0.0, 0.5, 0.25, 0.375)))       # every band candidate a pure D
    cs.append(("nan", 129, 70, 8, "nan", None))
    cs.append(("nan-B3-S300", 300, 30, 3, "nan", None))
    cs.append(("zero", 65, 20, 8, "zero", None))
    cs.append(("jump0", 65, 70, 8, "contour", (4.0, 0.0, 0.3, 0.35)))
    cs.append(("switch0", 65, 70, 8, "contour", (4.0, 0.5, 0.0, 0.35)))
    cs.append(("both0-B2", 129, 70, 2, "contour", (4.0, 0.0, 0.0, 0.35)))
    cs.append(("lambda0", 65, 40, 8, "contour", (0.0, 0.5, 0.3, 0.35)))
    return cs


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]


def case_inputs(i):
    """(q [F][tau_max + 1] float32, TrackParams) of case i; ties: tau_min 16, so with lambda 8
    and costs in eighths many candidates are equal in every bit"""
    name, S, F, B, kind, costs = CASES[i]
    tau_min = 16 if kind == "ties" else 20
    tau_max = tau_min + S - 1
    lam, jump, sw, uc = costs or DEFAULT_COSTS[:4]
    q = curves(F, tau_min, tau_max, 1000 + i, kind)
    return q, tparams(tau_min, tau_max, lam, jump, sw, uc, B)


_MODEL_CACHE = {}


def case_model(i):
    """the model of case i, computed once per process"""
    if i not in _MODEL_CACHE:
        _MODEL_CACHE[i] = model(*case_inputs(i))
    return _MODEL_CACHE[i]


# ------------------------------------------------------------- the behaviour fixture
BEHAVIOUR = dict(frame=400, hop=160, fmin=80.0, fmax=500.0, threshold=0.15, fs=16000.0)


def behaviour_signal():
    """tests/golden/track_signal.npz (make_golden_track.py): sig float32, f_true [n] Hz,
    gap (start, stop) samples of the noise gap"""
    with np.load(os.path.join(GOLDEN, "track_signal.npz"), allow_pickle=False) as z:
        return z["sig"], z["f_true"], tuple(int(v) for v in z["gap"])


def frame_truth(f_true, gap, frame, hop, fs):
    """per frame (no centring): the true period in samples at the frame's middle, and
    whether the frame lies clear of the gap (no sample within the gap or a frame of it)"""
    n = len(f_true)
    F = 1 + (n - frame) // hop
    mid = np.arange(F) * hop + frame // 2
    period = fs / f_true[mid]
    start = np.arange(F) * hop
    clear = (start + frame <= gap[0] - frame) | (start >= gap[1] + frame)
    inside = (start >= gap[0]) & (start + frame <= gap[1])
    return period, clear, inside


# ------------------------------------------------------------- the C API (host pointers)
class TrackApi:
    def __init__(self, path_or_lib):
        L = C.CDLL(path_or_lib) if isinstance(path_or_lib, str) else path_or_lib
        L.vv_dsp_pitch_track.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(TrackParams),
                                         C.POINTER(TrackOut)]
        L.vv_dsp_pitch_track_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                C.POINTER(TrackParams), C.POINTER(TrackOut), C.c_size_t, C.c_void_p]
        L.vv_dsp_amd_last_error.restype = C.c_char_p
        self.lib = L

    def track(self, q, p, what=("lag", "f0", "aperiodicity", "cost"), frames=None, row_stride=None):
        """-> (status, dict of the outputs in `what`, sentinel-filled where not written)"""
        q = np.ascontiguousarray(q, np.float32)
        F = q.shape[0] if frames is None else frames
        res = {"lag": np.full(max(F, 1), 987654321, np.uint32), "f0": np.full(max(F, 1), -123.0, np.float32),
               "aperiodicity": np.full(max(F, 1), -123.0, np.float32), "cost": np.full(1, -123.0, np.float64)}
        out = TrackOut(*(res[k].ctypes.data if k in what else None for k in ("lag", "f0", "aperiodicity", "cost")))
        st = self.lib.vv_dsp_pitch_track(q.ctypes.data, F, q.shape[1] if row_stride is None else row_stride,
                                         C.byref(p) if p is not None else None, C.byref(out))
        return st, res
