"""The numpy model of include/vv_dsp/spectral/denoise.h, shared by test_denoise_host.py and
test_gpu_denoise.py.

The model is written twice, independently: `denoise_model` works on whole planes (the
running mean as W array adds in the header's order, the minimum over a sliding view of the
keys of tests/median_util.py); `denoise_naive` is the header read aloud, one scalar loop
per cell.  The host tests hold the two equal bit for bit on every case the GPU tests run.

K = n_fft // 2 + 1 and n_fft >= 2, so the narrowest row has two bins: the cases start at
K = 2, not 1."""
import os

import numpy as np

import median_util as mu
from median_util import OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_UNSUPPORTED, bits, canon   # noqa: F401

GATE, WIENER, SUBTRACT = 0, 1, 2
MAX_SMOOTH, MAX_REACH = 64, 511
NAMES = ("smooth", "noise", "gain")
KEY_NONE = np.uint32(0xFFFFFFFF)          # above the key of NaN


def _groups(rows, rows_per_group):
    rpg = rows if rows_per_group == 0 or rows_per_group > rows else rows_per_group
    return [(r0, min(r0 + rpg, rows)) for r0 in range(0, rows, max(rpg, 1))]


# ---- the vectorised form ----------------------------------------------------------------
def smooth_plane(p, W):
    """S of one group (G, K): W f64 adds per cell, oldest row first, rows before the first as the first"""
    G = p.shape[0]
    t = np.arange(G)
    acc = np.zeros(p.shape, np.float64)
    with np.errstate(all="ignore"):
        for j in range(W - 1, -1, -1):
            acc = acc + p[np.maximum(t - j, 0)].astype(np.float64)
        return canon((acc / np.float64(W)).astype(np.float32))


def floor_plane(S, back, ahead):
    """M of one group: the minimum in key order over rows [t - back, t + ahead] inside the group"""
    G, K = S.shape
    k = np.concatenate([np.full((back, K), KEY_NONE), mu.keys(S), np.full((ahead, K), KEY_NONE)])
    w = np.lib.stride_tricks.sliding_window_view(k, back + ahead + 1, axis=0)      # (G, K, B)
    return mu.unkey(w.min(axis=-1))


def gain_plane(p, M, bias, floor, mode):
    """(noise, gain) of powers p and floors M, float32 arrays"""
    with np.errstate(all="ignore"):
        r = np.float64(np.float32(bias)) * M.astype(np.float64)
        a = p.astype(np.float64)
        F = np.float64(np.float32(floor))
        one = np.float64(1.0)
        if mode == GATE:
            g = np.where(a > r, one, F)
        else:
            d = a - r
            q = d / a
            if mode == WIENER:
                g = np.where(q > F, q, F)
            else:
                assert mode == SUBTRACT
                f2 = F * F
                g = np.sqrt(np.where(q > f2, q, f2))
        g = np.where(g > one, one, g)
        return canon(r.astype(np.float32)), g.astype(np.float32)


def denoise_model(power, n_fft, W, back, ahead, bias, floor, mode, rows_per_group=0):
    """{smooth, noise, gain} of packed rows (rows, K)"""
    p = np.ascontiguousarray(power, dtype=np.float32)
    rows, K = p.shape
    assert K == n_fft // 2 + 1
    out = {name: np.empty_like(p) for name in NAMES}
    for r0, r1 in _groups(rows, rows_per_group):
        S = smooth_plane(p[r0:r1], W)
        out["smooth"][r0:r1] = S
        out["noise"][r0:r1], out["gain"][r0:r1] = gain_plane(p[r0:r1], floor_plane(S, back, ahead), bias, floor, mode)
    return out


# ---- the scalar form ----------------------------------------------------------------------
def _key1(v):
    b = int(np.float32(v).view(np.uint32))
    if v != v:
        b = 0x7FC00000
    return (b ^ 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def _f32(x):
    v = np.float32(x)
    return np.uint32(0x7FC00000).view(np.float32) if v != v else v


def denoise_naive(power, n_fft, W, back, ahead, bias, floor, mode, rows_per_group=0):
    p = np.ascontiguousarray(power, dtype=np.float32)
    rows, K = p.shape
    assert K == n_fft // 2 + 1
    out = {name: np.empty_like(p) for name in NAMES}
    f64 = np.float64
    F, bias64, one = f64(np.float32(floor)), f64(np.float32(bias)), f64(1.0)
    with np.errstate(all="ignore"):
        for r0, r1 in _groups(rows, rows_per_group):
            G = r1 - r0
            for k in range(K):
                col = [f64(v) for v in p[r0:r1, k]]
                S = []
                for t in range(G):
                    acc = f64(0.0)
                    for j in range(W - 1, -1, -1):
                        acc = acc + col[max(t - j, 0)]
                    S.append(_f32(acc / f64(W)))
                key = [_key1(s) for s in S]
                for t in range(G):
                    best = max(t - back, 0)
                    for u in range(max(t - back, 0), min(t + ahead, G - 1) + 1):
                        if key[u] < key[best]:
                            best = u
                    r = bias64 * f64(S[best])
                    a = col[t]
                    if mode == GATE:
                        g = one if a > r else F
                    else:
                        d = a - r
                        q = d / a
                        if mode == WIENER:
                            g = q if q > F else F
                        else:
                            f2 = F * F
                            q = q if q > f2 else f2
                            g = np.sqrt(q)
                    g = one if g > one else g
                    out["smooth"][r0 + t, k] = S[t]
                    out["noise"][r0 + t, k] = _f32(r)
                    out["gain"][r0 + t, k] = np.float32(g)
    return out


# ---- the rows and the cases ----------------------------------------------------------------
def power_rows(n_fft, rows, seed):
    """power rows (rows, K): a noise floor that differs per bin (chi-square with 2 degrees, as
    a periodogram), bursts on top of it, runs of equal values (ties in the minimum), some exact
    zeros and one denormal"""
    rng = np.random.default_rng(seed)
    K = n_fft // 2 + 1
    level = 10.0 ** rng.uniform(-4, 0, (1, K))
    p = level * rng.exponential(1.0, (rows, K))
    burst = rng.random((rows, K)) < 0.1
    p[burst] *= 100.0
    p = p.astype(np.float32)
    tie = rng.random((rows, K)) < 0.2
    p[tie] = np.float32(0.25)
    p[rng.random((rows, K)) < 0.03] = 0.0
    p[rows // 2, K // 2] = np.float32(1e-41)
    return p


def hostile_rows(n_fft, rows, seed):
    """power_rows with a quarter of the cells NaN (both signs, payloads), +-inf, -0, negative
    and denormal, and two columns that are NaN throughout"""
    rng = np.random.default_rng(seed)
    p = power_rows(n_fft, rows, seed)
    K = p.shape[1]
    sp = rng.random(p.shape) < 0.25
    pool = np.concatenate([mu.SPECIALS, np.array([-1.0, -3.5e-3, 1e-39, -1e-40, 3e38], np.float32)])
    p[sp] = pool[rng.integers(0, len(pool), int(sp.sum()))]
    p[:, K // 3] = np.float32(np.nan)
    p[:, K - 1] = mu.SPECIALS[-1]
    return p


def case(n_fft, rows, W=8, back=5, ahead=3, bias=4.0, floor=0.1, mode=WIENER, seg=0, rpg=0):
    return dict(n_fft=n_fft, rows=rows, W=W, back=back, ahead=ahead, bias=bias, floor=floor, mode=mode, seg=seg,
                rpg=rpg)


def case_id(c):
    return "n%d_r%d_w%d_b%d_a%d_m%d_s%d" % (c["n_fft"], c["rows"], c["W"], c["back"], c["ahead"], c["mode"], c["seg"])


def model_args(c):
    return (c["n_fft"], c["W"], c["back"], c["ahead"], c["bias"], c["floor"], c["mode"], c["rpg"])


# K = 2, 3, 63, 64, 65, 129, 513: one bin short of a tile, a whole tile, one bin into the next
N_FFTS = (2, 4, 124, 126, 128, 256, 1024)
_W, _BACK, _AHEAD = 8, 5, 3
SHAPE_CASES = (
    [case(n, 11, W=3, back=2, ahead=3, mode=m % 3) for m, n in enumerate(N_FFTS)]
    # G = 1, 2, W - 1, W, back, back + ahead + 1
    + [case(128, G, mode=G % 3) for G in (1, 2, _W - 1, _W, _BACK, _BACK + _AHEAD + 1)]
    # G = L - 1, L, L + 1, 2 L + 1 with the segment forced to L: a direct window (9 rows) and a blockwise one (23)
    + [case(128, G, back=b, ahead=a, seg=L, mode=(G + L) % 3)
       for L in (8, 32) for G in (L - 1, L, L + 1, 2 * L + 1) for b, a in ((_BACK, _AHEAD), (12, 10))]
    + [case(1024, 65, back=12, ahead=10, seg=32)]
)
REACHES = ((0, 0), (5, 0), (0, 5), (48, 48), (511, 511))
SMOOTHS = (1, 2, 8, 64)
# every reach with every smooth_len on a group of 40 rows (shorter than 48 + 48 + 1 and than 511), the modes,
# the two biases and the three floors going round
SETTING_CASES = [case(64, 40, W=W, back=b, ahead=a, mode=(i + j) % 3, bias=(0.5, 4.0)[(i + j) % 2],
                      floor=(0.0, 0.1, 1.0)[(i + 2 * j) % 3])
                 for i, (b, a) in enumerate(REACHES) for j, W in enumerate(SMOOTHS)]
# a group longer than the default window: several segments with the knob unset would need more rows than a test
# should take, so the seams inside a long window are set by the knob
SETTING_CASES += [case(64, 120, back=48, ahead=48, mode=m, seg=s, floor=0.1) for m, s in ((GATE, 0), (WIENER, 32),
                                                                                          (SUBTRACT, 50))]
ALL_CASES = SHAPE_CASES + SETTING_CASES


def case_rows(c, seed=None):
    return power_rows(c["n_fft"], c["rows"], c["rows"] * 1000 + c["W"] if seed is None else seed)


# ---- the behaviour fixture ------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_signal.npz")
N_FFT, HOP = 256, 64


def fixture_signal():
    """(clean, noise), float32, 2.25 s at 16 kHz (tests/golden/make_golden_denoise.py)"""
    with np.load(GOLDEN, allow_pickle=False) as z:
        return z["clean"], z["noise"]


def hann(n_fft=N_FFT):
    """the library's Hann window (symmetric), float64"""
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / (n_fft - 1))


def stft64(x):
    return mu.stft64(x, N_FFT, HOP)


def istft64(rows, n_fft=N_FFT, hop=HOP):
    """(y, covered): the overlap-add of the windowed inverse rows over the sum of the squared
    windows, as vv_dsp_stft_reconstruct_device and the normalise step; covered[i] holds where
    n_fft / hop frames overlap (norm is full)"""
    T = rows.shape[0]
    ln = (T - 1) * hop + n_fft
    w = hann(n_fft)
    fr = np.fft.irfft(rows, n_fft, axis=1) * w
    y, norm, cnt = np.zeros(ln), np.zeros(ln), np.zeros(ln, np.int64)
    for t in range(T):
        y[t * hop:t * hop + n_fft] += fr[t]
        norm[t * hop:t * hop + n_fft] += w * w
        cnt[t * hop:t * hop + n_fft] += 1
    return np.where(norm > 1e-8, y / np.where(norm > 1e-8, norm, 1.0), 0.0), cnt == n_fft // hop


def snr_db(clean, est):
    """of real signals or of complex rows"""
    clean, est = (np.asarray(v).astype(np.result_type(np.asarray(v).dtype, np.float64)) for v in (clean, est))
    return float(10.0 * np.log10((np.abs(clean) ** 2).sum() / (np.abs(est - clean) ** 2).sum()))
