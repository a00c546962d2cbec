"""Float64 reference and derived error bounds for the mel / MFCC kernels
(k_mel_grp in mel_kernels.hip, mel_rows / mel_tail in stft_rows.hpp).

The reference is plain NumPy in float64 on the same float32 inputs (the
filterbank, the power rows and eps are upcast, never recomputed):

    log_mel64 = log(power64 @ fb64.T + eps)
    mfcc64[i] = L[i] * sum_m lm[m] cos(pi (m + 1/2) i / M)
    L[0] = 1, L[i] = 1 + (lifter / 2) sin(pi i / lifter)   (lifter > 0)

The bounds are derived from the kernels' arithmetic, with u = 2^-24:

log-mel.  Filter m has L_m bins in its non-zero range, cut into K_m chunks;
    each chunk is one FMA chain and the K_m partials are added in order, so
    for non-negative weights and power the f32 sum has relative error at most
    (L_m + K_m) u.  The add of eps is one more rounding, and logf is within
    2 ulp of its result (OCML's documented accuracy), i.e. 4 u |ref|:
        |got - ref| <= (L_m + K_m + 2) u + 4 u |ref|
    K_m <= ceil(L_m / 4), because the schedule's smallest chunk length is 4.
    With weights of both signs the sum's error is (L_m + K_m) u sum|w p|, so
    the first term is scaled by amp = sum|w p| / (e + eps); the tests keep
    amp <= 10 so that the log does not amplify cancellation.

MFCC from given log-mel rows.  Four FMA chains of M / 4, three adds, one
    rounding of the cosine table (rounded once from double), the lifter
    product and a few ulp for sinf in the lifter factor:
        |got_i - ref_i| <= (M / 4 + 16) u |L_i| sum_m |lm_m cos(...)|
    plus one term for the lifter factor itself.  The kernels use the
    reference's float32 factor 1 + (lifter / 2) sinf(pi_f i / lifter)
    (mel.c:300-302), whose angle a_i = pi i / lifter carries the rounding of
    pi, one product and one quotient (3 u a_i), sinf its 2 ulp (4 u) and the
    product with lifter / 2 one rounding, so the factor differs from the
    float64 formula above by up to dL_i = (lifter / 2) (3 a_i + 5) u -- at
    lifter 22, i = 44 (a_i = 2 pi, L_i = 1) it measures 120 u, at i = 22 60 u,
    far past "a few ulp" of L_i.  That is a gap in the plain bound, not a
    kernel defect: the factor is the reference's, bit for bit.  The bound is
        (M / 4 + 16) u |L_i| sum_m |lm_m cos(...)| + dL_i |sum_m lm_m cos(...)|
    and `plain=True` gives the first term alone (reported by the tests).
"""
import numpy as np

U = 2.0 ** -24

# name: (nfft, mels, sr, fmin, fmax, C, lifter, property the case is there for)
PLANS = {
    "P1": (1024, 1, 48000.0, 0.0, 24000.0, 1, 0.0, "one filter, about 64 chunks"),
    "P2": (1024, 2, 48000.0, 20.0, 24000.0, 2, 22.0, ""),
    "P3": (1024, 23, 16000.0, 0.0, 8000.0, 23, 22.0, "odd M, C = M"),
    "P4": (1024, 41, 48000.0, 20.0, 20000.0, 13, 1.0, "odd M"),
    "P5": (1024, 60, 48000.0, 0.0, 4000.0, 60, 22.0, "empty filter, fused-MFCC boundary, C = M"),
    "P6": (1024, 61, 48000.0, 20.0, 24000.0, 33, 0.5, "2C > 64"),
    "P7": (1024, 120, 48000.0, 0.0, 24000.0, 13, 22.0, "empty filter, two filters per lane"),
    "P8": (1024, 128, 48000.0, 0.0, 24000.0, 128, 0.0, "nc > 256"),
    "P9": (1024, 200, 48000.0, 0.0, 24000.0, 13, 22.0, "M > 128, several empty filters"),
    "P10": (1024, 40, 48000.0, 300.0, 3400.0, 13, 22.0, "filters of 1-6 bins"),
    "P11": (1024, 3, 48000.0, 10000.0, 24000.0, 3, 22.0, "first non-zero bin far from 0"),
    "P12": (16, 7, 8000.0, 0.0, 4000.0, 7, 22.0, "nbins 9, empty filter"),
    "P13": (4, 1, 8000.0, 0.0, 4000.0, 1, 0.0, "nbins 3"),
    "P14": (2048, 80, 44100.0, 0.0, 22050.0, 20, 22.0, "fr = 2"),
    "P15": (4096, 40, 48000.0, 20.0, 20000.0, 13, 22.0, "fr = 1"),
    "P16": (8192, 40, 48000.0, 20.0, 20000.0, 13, 22.0, "fr = 1, longest rows"),
}
NFFT1024 = ["P%d" % i for i in range(1, 12)]


def fb_ranges(fb):
    """-> (lo, length) of each filter's non-zero range (first .. last non-zero
    bin, zeros inside count); an all-zero filter has length 0."""
    fb = np.asarray(fb)
    lo = np.zeros(fb.shape[0], np.int64)
    ln = np.zeros(fb.shape[0], np.int64)
    for m in range(fb.shape[0]):
        nz = np.flatnonzero(fb[m])
        if nz.size:
            lo[m], ln[m] = nz[0], nz[-1] + 1 - nz[0]
    return lo, ln


def chunk_count(fb):
    """The chunk schedule of mel_kernels.hip restated (mel_chunk_schedule): the
    chunk length lc (a multiple of 4 minimising rounds of 64 lanes x (lc + 8))
    and the number of chunks nc.  Only for asserting what a plan exercises
    (nc > 256 takes the two launches); no bound uses it."""
    _, ln = fb_ranges(fb)
    maxlen = max(1, int(ln.max()))
    best = None
    lc = 4
    while lc < 2 * maxlen + 4:
        nc = int(np.sum((ln + lc - 1) // lc))
        cost = (nc + 63) // 64 * (lc + 8)
        if best is None or cost < best[0]:
            best = (cost, lc, nc)
        if lc >= maxlen:
            break
        lc += 4
    return best[1], best[2]


def log_mel64(power, fb, eps):
    p, w = np.asarray(power, np.float64), np.asarray(fb, np.float64)
    with np.errstate(divide="ignore"):
        return np.log(p @ w.T + float(np.float32(eps)))


def log_mel_bound(power, fb, eps, ref=None, unit=False):
    """Bound of |log-mel - log_mel64| per (row, filter).  unit: L_m = K_m = 1
    (a power row with one non-zero bin).  Banks with negative weights scale
    the sum's term by amp = sum|w p| / (e + eps); returns (bound, amp)."""
    p, w = np.asarray(power, np.float64), np.asarray(fb, np.float64)
    ref = log_mel64(power, fb, eps) if ref is None else ref
    _, ln = fb_ranges(fb)
    lk = np.where(ln > 0, 2, 0) if unit else ln + (ln + 3) // 4
    amp = np.ones_like(ref)
    if np.any(w < 0):
        s = np.abs(p) @ np.abs(w).T
        arg = p @ w.T + float(np.float32(eps))
        amp = np.maximum(1.0, s / arg)
    with np.errstate(invalid="ignore"):
        fin = np.where(np.isfinite(ref), np.abs(ref), 0.0)
    return (lk[None, :] * amp + 2) * U + 4 * U * fin, amp


def lifter64(n_coeffs, lifter):
    lf = np.ones(n_coeffs)
    lifter = float(np.float32(lifter))
    if lifter > 0:
        i = np.arange(1, n_coeffs)
        lf[1:] = 1.0 + (lifter / 2.0) * np.sin(np.pi * i / lifter)
    return lf


def dct_table64(n_mels, n_coeffs):
    m, i = np.arange(n_mels), np.arange(n_coeffs)
    return np.cos(np.pi * (m[None, :] + 0.5) * i[:, None] / n_mels)   # [C][M]


def mfcc64(lm, n_coeffs, lifter):
    lm = np.asarray(lm, np.float64)
    return (lm @ dct_table64(lm.shape[1], n_coeffs).T) * lifter64(n_coeffs, lifter)[None, :]


def lifter_gap(n_coeffs, lifter):
    """dL_i: the float32 lifter factor's distance from the float64 formula (module docstring)"""
    lifter = float(np.float32(lifter))
    if lifter <= 0:
        return np.zeros(n_coeffs)
    a = np.pi * np.arange(n_coeffs) / lifter
    d = (lifter / 2.0) * (3.0 * a + 5.0) * U
    d[0] = 0.0
    return d


def mfcc_bound(lm, n_coeffs, lifter, plain=False):
    """Bound of |MFCC - mfcc64| per (row, coefficient) for the log-mel rows lm."""
    lm = np.asarray(lm, np.float64)
    M = lm.shape[1]
    tab = dct_table64(M, n_coeffs)
    mag = np.abs(lm) @ np.abs(tab).T
    b = (M / 4.0 + 16.0) * U * np.abs(lifter64(n_coeffs, lifter))[None, :] * mag
    return b if plain else b + lifter_gap(n_coeffs, lifter)[None, :] * np.abs(lm @ tab.T)


def mfcc_bound_from_power(lm_ref, lm_bound, n_coeffs, lifter):
    """End to end: the DCT bound on log-mel rows that are themselves within
    lm_bound of lm_ref, plus what that difference is worth after the f64 DCT."""
    M = lm_ref.shape[1]
    spread = lm_bound @ np.abs(dct_table64(M, n_coeffs)).T * np.abs(lifter64(n_coeffs, lifter))[None, :]
    gap = lifter_gap(n_coeffs, lifter)[None, :] * ((np.abs(lm_ref) + lm_bound) @ np.abs(dct_table64(M, n_coeffs)).T)
    return mfcc_bound(np.abs(lm_ref) + lm_bound, n_coeffs, lifter, plain=True) + gap + spread


def oracle_mfcc_bound(lm, n_coeffs, lifter):
    """Bound of |oracle MFCC - mfcc64|: mfcc_bound plus the oracle's own error.
    The oracle restates the reference's dct.c: one running f32 sum of M terms
    where the kernel has four chains of M / 4 (3 M / 4 u of sum|lm cos| more),
    and angles pi (m + 1/2) i / M that are f32 products (pi rounded, two
    products, one quotient: 4 u of an angle below pi i, so each cosine is off
    by up to 4 pi i u) where the kernel's table is rounded once from double."""
    lma = np.abs(np.asarray(lm, np.float64))
    M = lma.shape[1]
    i = np.arange(n_coeffs)
    mag = lma @ np.abs(dct_table64(M, n_coeffs)).T
    ang = 4.0 * np.pi * i[None, :] * lma.sum(axis=1)[:, None]
    own = (0.75 * M * mag + ang) * U * np.abs(lifter64(n_coeffs, lifter))[None, :]
    return mfcc_bound(lm, n_coeffs, lifter) + own


def ratio(got, ref, bound):
    """max(error / bound) over the finite entries of ref"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    err, b = np.abs(got[ok] - ref[ok]), np.asarray(bound, np.float64)[ok]
    # a zero bound (all-zero log-mel rows) asks for equality
    return float(np.max(np.where(err == 0, 0.0, err / np.where(b > 0, b, np.finfo(np.float64).tiny))))


def plan_power(nbins, rows, seed):
    """rand^2 * 10 with one row of exact zeros (the last)"""
    rng = np.random.default_rng(seed)
    p = (rng.random((rows, nbins)) ** 2 * 10).astype(np.float32)
    p[-1] = 0.0
    return p


def probe_power(nbins):
    """Row k < nbins is 2^10 e_k; row nbins is all zeros."""
    p = np.zeros((nbins + 1, nbins), np.float32)
    p[np.arange(nbins), np.arange(nbins)] = 1024.0
    return p


def caller_banks(nbins):
    """Filterbanks a caller may hand to vv_dsp_compute_log_mel_spectrogram:
    name -> float32 [filters][nbins]."""
    rng = np.random.default_rng(nbins)
    banks = {}
    gaps = np.zeros((6, nbins), np.float32)   # zeros inside each filter's range
    for m in range(6):
        lo = 3 + m * (nbins // 7)
        gaps[m, lo:lo + 37] = rng.random(37).astype(np.float32)
        gaps[m, lo + 5:lo + 30:3] = 0.0
        gaps[m, lo + 10:lo + 19] = 0.0
    banks["gaps"] = gaps
    ends = np.zeros((2, nbins), np.float32)   # single bins at 0 and nbins - 1
    ends[0, 0], ends[1, nbins - 1] = 0.75, 1.5
    banks["ends"] = ends
    banks["zero"] = np.zeros((5, nbins), np.float32)
    # mixed signs: every filter has a dominant positive part, so that
    # e + eps >= 0.1 sum|w p| holds for power in [1, 2] (asserted by the test)
    mixed = rng.random((7, nbins)).astype(np.float32)
    mixed[:, 1::3] *= -0.5
    mixed[3, : nbins // 2] = 0.0
    banks["mixed"] = mixed
    banks["dense"] = rng.random((40, nbins)).astype(np.float32)
    return banks
