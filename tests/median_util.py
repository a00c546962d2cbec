"""The numpy model of include/vv_dsp/filter/median.h and include/vv_dsp/spectral/hpss.h,
shared by test_median_host.py, test_gpu_medfilt.py and test_gpu_hpss.py.

The median is written twice, independently: `median_sort` sorts a window's keys and
takes rank h; `median_count` takes no order at all -- for every candidate it counts the
keys below it and the keys not above it and keeps the one whose two counts bracket h.
The host tests hold the two equal bit for bit on every case the GPU tests run."""
import numpy as np

OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_INTERNAL, ERR_NAN, ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5, 6
REFLECT, NEAREST, ZERO = 0, 1, 2
HARD, SOFT, WIENER = 0, 1, 2
QNAN = np.uint32(0x7FC00000)
MAX_WINDOW, MAX_BINS = 127, 8193


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def canon(x):
    """float32 array with every NaN replaced by the quiet NaN 0x7FC00000"""
    x = np.array(x, dtype=np.float32, copy=True)
    b = x.view(np.uint32)
    b[np.isnan(x)] = QNAN
    return x


def keys(x):
    b = bits(canon(x))
    return np.where(b & np.uint32(0x80000000), b ^ np.uint32(0xFFFFFFFF), b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return b.view(np.float32)


def fold(i, n, mode):
    """indices that stand for i (any integers) on a line of n values; -1: the value +0.0"""
    i = np.asarray(i, dtype=np.int64)
    inside = (i >= 0) & (i < n)
    if mode == ZERO:
        return np.where(inside, i, -1)
    if mode == NEAREST:
        return np.clip(i, 0, n - 1)
    assert mode == REFLECT
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def windows(x, L, mode, axis=-1):
    """keys of every window: shape x.shape + (L,), the window of position i along `axis`"""
    x = np.moveaxis(np.asarray(x, dtype=np.float32), axis, -1)
    n, h = x.shape[-1], L // 2
    k = np.concatenate([keys(x), np.full(x.shape[:-1] + (1,), 0x80000000, np.uint32)], axis=-1)   # [-1]: +0.0
    idx = fold(np.arange(n)[:, None] + np.arange(-h, h + 1)[None, :], n, mode)
    return k[..., idx]            # (..., n, L)


def median_sort(x, L, mode=REFLECT, axis=-1):
    w = np.sort(windows(x, L, mode, axis), axis=-1)
    return np.moveaxis(unkey(w[..., L // 2]), -1, axis)


def median_count(x, L, mode=REFLECT, axis=-1):
    w = windows(x, L, mode, axis)
    h = L // 2
    out = np.zeros(w.shape[:-1], np.uint32)
    done = np.zeros(w.shape[:-1], bool)
    for i in range(L):
        c = w[..., i:i + 1]
        below = (w < c).sum(axis=-1)
        upto = (w <= c).sum(axis=-1)
        hit = (below <= h) & (h < upto) & ~done
        out[hit] = w[..., i][hit]
        done |= hit
    assert done.all()
    return np.moveaxis(unkey(out), -1, axis)


def weights(power, magnitude):
    p = np.asarray(power, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return canon(np.sqrt(p) if magnitude else p)


def mask_of(a, b, margin, kind):
    """hpss.h's mask of this median a against the other b: float32 arrays -> float32"""
    a = a.astype(np.float64)
    b = np.float64(np.float32(margin)) * b.astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == HARD:
            return (a > b).astype(np.float32)
        if kind == WIENER:
            a = a * a
            b = b * b
        d = a + b
        q = np.where(d == 0.0, 0.5, a / np.where(d == 0.0, 1.0, d))
        return canon(q.astype(np.float32))


def hpss_model(power, n_fft, magnitude, win_harm, win_perc, margin_harm, margin_perc, kind, rows_per_group=0,
               median=median_sort):
    """{harm, perc, mask_harm, mask_perc} of packed rows (rows, K)"""
    p = np.asarray(power, dtype=np.float32)
    rows, K = p.shape
    assert K == n_fft // 2 + 1
    w = weights(p, magnitude)
    rpg = rows if rows_per_group == 0 or rows_per_group > rows else rows_per_group
    H = np.empty_like(w)
    for r0 in range(0, rows, max(rpg, 1)):
        H[r0:r0 + rpg] = median(w[r0:r0 + rpg], win_harm, REFLECT, axis=0)
    P = median(w, win_perc, REFLECT, axis=1)
    return {"harm": H, "perc": P, "mask_harm": mask_of(H, P, margin_harm, kind),
            "mask_perc": mask_of(P, H, margin_perc, kind)}


# ---- fixtures -------------------------------------------------------------------------
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF,
                     0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FA5A5A5], np.uint32).view(np.float32)
MEDFILT_N = (1, 2, 5, 63, 64, 65, 1000, 4099)
MEDFILT_L = (1, 3, 5, 31, 33, 127)


def medfilt_rows(n, seed, batch=3):
    """`batch` rows of n: seeded floats quantised to 8 levels (windows full of ties), a
    fifth of the positions +-0, +-inf, denormals and NaNs of both signs with payloads"""
    rng = np.random.default_rng(seed)
    x = (np.floor(rng.uniform(-4, 4, (batch, n))) * 0.25).astype(np.float32)
    sp = rng.random((batch, n)) < 0.2
    x[sp] = SPECIALS[rng.integers(0, len(SPECIALS), int(sp.sum()))]
    return x


HPSS_SHAPES = ((2, 1), (64, 2), (64, 7), (256, 28), (1024, 200))     # (n_fft, T)
HPSS_WINDOWS = ((1, 1), (9, 9), (31, 17))                            # (127, 127) runs on T = 7


def hpss_rows(n_fft, T, seed):
    """power rows (T, K): quantised noise with ties, a zero column, a negative power and a NaN"""
    rng = np.random.default_rng(seed)
    K = n_fft // 2 + 1
    p = (np.floor(rng.uniform(0, 6, (T, K))) ** 2 * 0.125).astype(np.float32)
    p *= (1.0 + rng.integers(0, 3, (1, K))).astype(np.float32)         # some structure along frequency
    p[:, K // 2] = 0.0
    if K > 2:
        p[:, K // 2 - 1] = 0.0                                          # zero neighbours: P is 0 there too
    p[T // 2, K // 3] = -1.0
    p[T // 3, K - 1] = SPECIALS[-1]
    return p


SR, SIG_N = 8000, 2000


def separation_signals():
    """(tone, clicks, noise), float32, of the issue's fixture"""
    t = np.arange(SIG_N) / SR
    tone = (0.5 * np.sin(2 * np.pi * 500 * t) + 0.3 * np.sin(2 * np.pi * 1250 * t)).astype(np.float32)
    clicks = np.zeros(SIG_N, np.float32)
    clicks[300::450] = 1.0
    clicks[301::450] = -0.8
    noise = (1e-3 * np.random.default_rng(7).standard_normal(SIG_N)).astype(np.float32)
    return tone, clicks, noise


def stft64(x, n_fft=256, hop=64):
    """float64 STFT rows (T, K) with the symmetric Hann window, frames as the library counts them"""
    x = np.asarray(x, dtype=np.float64)
    T = 1 if len(x) < n_fft else 1 + (len(x) - n_fft + hop) // hop
    xp = np.concatenate([x, np.zeros(max(0, (T - 1) * hop + n_fft - len(x)))])
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / (n_fft - 1))
    fr = np.stack([xp[t * hop:t * hop + n_fft] * win for t in range(T)])
    return np.fft.rfft(fr, axis=1)


def kept(mask, spec):
    """the share of spec's energy that the mask keeps"""
    e = np.abs(spec) ** 2
    return float(((mask.astype(np.float64) ** 2) * e).sum() / e.sum())
