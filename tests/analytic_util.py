"""Float64 references, the per-pair error measure and the launch helpers of
tests/test_gpu_analytic_rows.py (batched Hilbert and DCT rows:
shim_analytic.hip, hilbert_fused.hpp, dct2_fused.hpp, spectral_kernels.hip).

The measure.  The fused kernels put rows 2j and 2j + 1 of a batch into one
complex FFT (z = a + i b), so the rounding error of either row scales with the
larger of the two: an f32 two-for-one DCT-II on the CPU (complex64, 200 random
pairs per size, n = 16...8192) has a row error of 2.0e-7...2.3e-7 of the pair's
max-abs with rows of one scale, and with the partner scaled by 1e-4 the small
row is off by 1.2e-3...1.7e-3 of its own max-abs but by 0.8e-7...1.4e-7 of the
pair's.  So the unit of the check is the pair:

    err_j = max |y - ref| over rows 2j, 2j + 1  /  max |ref| over rows 2j, 2j + 1

(the last row alone when the batch is odd), and every err_j is held to the
project's bound for these operations, 2e-6 * max(1, log2 n)
(test_hilbert_batched_device, test_dct2_batched_device), which those tests
apply to one number over the whole batch.  A wrong small row, or a row stored
in its neighbour's slot, moves its own pair's err_j to order 1.  The multi-pass
routes have no pairs; there the pair is only the grouping.
"""
import ctypes as C
import functools

import numpy as np

GUARD = 3          # NaN rows behind every output
FLT_MAX = 3.402823466e+38
ST_OK, ST_RANGE, ST_NAN = 0, 3, 5

# (what, n) -> worst err / bound seen in this process (printed per call as well:
# run with -s to collect the figures of the module docstring)
WORST = {}


def bound(n):
    return 2e-6 * max(1.0, np.log2(n))


def assert_pairs(y, ref, n, rows=None, only=None, what=""):
    """Every pair of the given rows meets bound(n).

    y, ref: (R, n) arrays, row i being row rows[i] of the batch (default i).
    Rows are grouped by rows // 2.  `only`: batch rows whose error counts (the
    others of the group still count in the group's max |ref|); groups without
    such a row are left out.  -> worst err / bound."""
    y, ref = np.asarray(y), np.asarray(ref)
    assert y.shape == ref.shape and y.ndim == 2 and y.shape[1] == n, (y.shape, ref.shape, n)
    rows = np.arange(y.shape[0]) if rows is None else np.asarray(rows)
    assert rows.shape == (y.shape[0],)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.abs(y.astype(ref.dtype) - ref)
    num = np.where(np.isnan(diff), np.inf, diff).max(axis=1)
    den = np.abs(ref).max(axis=1)
    b = bound(n)
    worst, worst_j = 0.0, None
    for j in np.unique(rows // 2):
        grp = rows // 2 == j
        cnt = grp if only is None else grp & np.isin(rows, list(only))
        if not cnt.any():
            continue
        e, d = num[cnt].max(), den[grp].max()
        err = (0.0 if e == 0 else np.inf) if d == 0 else e / d
        if worst_j is None or err > worst:
            worst, worst_j = err, j
    assert worst_j is not None, "no rows to check"
    ratio = worst / b
    key = (what.split()[0] if what else "", n)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"analytic_rows {what} n={n} rows={y.shape[0]} worst err/bound {ratio:.4f} (pair {worst_j})")
    assert worst <= b, (f"{what} n={n}: pair {worst_j} (rows {2 * worst_j}, {2 * worst_j + 1}) "
                        f"err {worst:.3e} > bound {b:.3e}")
    return ratio


# ---------------------------------------------------------------- references
@functools.lru_cache(maxsize=1)
def _cos3(n):
    """cos(pi k (m + 1/2) / n), k < n rows, m = 1...n-1 columns (test_dct_types_vs_formula)"""
    kk = np.arange(n)[:, None]
    mm = np.arange(1, n)[None, :]
    return np.cos(np.pi * kk * (mm + 0.5) / n)


def dct_ref(x64, dct_type, inverse):
    """The f64 rows vv_dsp_dct_execute gives (dct.c:21-68), with the scalings of
    test_dct_types_vs_formula: II forward dct2 / 2; II and III backward
    idct2(2 x); IV forward dct4 / 2, backward dct4 / n; III forward
    y[k] = x[0] + 2 sum_{m >= 1} x[m] cos(pi k (m + 1/2) / n)."""
    import scipy.fft
    n = x64.shape[-1]
    if dct_type == 2 and not inverse:
        return scipy.fft.dct(x64, 2, axis=-1) / 2
    if dct_type in (2, 3) and inverse:
        return scipy.fft.idct(2 * x64, 2, axis=-1)
    if dct_type == 4:
        return scipy.fft.dct(x64, 4, axis=-1) / (n if inverse else 2)
    assert dct_type == 3
    if n == 1:
        return x64.copy()
    return x64[:, :1] + 2 * (x64[:, 1:] @ _cos3(n).T)


def hilbert_ref(x64):
    import scipy.signal
    return scipy.signal.hilbert(x64, axis=1)


def policy_on_read(x64, policy):
    """src/core/nan_policy.c on the input: 1 IGNORE non-finite -> 0, 3 CLAMP NaN -> 0, +-Inf -> +-FLT_MAX"""
    x = x64.copy()
    if policy == 1:
        x[~np.isfinite(x)] = 0.0
    elif policy == 3:
        x[np.isnan(x)] = 0.0
        x[np.isposinf(x)] = FLT_MAX
        x[np.isneginf(x)] = -FLT_MAX
    return x


# ---------------------------------------------------------------- launches
def rows_input(batch, n, seed, scale=None):
    """iid normal rows generated on the device; scale: per-row factors (cycled)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(batch, n, device="cuda", generator=g)
    if scale is not None:
        s = torch.tensor([scale[r % len(scale)] for r in range(batch)], device="cuda")
        x = x * s[:, None]
    return x


def run_dct(vv, x, dct_type=2, inverse=False, fill=float("nan")):
    """vv_dsp_dct_execute_device on x (batch, n) into rows with GUARD rows of
    `fill` behind them -> (status, all rows as one (batch + GUARD, n) tensor)"""
    import torch
    L = vv.lib()
    batch, n = x.shape
    full = torch.full((batch + GUARD, n), fill, device="cuda")
    assert x.is_contiguous() and x.data_ptr() % 16 == 0 and full.data_ptr() % 16 == 0   # the staged kernels' gate
    pl = C.c_void_p()
    assert L.vv_dsp_dct_make_plan(n, dct_type, -1 if inverse else 1, C.byref(pl)) == 0
    try:
        st = L.vv_dsp_dct_execute_device(pl, C.c_void_p(x.data_ptr()), C.c_void_p(full.data_ptr()), batch,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    finally:
        L.vv_dsp_dct_destroy(pl)
    torch.cuda.synchronize()
    return st, full


def run_hilbert(vv, x):
    """vv_dsp_hilbert_analytic_device on x (batch, n) -> (status, all rows as one
    (batch + GUARD, 2 n) float tensor of NaN-guarded interleaved re, im)"""
    import torch
    L = vv.lib()
    batch, n = x.shape
    full = torch.full((batch + GUARD, 2 * n), float("nan"), device="cuda")
    assert x.is_contiguous() and x.data_ptr() % 16 == 0 and full.data_ptr() % 16 == 0
    st = L.vv_dsp_hilbert_analytic_device(C.c_void_p(x.data_ptr()), n, batch, C.c_void_p(full.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st, full


def guards_intact(full, batch):
    import torch
    return bool(torch.isnan(full[batch:]).all())


def as_complex(a):
    """(R, 2 n) float32 ndarray of interleaved re, im -> (R, n) complex64"""
    return np.ascontiguousarray(a).view(np.complex64)
