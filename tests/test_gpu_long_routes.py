"""GPU tests of the long-transform routes: every geometry and variant of the
two-pass four-step kernels, the five-pass transpose path, and the element-wise
glue of the unfused chirp-z chain.

The four-step bound is test_gpu_parity.py's test_large_pow2_chunked_batch's:
each row against NumPy f64 by harness_or_normwise with SciPy's f32 FFT of the
same row as the yardstick, factor 4."""
import functools

import numpy as np
import pytest

from test_gpu_parity import harness_or_normwise

pytestmark = pytest.mark.gpu

BATCH = 3
# n, the knobs that send it to the four-step kernels: N1 = 64 (the smallest column
# length; 8192 runs in one workgroup unless C2C_MAX says otherwise), N1 = N2 = 128, N1 != N2
GEOMETRIES = [(8192, {"C2C_MAX": 4096}), (16384, {}), (32768, {})]
VARIANTS = [{"FS_VAR": 0}, {"FS_VAR": 1}, {"FS_VAR": 2}, {"FS_VAR": 3}, {"FS_CHUNK_MB": 1}]


def chunked_batch(n):
    """one transform more than FS_CHUNK_MB=1 puts in a chunk, (1 MiB) / (8 n): a full
    chunk, then the loop's second turn with b0 > 0 and a chunk of one (17, 9, 5 rows)"""
    return (1 << 20) // (8 * n) + 1


@functools.lru_cache(maxsize=None)
def _case(n, batch):
    """input rows, their f64 transforms both ways and SciPy's f32 ones (computed once per shape, read-only)"""
    import scipy.fft
    rng = np.random.default_rng(n + batch)
    x = (rng.random((batch, n)) - 0.5 + 1j * (rng.random((batch, n)) - 0.5)).astype(np.complex64)
    x64 = x.astype(np.complex128)
    out = (x, np.fft.fft(x64, axis=1), np.fft.ifft(x64, axis=1), scipy.fft.fft(x, axis=1), scipy.fft.ifft(x, axis=1))
    for a in out:
        a.setflags(write=False)
    return out


def _check_both_ways(vdev, knob, n, batch, knobs):
    import torch
    x, f64, b64, f32, b32 = _case(n, batch)
    xd = torch.tensor(x, device="cuda")
    for k, v in knobs.items():
        knob(k, v)
    yf = vdev.FftPlan(n, vdev.C2C, vdev.FWD, batch=batch)(xd).cpu().numpy()
    yb = vdev.FftPlan(n, vdev.C2C, vdev.BWD, batch=batch)(xd).cpu().numpy()
    for i in range(batch):
        harness_or_normwise(yf[i], f64[i], f32[i], 4)
        harness_or_normwise(yb[i], b64[i], b32[i], 4)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join("%s%d" % kv for kv in v.items()))
@pytest.mark.parametrize("n,route", GEOMETRIES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_fourstep_geometry_variant(vdev, knob, n, route, variant):
    """k_fs_cols / k_fs_rows at N1 = 64, N1 = N2 and N1 != N2, with the RI and float2
    exchanges at 16 and 8 transforms per workgroup (FS_VAR 0..3) on 3 rows, and a
    batch cut into two chunks (FS_CHUNK_MB=1, chunked_batch rows), forward and backward."""
    batch = chunked_batch(n) if "FS_CHUNK_MB" in variant else BATCH
    _check_both_ways(vdev, knob, n, batch, {**route, **variant})


@pytest.mark.parametrize("n,batch,knobs",
                         [(16384, BATCH, {"FS_OLD": 1}), (32768, BATCH, {"FS_OLD": 1}), (1 << 21, 1, {})],
                         ids=["16384-FS_OLD", "32768-FS_OLD", "2^21"])
def test_fivepass_path(vdev, knob, n, batch, knobs):
    """transpose, N1-point FFTs, twiddled transpose, N2-point FFTs, transpose: the
    route of n > 2^20, and of the shorter lengths under FS_OLD=1 (square and N1 != N2)."""
    _check_both_ways(vdev, knob, n, batch, knobs)


def _czt_plan(vdev, n, m):
    w, a = np.exp(-2j * np.pi * 0.13 / m), np.exp(0.2j)
    w, a = complex(np.complex64(w)), complex(np.complex64(a))
    return vdev.CztPlan(n, m, w, a), w, a


def test_czt_unfused_chain_vs_host(vdev, amd):
    """N = 3000, M = 1200: P = 8192 is above the one-pass kernel, so the rows go
    through the element-wise pre / product / post kernels around the library's
    FFTs.  Three rows, complex and real: bit-identical to the C API's one-row host
    call, and within test_gpu_czt.py's 1e-5 (normwise) of scipy.signal.czt in f64."""
    import torch
    from scipy.signal import czt
    from test_gpu_czt import _eff, _normwise
    n, m = 3000, 1200
    plan, w, a = _czt_plan(vdev, n, m)
    g = torch.Generator(device="cuda").manual_seed(n + m)
    xc = torch.complex(torch.randn(3, n, device="cuda", generator=g), torch.randn(3, n, device="cuda", generator=g))
    for x in (xc, xc.real.contiguous()):
        y = plan(x).cpu().numpy()
        xh = x.cpu().numpy()
        for r in range(3):
            st, host = amd.czt_status(xh[r], m, w, a)
            assert st == 0
            np.testing.assert_array_equal(y[r], host)
            ref = czt(xh[r].astype(np.complex128 if np.iscomplexobj(xh) else np.float64), m=m, w=_eff(w), a=_eff(a))
            assert _normwise(y[r], ref) <= 1e-5, (r, _normwise(y[r], ref))


def test_czt_unfused_equals_fused_small(vdev, knob):
    """N = 300, M = 200 (P = 512): the element-wise chain under CZT_UNFUSED=1 gives
    the one-pass kernel's rows bit for bit, complex and real input."""
    import torch
    n, m = 300, 200
    plan, _, _ = _czt_plan(vdev, n, m)
    g = torch.Generator(device="cuda").manual_seed(n + 3 * m)
    xc = torch.complex(torch.randn(3, n, device="cuda", generator=g), torch.randn(3, n, device="cuda", generator=g))
    for x in (xc, xc.real.contiguous()):
        knob("CZT_UNFUSED", "0")
        fused = plan(x)
        knob("CZT_UNFUSED", "1")
        chain = plan(x)
        knob("CZT_UNFUSED", "")
        torch.cuda.synchronize()
        assert torch.equal(fused, chain)
