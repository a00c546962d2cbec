"""The two FIR launch routes that only a knob reaches.

FIR_DIRECT_LDS=1: the LDS direct-form kernel (k_fir_direct) instead of the
register one (k_fir_reg).  Both promise the reference's sums in the reference's
order, so they must agree bit for bit -- for `apply` and for both filtfilt
passes -- at one output, at exactly one register tile (4096 outputs), and one
past it with an odd row stride (the element-by-element sample path), with a
partial tap tile (1), one full tile (16), full plus partial (17) and config 4's
filter length (257).

FIR_R32=0 with FIR_OLD=1: the bulk pairs through the LDS-DMA kernel
(k_fir_pair<1024, true>) and the edge pairs through k_fir_pair<1024, false>.
None of the other routes' counters may move; the bounds are those of
test_fir_r32_vs_direct_and_previous (same filter, same input range)."""
import numpy as np
import pytest
import vvdsp_amd as vv

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 4096), (3, 4097)]


def _plan(vdev, taps):
    import torch
    h = np.random.default_rng(taps).uniform(-1, 1, taps).astype(np.float32)
    return vdev.FirPlan(torch.from_numpy(h))


def _input(nch, n):
    import torch
    g = torch.Generator(device="cuda").manual_seed(nch * 31 + n % 1013)
    return torch.rand(nch, n, device="cuda", generator=g) * 2 - 1


@pytest.mark.parametrize("nch,n", SHAPES)
@pytest.mark.parametrize("taps", [1, 16, 17, 257])
def test_fir_direct_lds_equals_register_kernel(vdev, taps, nch, n):
    import torch
    plan = _plan(vdev, taps)
    x = _input(nch, n)
    y = plan(x, direct=True)
    with vv.knobs(FIR_DIRECT_LDS=1):
        yl = plan(x, direct=True)
    torch.cuda.synchronize()
    assert torch.equal(yl, y)


@pytest.mark.parametrize("nch,n", SHAPES[1:])
@pytest.mark.parametrize("taps", [17, 257])
def test_filtfilt_lds_equals_register_kernel(vdev, taps, nch, n):
    import torch
    plan = _plan(vdev, taps)
    x = _input(nch, n)
    y = plan.filtfilt(x)
    with vv.knobs(FIR_DIRECT_LDS=1):
        yl = plan.filtfilt(x)
    torch.cuda.synchronize()
    assert torch.equal(yl, y)


# multiple-of-4 channel lengths (16 B aligned channels) with a front edge pair,
# at least one bulk pair and a tail edge pair per channel: 1536 outputs per pair
@pytest.mark.parametrize("nch,n", [(3, 3940), (2, 7684)])
def test_fir_pair_route(vdev, orc, nch, n):
    import torch
    plan = vdev.FirPlan(torch.from_numpy(orc.fir_design_lowpass(257, 0.25, 2)))
    x = _input(nch, n)
    stats = ("STAT_FIR_R32", "STAT_FIR_DYN", "STAT_FIR_STATIC")
    before = [vv.debug_get(s) for s in stats]
    with vv.knobs(FIR_R32=0, FIR_OLD=1):
        y = plan(x)
        y2 = plan(x)
    torch.cuda.synchronize()
    assert [vv.debug_get(s) for s in stats] == before
    yd = plan(x, direct=True)
    with vv.knobs(FIR_R32=0):
        yo = plan(x)
    torch.cuda.synchronize()
    err_direct, err_reg = (y - yd).abs().max().item(), (y - yo).abs().max().item()
    print("pair route (%d, %d): |y - direct| %.3g, |y - bulk_reg| %.3g" % (nch, n, err_direct, err_reg))
    assert err_direct < 1e-5
    assert err_reg < 2e-6
    assert torch.equal(y, y2)
