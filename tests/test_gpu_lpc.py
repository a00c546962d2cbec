"""GPU tests of the batched LPC (lpc_kernels.hip, shim_lpc.hip) against the
reference's outputs in tests/golden/lpc_*.npz.

What is compared how:
  * autocorrelation rows against the f64 sums, with the bound
    max(2 x the reference's own error over the case, 2^-22) on
    max|r - r_f64| / r_f64[0] (another summation order draws another sample of
    the same error class; an exact sum still rounds once);
  * Levinson bit for bit against the reference's a / err on the reference's r,
    through both kernels;
  * lpc bit for bit against levinson(autocorr), the host call against the
    batch row, lpc_frames bit for bit against fetch_frames -> lpc; end to end
    against the reference on the white rows only, at the harness tolerance
    (the resonant rows' coefficients hang on conditioning);
  * lpspec against the f64 model with the exact residue (m k) mod nfft, bound
    max(2 x the reference's own error for that row, 2^-22) on the relative error.
"""
import numpy as np
import pytest

import frames_util
from conftest import tolerances
from frames_util import fetch_frames, hamming
from lpc_util import (LpcApi, CASES, GENERIC_CASES, WHITE_ROWS, SPEC_NFFT, SENTINEL, ERR_INTERNAL, OK, key, load)

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22


@pytest.fixture(scope="module")
def cases():
    return load("lpc_cases")


@pytest.fixture(scope="module")
def spec():
    return load("lpc_spec")


@pytest.fixture(scope="module")
def signals():
    return load("lpc_signals")


@pytest.fixture
def counters(vdev):
    vdev.debug_clear("STAT_LPC_WAVE")
    vdev.debug_clear("STAT_LPC_GENERIC")
    return lambda: (vdev.debug_get("STAT_LPC_WAVE"), vdev.debug_get("STAT_LPC_GENERIC"))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tiled(rows, batch):
    return np.ascontiguousarray(np.tile(rows, ((batch + len(rows) - 1) // len(rows), 1))[:batch])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- 1. autocorrelation
@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("n,order", CASES)
def test_autocorr_rows(vdev, cases, knob, counters, n, order, generic):
    if generic:
        knob("LPC_GENERIC", 1)
    x = tiled(cases[key(n, order, "x")], 67)       # not a multiple of 64, more than one wave
    r64 = cases[key(n, order, "r_f64")]
    r = vdev.autocorr(dev(x), order).cpu().numpy().astype(np.float64)
    assert r.shape == (67, order + 1)
    own = np.max(np.abs(cases[key(n, order, "r_ref")].astype(np.float64) - r64), axis=1) / r64[:, 0]
    bound = max(2.0 * own.max(), FLOOR)
    want = tiled(r64, 67)
    got = np.max(np.abs(r - want), axis=1) / want[:, 0]
    print(f"autocorr n={n} order={order} generic={generic}: max {got.max():.3e}, reference {own.max():.3e}, "
          f"bound {bound:.3e}")
    assert got.max() <= bound
    wave, gen = counters()
    assert (wave, gen) == ((0, 1) if generic or (n, order) in GENERIC_CASES else (1, 0))


# ---------------------------------------------------------------- 2. Levinson
@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("n,order", CASES)
def test_levinson_rows_bit_identical(vdev, cases, knob, counters, n, order, generic):
    if generic:
        knob("LPC_GENERIC", 1)
    r = tiled(cases[key(n, order, "r_ref")], 130)
    a_ref = tiled(cases[key(n, order, "a_ref")], 130)
    err_ref = tiled(cases[key(n, order, "err_ref")][:, None], 130)[:, 0]
    r[63, 0] = 0.0        # the silent frame and a negative r[0], mid-batch across a wave boundary
    r[64, 0] = -1.0
    a, err = vdev.levinson(dev(r))
    a, err = a.cpu().numpy(), err.cpu().numpy()
    keep = np.ones(130, bool)
    keep[63:65] = False
    assert same_bits(a[keep], a_ref[keep])
    assert same_bits(err[keep], err_ref[keep])
    unit = np.zeros(order + 1, np.float32)
    unit[0] = 1.0
    for i in (63, 64):
        assert same_bits(a[i], unit) and err[i] == 0.0
    wave, gen = counters()
    assert (wave, gen) == ((0, 1) if generic or order > 32 else (1, 0))


def test_levinson_nan_propagates_like_the_reference(vdev, cases):
    """lpc.c:25 compares e <= 0, which a NaN passes: the row runs the recursion."""
    r = cases[key(400, 16, "r_ref")][:3].copy()
    r[1, 0] = np.nan
    a, err = vdev.levinson(dev(r))
    a, err = a.cpu().numpy(), err.cpu().numpy()
    assert a[1, 0] == 1.0 and np.isnan(a[1, 1:]).all() and np.isnan(err[1])
    assert same_bits(a[[0, 2]], cases[key(400, 16, "a_ref")][[0, 2]])


# ---------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("n,order", CASES)
def test_lpc_is_levinson_of_autocorr(vdev, amd, cases, n, order):
    x = tiled(cases[key(n, order, "x")], 67)
    dx = dev(x)
    a, err = vdev.lpc(dx, order)
    a2, err2 = vdev.levinson(vdev.autocorr(dx, order))
    a, err = a.cpu().numpy(), err.cpu().numpy()
    assert same_bits(a, a2.cpu().numpy()) and same_bits(err, err2.cpu().numpy())
    # the host call (the reference's signature) on one row is the batch's row
    st, ha, herr = LpcApi(amd.lib).lpc(x[3], order)
    assert st == OK
    assert same_bits(ha, a[3]) and same_bits(np.float32(herr), err[3])
    # end to end on the white rows: the reference's own error there is below 2e-6
    rtol, atol = tolerances()
    np.testing.assert_allclose(a[WHITE_ROWS], cases[key(n, order, "lpc_a_ref")][WHITE_ROWS], rtol=rtol, atol=atol)
    np.testing.assert_allclose(err[WHITE_ROWS], cases[key(n, order, "lpc_err_ref")][WHITE_ROWS], rtol=rtol,
                               atol=atol)


def test_host_calls_match_device_rows_and_reference_statuses(vdev, amd, cases):
    api = LpcApi(amd.lib)
    want = dict(zip((str(s) for s in cases["arg_names"]), (int(s) for s in cases["arg_status"])))
    got = api.argument_cases(device=True)
    assert got == want
    # a silent row: INTERNAL from the device with the row, outputs untouched (lpc.c:25, :50)
    st, a, err = api.lpc(np.zeros(64, np.float32), 8)
    assert st == ERR_INTERNAL and np.all(a == SENTINEL) and err == SENTINEL
    x = cases[key(400, 16, "x")]
    st, r = api.autocorr(x[7], 16)
    assert st == OK and same_bits(r, vdev.autocorr(dev(x), 16).cpu().numpy()[7])
    st, a, err = api.levinson(cases[key(400, 16, "r_ref")][7])
    assert st == OK and same_bits(a, cases[key(400, 16, "a_ref")][7])
    assert same_bits(np.float32(err), cases[key(400, 16, "err_ref")][7])
    st, a, err = api.levinson(np.array([2.0], np.float32))     # order 0: the reference leaves a[0] = 0
    assert st == OK and same_bits(a, np.zeros(1, np.float32)) and err == 2.0


# ---------------------------------------------------------------- 4. fused frames
@pytest.fixture(scope="module")
def three_channels(signals):
    return frames_util.three_channels(signals["white"], signals["resonant"])


@pytest.mark.parametrize("windowed", [0, 1])
@pytest.mark.parametrize("center", [0, 1])
@pytest.mark.parametrize("frame,hop,order", [(400, 160, 16), (33, 7, 32), (64, 64, 1), (600, 200, 128)])
def test_lpc_frames_is_the_pipeline(vdev, three_channels, counters, frame, hop, order, center, windowed):
    import torch
    sig = three_channels
    assert sig.stride(0) == 16004
    win = dev(hamming(frame)) if windowed else None
    a, err = vdev.lpc_frames(sig, frame, hop, order, window=win, center=bool(center))
    wave, gen = counters()
    assert (wave, gen) == ((0, 1) if order > 32 else (1, 0))
    fr = vdev.num_frames(16000, frame, hop, center)
    assert a.shape == (3, fr, order + 1) and err.shape == (3, fr) and fr > 64
    for c in range(3):
        rows = fetch_frames(vdev, sig[c].contiguous(), frame, hop, center, win)
        a2, err2 = vdev.lpc(rows, order)
        assert torch.equal(a[c].view(torch.int32), a2.view(torch.int32)), (c,)
        assert torch.equal(err[c].view(torch.int32), err2.view(torch.int32)), (c,)


def test_lpc_frames_zero_frames_and_sizes(vdev, three_channels):
    import torch
    L = vdev.lib()
    sig = three_channels
    a = torch.full((3, 4, 17), float(SENTINEL), dtype=torch.float32, device="cuda")
    err = torch.full((3, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(n, frame, hop, center, order):
        return L.vv_dsp_lpc_frames_device(sig.data_ptr(), n, 3, 16004, frame, hop, center, None, order, a.data_ptr(),
                                          4 * 17, err.data_ptr(), 4, s)

    assert call(100, 400, 160, 0, 16) == OK        # n < frame_len, not centred: no frames
    torch.cuda.synchronize()
    assert bool((a == float(SENTINEL)).all()) and bool((err == float(SENTINEL)).all())
    assert call(16000, 400, 0, 0, 16) == 2
    assert call(16000, 0, 160, 0, 0) == 2
    assert call(16000, 16, 160, 0, 16) == 2        # order + 1 > frame_len
    assert L.vv_dsp_lpc_frames_device(None, 16000, 3, 16004, 400, 160, 0, None, 16, a.data_ptr(), 68, err.data_ptr(),
                                      4, s) == 1


# ---------------------------------------------------------------- 5. lpspec
@pytest.mark.parametrize("sign", [0, 1])
@pytest.mark.parametrize("nfft", SPEC_NFFT)
def test_lpspec(vdev, amd, spec, nfft, sign):
    import torch
    api = LpcApi(amd.lib)
    gains = spec["gain"]
    for i in range(4):
        a = dev(spec[f"a{i}"])
        m64 = spec[f"mag_f64_s{sign}_{nfft}"][i]
        own = np.max(np.abs(spec[f"mag_ref_s{sign}_{nfft}"][i].astype(np.float64) - m64) / m64)
        bound = max(2.0 * own, FLOOR)
        mag = vdev.lpspec(a, nfft, gain=dev(gains[i:i + 1]), levinson_sign=bool(sign))
        got = np.max(np.abs(mag.cpu().numpy().astype(np.float64) - m64) / m64)
        print(f"lpspec nfft={nfft} sign={sign} row={i}: max {got:.3e}, reference {own:.3e}, bound {bound:.3e}")
        assert mag.shape == (nfft,)
        assert got <= bound
        if gains[i] == 1.0:     # no gain pointer means gain 1
            assert torch.equal(vdev.lpspec(a, nfft, levinson_sign=bool(sign)), mag)
        if sign == 0:           # the host call keeps the reference's convention
            st, hmag = api.lpspec(spec[f"a{i}"], float(gains[i]), nfft)
            assert st == OK and same_bits(hmag, mag.cpu().numpy())
    # rows of one order as a batch with per-row gains: each row as alone
    a2 = dev(np.stack([spec["a1"], spec["a2"]]))
    both = vdev.lpspec(a2, nfft, gain=dev(gains[1:3]), levinson_sign=bool(sign))
    for j, i in enumerate((1, 2)):
        alone = vdev.lpspec(dev(spec[f"a{i}"]), nfft, gain=dev(gains[i:i + 1]), levinson_sign=bool(sign))
        assert torch.equal(both[j], alone)


def test_lpspec_levinson_sign_gives_the_envelope(vdev, cases):
    """The reference's 1 - sum convention on Levinson's coefficients flattens the
    envelope of a resonant frame; levinson_sign restores it."""
    a = dev(cases[key(400, 16, "lpc_a_ref")][5])
    flat = vdev.lpspec(a, 512).cpu().numpy()
    env = vdev.lpspec(a, 512, levinson_sign=True).cpu().numpy()
    assert env.max() / env.min() > 10 * flat.max() / flat.min()


# ---------------------------------------------------------------- 6. the binding's checks
def test_binding_shape_checks(vdev):
    import torch
    x = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
    with pytest.raises(vdev.VvError):
        vdev.autocorr(x.double(), 8)
    with pytest.raises(vdev.VvError):
        vdev.lpc(x, 64)                                    # order + 1 > n
    with pytest.raises(vdev.VvError):
        vdev.autocorr(x[:, ::2], 8)                        # not contiguous
    with pytest.raises(vdev.VvError):
        vdev.levinson(x.to(torch.float16))
    with pytest.raises(vdev.VvError):
        vdev.lpc_frames(x, 32, 16, 8, window=torch.ones(31, device="cuda"))
    with pytest.raises(vdev.VvError):
        vdev.lpc_frames(x, 32, 16, 32)
    with pytest.raises(vdev.VvError):
        vdev.lpc_frames(x.double(), 32, 16, 8)
    with pytest.raises(vdev.VvError):
        vdev.lpspec(x, 16, gain=torch.ones(3, device="cuda"))
    with pytest.raises(vdev.VvError):
        vdev.lpspec(x.double(), 16)
