"""The resampler on the GPU: every recorded reference output
(tests/golden/resample_*.npz) through the host-pointer API and through
vvdsp_amd.Resampler on device tensors -- linear bit-identical, sinc within the
harness rule (tests/conftest.py::tolerances) -- and, against the NumPy model of
tests/resample_util.py (held to the same fixtures in test_resample_host.py),
the shapes no fixture holds: batched strided rows, run boundaries of the table
kernel, the generic kernel, and positions past 2^24 input samples."""
import ctypes as C
import math

import numpy as np
import pytest

import resample_util as ru
from vvapi import OK, ERR_SIZE

pytestmark = pytest.mark.gpu

SENT = -777.0


@pytest.fixture(scope="module")
def misc():
    return ru.fixture_misc()


@pytest.fixture(scope="module")
def api(amd):
    return ru.ResamplerApi(amd.lib)


def dev(vdev, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


@pytest.mark.parametrize("num,den", ru.RATIOS)
def test_fixtures_host_pointers(api, misc, num, den):
    fx = ru.fixture(num, den)
    worst = 0.0
    for n in ru.LENGTHS:
        for taps in [None] + ru.TAPS:
            want = fx[ru.key(n, taps)]
            st, out_n, y = api.process(misc["x"][:n], num, den, taps)
            assert st == OK and out_n == len(want), (n, taps, st, out_n)
            if taps is None:
                assert y[:out_n].tobytes() == want.tobytes(), (n, "linear")
            else:
                worst = max(worst, ru.within_harness(y[:out_n], want))
            assert np.all(y[out_n:] == np.float32(-123.0))
    print(f"host API vs reference {num}/{den}: sinc max |diff| {worst:.3g}")


@pytest.mark.parametrize("num,den", ru.RATIOS)
def test_fixtures_device_tensors(vdev, misc, num, den):
    fx = ru.fixture(num, den)
    worst = 0.0
    for n in ru.LENGTHS:
        x = dev(vdev, misc["x"][:n])
        for taps in [None] + ru.TAPS:
            want = fx[ru.key(n, taps)]
            rs = vdev.Resampler(num, den, sinc=taps is not None, taps=taps or 32)
            assert rs.output_length(n) == len(want)
            y = rs(x).cpu().numpy()
            if taps is None:
                assert y.tobytes() == want.tobytes(), (n, "linear")
            else:
                worst = max(worst, ru.within_harness(y, want))
    print(f"Resampler vs reference {num}/{den}: sinc max |diff| {worst:.3g}")


def test_reduced_ratio_is_bit_identical(vdev, misc):
    x = dev(vdev, misc["x"])
    for sinc in (False, True):
        a = vdev.Resampler(2, 6, sinc=sinc)(x).cpu().numpy()
        b = vdev.Resampler(1, 3, sinc=sinc)(x).cpu().numpy()
        assert a.tobytes() == b.tobytes()


def test_centre_below_the_rational_one_80_147(vdev, misc):
    """At 80/147 the reference's f64 quotient falls below the integer k 147 / 80 at
    outputs 240, 400, 480, 720, ...; it then centres one sample lower, a different
    filter (an exact-rational centre is off by 1.7e-2 there)."""
    vdev.debug_clear("STAT_RESAMPLE_TABLE")
    y = vdev.Resampler(80, 147, sinc=True, taps=32)(dev(vdev, misc["x"])).cpu().numpy()
    assert vdev.debug_get("STAT_RESAMPLE_TABLE") == 1
    want = ru.fixture(80, 147)[ru.key(6000, 32)]
    at = np.array([240, 400, 480, 720])
    print("80/147 |diff| at 240, 400, 480, 720:", np.abs(y[at].astype(np.float64) - want[at]))
    ru.within_harness(y[at], want[at])
    ru.within_harness(y, want)


def test_generic_kernel(vdev, misc, knob):
    x = dev(vdev, misc["x"])
    for num, den in ((160, 441), (80, 147)):
        want = ru.fixture(num, den)[ru.key(6000, 32)]
        rs = vdev.Resampler(num, den, sinc=True, taps=32)
        vdev.debug_clear("STAT_RESAMPLE_TABLE")
        vdev.debug_clear("STAT_RESAMPLE_GENERIC")
        t = rs(x).cpu().numpy()
        assert (vdev.debug_get("STAT_RESAMPLE_TABLE"), vdev.debug_get("STAT_RESAMPLE_GENERIC")) == (1, 0)
        knob("RESAMPLE_GENERIC", 1)
        g = rs(x).cpu().numpy()
        knob("RESAMPLE_GENERIC", None)
        assert (vdev.debug_get("STAT_RESAMPLE_TABLE"), vdev.debug_get("STAT_RESAMPLE_GENERIC")) == (1, 1)
        print(f"{num}/{den}: table {ru.within_harness(t, want):.3g}, generic {ru.within_harness(g, want):.3g}, "
              f"table vs generic {np.max(np.abs(t - g)):.3g}")
    # a ratio whose table (44,101 rows) does not fit LDS: the generic kernel without the knob
    assert vdev.lib().vvhip_resample_run_length(44100, 48001, 32) == 0
    vdev.debug_clear("STAT_RESAMPLE_TABLE")
    vdev.debug_clear("STAT_RESAMPLE_GENERIC")
    g = vdev.Resampler(44100, 48001, sinc=True, taps=32)(x).cpu().numpy()
    assert (vdev.debug_get("STAT_RESAMPLE_TABLE"), vdev.debug_get("STAT_RESAMPLE_GENERIC")) == (0, 1)
    print(f"44100/48001 generic vs model: {ru.within_harness(g, ru.model_sinc(misc['x'], 44100, 48001, 32)):.3g}")


@pytest.mark.parametrize("taps", [None, 32, 6])
def test_batched_unaligned_rows(vdev, misc, taps):
    """nch = 3, input rows n + 3 floats apart, output rows out_n + 1 apart, the base
    pointers one float past an allocation's start: nothing 16-byte aligned.  Every row
    equals the single-row result bit for bit and the padding floats stay untouched."""
    import torch
    num, den, n, nch = 80, 147, 6000, 3
    rng = np.random.default_rng(7)
    rows = np.concatenate([misc["x"][None, :], rng.uniform(-1, 1, (nch - 1, n)).astype(np.float32)])
    rs = vdev.Resampler(num, den, sinc=taps is not None, taps=taps or 32)
    m = rs.output_length(n)
    singles = [rs(dev(vdev, r)).cpu().numpy() for r in rows]
    if taps == 32:
        ru.within_harness(singles[0], ru.fixture(num, den)[ru.key(n, 32)])
    xin = np.full(1 + nch * (n + 3), SENT, np.float32)
    for c in range(nch):
        xin[1 + c * (n + 3):1 + c * (n + 3) + n] = rows[c]
    d_in = dev(vdev, xin)
    d_out = torch.full((1 + nch * (m + 1) + 8,), SENT, dtype=torch.float32, device="cuda")
    got = C.c_size_t(0)
    st = vdev.lib().vv_dsp_resampler_process_device(rs.h, C.c_void_p(d_in.data_ptr() + 4), n, nch, n + 3,
                                                    C.c_void_p(d_out.data_ptr() + 4), m, m + 1,
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(got))
    assert st == OK and got.value == m
    out = d_out.cpu().numpy()
    assert out[0] == SENT and np.all(out[1 + nch * (m + 1) - 1:] == SENT)
    for c in range(nch):
        row = out[1 + c * (m + 1):1 + c * (m + 1) + m + 1]
        assert row[:m].tobytes() == singles[c].tobytes(), c
        assert row[m] == SENT, c


def _in_n_for(out_n, num, den):
    n = max(int(math.ceil((out_n - 1) * den / num)) - 2, 1)
    while ru.output_length(n, num, den) < out_n:
        n += 1
    assert ru.output_length(n, num, den) == out_n
    return n


@pytest.mark.parametrize("num,den", [(160, 441), (80, 147)])   # decimating: every output length occurs
def test_run_boundaries_and_capacity(vdev, num, den):
    """out_n one short of, equal to, and one past a workgroup's run, and two runs
    plus one; out_cap == out_n succeeds, out_cap == out_n - 1 is INVALID_SIZE and
    writes nothing."""
    import torch
    R = vdev.lib().vvhip_resample_run_length(num, den, 32)
    assert R >= 64
    rs = vdev.Resampler(num, den, sinc=True, taps=32)
    rng = np.random.default_rng(11)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for out_n in (R - 1, R, R + 1, 2 * R + 1):
        n = _in_n_for(out_n, num, den)
        x = rng.uniform(-1, 1, n).astype(np.float32)
        d_in = dev(vdev, x)
        d_out = torch.full((out_n + 4,), SENT, dtype=torch.float32, device="cuda")
        got = C.c_size_t(123)
        st = vdev.lib().vv_dsp_resampler_process_device(rs.h, C.c_void_p(d_in.data_ptr()), n, 1, n,
                                                        C.c_void_p(d_out.data_ptr()), out_n - 1, out_n, stream,
                                                        C.byref(got))
        assert st == ERR_SIZE and got.value == 123
        assert bool((d_out == SENT).all())
        st = vdev.lib().vv_dsp_resampler_process_device(rs.h, C.c_void_p(d_in.data_ptr()), n, 1, n,
                                                        C.c_void_p(d_out.data_ptr()), out_n, out_n, stream,
                                                        C.byref(got))
        assert st == OK and got.value == out_n
        y = d_out.cpu().numpy()
        assert np.all(y[out_n:] == SENT)
        ru.within_harness(y[:out_n], ru.model_sinc(x, num, den, 32))


def test_large_positions(vdev):
    """One channel of 20,000,000 samples at 160/147: the f32 position of the linear
    path coarsens past 2^24 input samples exactly as the reference's does (bit-identical
    to the model over the whole output); the sinc path keeps its f64 centre."""
    num, den, n = 160, 147, 20_000_000
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(np.float32)
    d = dev(vdev, x)
    y = vdev.Resampler(num, den)(d).cpu().numpy()
    want = ru.model_linear(x, num, den)
    assert y.shape == want.shape and y.tobytes() == want.tobytes()
    s = vdev.Resampler(num, den, sinc=True, taps=32)(d).cpu().numpy()
    out_n = len(s)
    k24 = int(math.ceil((2 ** 24) * num / den))
    for ks in (np.arange(out_n - 4096, out_n), np.arange(k24 - 2048, k24 + 2048)):
        print(f"sinc outputs {ks[0]}..{ks[-1]}: {ru.within_harness(s[ks], ru.model_sinc(x, num, den, 32, ks)):.3g}")


def test_changed_plan_rebuilds_table(vdev, misc):
    x = dev(vdev, misc["x"])
    rs = vdev.Resampler(160, 441, sinc=True, taps=32)
    first = rs(x).cpu().numpy()
    ru.within_harness(first, ru.fixture(160, 441)[ru.key(6000, 32)])
    rs.set_quality(True, 127)
    rs.set_ratio(80, 147)
    y = rs(x).cpu().numpy()
    fresh = vdev.Resampler(80, 147, sinc=True, taps=127)(x).cpu().numpy()
    assert y.tobytes() == fresh.tobytes()
    ru.within_harness(y, ru.fixture(80, 147)[ru.key(6000, 127)])
    rs.set_quality(False)
    rs.set_ratio(2, 6)
    assert rs(x).cpu().numpy().tobytes() == ru.fixture(1, 3)[ru.key(6000, None)].tobytes()
