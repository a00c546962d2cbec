"""The resampler without a GPU: argument checks and output lengths against the
recorded reference (tests/golden/resample_*.npz, written by
tests/golden/make_golden_resample.py), the host-built polyphase table, and the
NumPy model of tests/resample_util.py against every fixture -- the GPU tests
use that model at sizes no fixture could hold, so it is held to the fixtures
here: sinc within the harness rule, linear bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import resample_util as ru
from vvapi import OK, ERR_UNSUPPORTED

_fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def api(amd_lib_path):
    a = ru.ResamplerApi(amd_lib_path)
    L = a.lib
    L.vv_dsp_resampler_output_length.argtypes = [C.c_void_p, C.c_size_t]
    L.vv_dsp_resampler_output_length.restype = C.c_size_t
    L.vvhip_resample_table_host.argtypes = [C.c_uint, C.c_uint, C.c_uint, _fp, C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_uint)]
    L.vvhip_last_error.restype = C.c_char_p
    return a


@pytest.fixture(scope="module")
def misc():
    return ru.fixture_misc()


def host_table(L, num, den, taps):
    phases, te = C.c_size_t(), C.c_uint()
    assert L.vvhip_resample_table_host(num, den, taps, None, C.byref(phases), C.byref(te)) == OK
    out = np.zeros((phases.value, te.value), np.float32)
    assert L.vvhip_resample_table_host(num, den, taps, out.ctypes.data_as(_fp), C.byref(phases), C.byref(te)) == OK
    return out


def test_argument_statuses_match_reference(api, misc):
    """resampler.c:16-76: NULL for a zero ratio, OUT_OF_RANGE, the order null
    pointers / in_n == 0 / capacity, and whether *out_n was written."""
    got = api.argument_cases()
    names = [str(s) for s in misc["arg_names"]]
    assert sorted(got) == names
    for name, st, out_n in zip(names, misc["arg_status"], misc["arg_out_n"]):
        assert got[name] == (st, out_n), (name, got[name], st, out_n)


def test_output_length_matches_reference(api, misc):
    L = api.lib
    assert L.vv_dsp_resampler_output_length(None, 10) == 0
    for (in_n, num, den), want in zip(misc["len_cases"], misc["len_out"]):
        rs = L.vv_dsp_resampler_create(int(num), int(den))
        try:
            assert L.vv_dsp_resampler_output_length(rs, int(in_n)) == want == ru.output_length(int(in_n), int(num),
                                                                                               int(den))
            assert L.vv_dsp_resampler_output_length(rs, 0) == 0
        finally:
            L.vv_dsp_resampler_destroy(rs)
    # every fixture's length, too
    for num, den in ru.RATIOS:
        fx = ru.fixture(num, den)
        for n in ru.LENGTHS:
            assert len(fx[ru.key(n, None)]) == len(fx[ru.key(n, 32)]) == ru.output_length(n, num, den)


@pytest.mark.parametrize("num,den", [(160, 441), (80, 147), (1, 3)])
def test_table_host(api, num, den):
    """(P + 1) rows of the effective taps, every row sums to 1, within 1e-7 of the f64 model."""
    for taps in ru.TAPS:
        W = host_table(api.lib, num, den, taps)
        P = num // math.gcd(num, den)
        assert W.shape == (P + 1, ru.effective_taps(taps))
        assert np.max(np.abs(W.astype(np.float64).sum(axis=1) - 1.0)) <= 1e-6
        W32, W64 = ru.model_table(num, den, taps)
        assert np.max(np.abs(W.astype(np.float64) - W64)) <= 1e-7
        assert np.max(np.abs(W - W32)) <= 1e-7
    # the reduced ratio gives the same table
    assert np.array_equal(host_table(api.lib, 2, 6, 32), host_table(api.lib, 1, 3, 32))
    assert api.lib.vvhip_resample_table_host(0, 3, 32, None, C.byref(C.c_size_t()), C.byref(C.c_uint())) != OK
    assert api.lib.vvhip_resample_table_host(1, 3, 32, None, None, None) != OK


@pytest.mark.parametrize("num,den", ru.RATIOS)
def test_model_reproduces_fixtures(misc, num, den):
    x = misc["x"]
    fx = ru.fixture(num, den)
    worst = 0.0
    for n in ru.LENGTHS:
        lin = ru.model_linear(x[:n], num, den)
        assert lin.tobytes() == fx[ru.key(n, None)].tobytes(), (num, den, n)
        for taps in ru.TAPS:
            worst = max(worst, ru.within_harness(ru.model_sinc(x[:n], num, den, taps), fx[ru.key(n, taps)]))
    print(f"model vs reference {num}/{den}: max |diff| {worst:.3g}")
    # clamping and the odd-to-even step, as recorded
    assert np.array_equal(fx[ru.key(6000, 1)], fx[ru.key(6000, 4)])
    assert np.array_equal(fx[ru.key(6000, 200)], fx[ru.key(6000, 128)])
    assert np.array_equal(fx[ru.key(6000, 127)], fx[ru.key(6000, 128)])


def test_model_centre_falls_below_the_rational_one():
    """At 80/147 floor((double)k / ratio) is one below (k 147) // 80 at outputs 240,
    400, 480, 720, ...: 24 of the first 3265; there the model takes table row P."""
    ks = np.arange(3265, dtype=np.int64)
    centre, row = ru.model_centres(80, 147, ks)
    exact = (ks * 147) // 80
    low = np.flatnonzero(centre != exact)
    assert list(low[:4]) == [240, 400, 480, 720] and len(low) == 24
    assert np.array_equal(centre[low], exact[low] - 1)
    assert np.all(row[low] == 80) and np.all((ks[low] * 147) % 80 == 0)
    others = np.setdiff1d(ks, low)
    assert np.array_equal(row[others], (others * 147) % 80)
    # 160/147: 944 of the first 217,686 outputs
    ks = np.arange(217686, dtype=np.int64)
    centre, _ = ru.model_centres(160, 147, ks)
    assert int(np.sum(centre != (ks * 147) // 160)) == 944


def test_no_gpu_fails_loudly(api, misc):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    for taps in (None, 32):
        st, out_n, _ = api.process(misc["x"][:100], 160, 441, taps)
        assert st == ERR_UNSUPPORTED
        assert b"no HIP device" in L.vvhip_last_error()
