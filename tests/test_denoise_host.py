"""CPU tests of spectral noise suppression (include/vv_dsp/spectral/denoise.h): the two
forms of the numpy model (tests/denoise_util.py) agree bit for bit on every case the GPU
tests run, every argument check returns its status in the header's order through the C ABI
before any device work, the defaults, a valid call with no GPU returns UNSUPPORTED instead
of computing on the CPU, and the model does on the noisy-bursts fixture what it is for.

The fixture, measured with the model alone on a float64 STFT (n_fft 256, hop 64, the
library's symmetric Hann; smooth_len 8, back = ahead = 48, bias 4, floor 0.1): the
STFT-domain SNR against the clean rows goes from 14.64 dB to 21.08 dB (WIENER), 19.22 dB
(SUBTRACT) and 16.36 dB (GATE); on the noise part alone the floor over the true per-bin noise
power has median 0.294 (5th to 95th percentile 0.143 to 0.469), which is why the default
bias is near 1 / 0.29.  The limits asserted are +4 dB, +3 dB, above 0 dB and [0.2, 0.45]."""
import ctypes as C

import numpy as np
import pytest

import denoise_util as du
from denoise_util import OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_UNSUPPORTED, bits

NAN, INF = float("nan"), float("inf")


class DenoiseParams(C.Structure):
    _fields_ = [("n_fft", C.c_size_t), ("smooth_len", C.c_int), ("back", C.c_int), ("ahead", C.c_int),
                ("bias", C.c_float), ("floor", C.c_float), ("mode", C.c_int)]


class DenoiseOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("smooth", "noise", "gain")]


@pytest.fixture(scope="module")
def L(amd_lib_path):
    lib = C.CDLL(amd_lib_path)
    sz, vp = C.c_size_t, C.c_void_p
    lib.vv_dsp_denoise_params_default.argtypes = [sz, C.POINTER(DenoiseParams)]
    lib.vv_dsp_denoise.argtypes = [vp, sz, C.POINTER(DenoiseParams), C.POINTER(DenoiseOut)]
    lib.vv_dsp_denoise_device.argtypes = [vp, sz, sz, sz, C.POINTER(DenoiseParams), C.POINTER(DenoiseOut), sz, vp]
    lib.vv_dsp_stft_denoise_device.argtypes = [vp, C.POINTER(DenoiseParams), vp, sz, sz, sz, vp, sz, vp, C.POINTER(sz)]
    lib.vvhip_available.restype = C.c_int
    return lib


def test_symbols_exported(L):
    for name in ("vv_dsp_denoise_params_default", "vv_dsp_denoise", "vv_dsp_denoise_device",
                 "vv_dsp_stft_denoise_device"):
        assert hasattr(L, name), name


@pytest.mark.parametrize("c", du.ALL_CASES, ids=du.case_id)
def test_model_forms_agree(c):
    p = du.case_rows(c)
    a, b = du.denoise_model(p, *du.model_args(c)), du.denoise_naive(p, *du.model_args(c))
    for name in du.NAMES:
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    assert np.all(a["gain"] >= np.float32(c["floor"])) and np.all(a["gain"] <= 1)


@pytest.mark.parametrize("mode", (du.GATE, du.WIENER, du.SUBTRACT))
def test_model_forms_agree_on_hostile_powers(mode):
    p = du.hostile_rows(128, 40, 7)
    for floor in (0.0, 0.1):
        for rpg in (0, 15):
            a = du.denoise_model(p, 128, 8, 5, 3, 4.0, floor, mode, rpg)
            b = du.denoise_naive(p, 128, 8, 5, 3, 4.0, floor, mode, rpg)
            for name in du.NAMES:
                assert np.array_equal(bits(a[name]), bits(b[name])), (floor, rpg, name)
            g = a["gain"]
            assert not np.isnan(g).any() and g.min() >= np.float32(floor) and g.max() <= 1
            # a column of NaNs: the floor is the NaN, the gain the floor (GATE, WIENER) or its clamp
            assert np.all(bits(a["noise"][:, 65 // 3]) == 0x7FC00000)


def test_model_known_values():
    p = np.array([[4.0], [2.0], [6.0], [0.0], [8.0]], np.float32)
    p = np.concatenate([p, p], axis=1)                       # K = 2 (n_fft = 2)
    m = du.denoise_model(p, 2, 2, 1, 0, 0.5, 0.25, du.WIENER)
    assert m["smooth"][:, 0].tolist() == [4, 3, 4, 3, 4]     # row -1 is row 0
    assert m["noise"][:, 0].tolist() == [2, 1.5, 1.5, 1.5, 1.5]
    assert m["gain"][:, 0].tolist() == [0.5, 0.25, 0.75, 0.25, np.float32(6.5 / 8)]   # a = 0: q = -inf, the floor
    g = du.denoise_model(p, 2, 2, 1, 0, 0.5, 0.25, du.GATE)["gain"][:, 1]
    assert g.tolist() == [1, 1, 1, 0.25, 1]
    s = du.denoise_model(p, 2, 2, 1, 0, 0.5, 0.25, du.SUBTRACT)["gain"][:, 0]
    assert s.tolist() == [np.float32(np.sqrt(0.5)), 0.5, np.float32(np.sqrt(0.75)), 0.25, np.float32(np.sqrt(6.5 / 8))]
    # the order of the minimum: -0 below +0, a NaN above everything
    z = np.array([[0.0, NAN], [-0.0, 1.0], [0.0, NAN]], np.float32)
    f = du.floor_plane(z, 1, 1)
    assert bits(f[:, 0]).tolist() == [0x80000000] * 3 and f[:, 1].tolist() == [1, 1, 1]


def _prm(n_fft=64, W=8, back=5, ahead=3, bias=4.0, floor=0.1, mode=du.WIENER):
    return DenoiseParams(n_fft, W, back, ahead, bias, floor, mode)


BAD = {"smooth_0": dict(W=0), "smooth_negative": dict(W=-2), "back_negative": dict(back=-1),
       "ahead_negative": dict(ahead=-1), "mode_3": dict(mode=3), "mode_negative": dict(mode=-1),
       "bias_0": dict(bias=0.0), "bias_negative": dict(bias=-1.0), "bias_nan": dict(bias=NAN),
       "bias_inf": dict(bias=INF), "floor_negative": dict(floor=-0.5), "floor_above_1": dict(floor=1.5),
       "floor_nan": dict(floor=NAN)}
OVER = {"smooth_65": dict(W=65), "back_512": dict(back=512), "ahead_512": dict(ahead=512),
        "bins": dict(n_fft=2 * 8193)}


def test_argument_rules_in_order(L):
    buf = np.zeros(33 * 4, np.float32)
    p = buf.ctypes.data
    out = DenoiseOut(p, p, p)
    host, dev = L.vv_dsp_denoise, L.vv_dsp_denoise_device
    good, bad = _prm(), _prm(n_fft=1, W=0)
    # 1. NULL params, rows or out
    assert host(None, 4, C.byref(bad), C.byref(out)) == ERR_NULL
    assert host(p, 4, None, C.byref(out)) == ERR_NULL and host(p, 4, C.byref(bad), None) == ERR_NULL
    assert dev(None, 4, 0, 0, C.byref(bad), C.byref(out), 0, None) == ERR_NULL
    assert dev(p, 4, 0, 0, None, C.byref(out), 0, None) == ERR_NULL
    assert dev(p, 4, 0, 0, C.byref(bad), None, 0, None) == ERR_NULL
    # 2. n_fft < 2 or a pitch below K, before the parameters
    assert host(p, 4, C.byref(bad), C.byref(out)) == ERR_SIZE
    assert dev(p, 4, 33, 0, C.byref(bad), C.byref(out), 33, None) == ERR_SIZE
    for rp, op in ((32, 33), (33, 32)):
        assert dev(p, 4, rp, 0, C.byref(_prm(W=0)), C.byref(out), op, None) == ERR_SIZE
    # 3. the lengths, the mode, the bias and the floor, before the limits
    for name, kw in BAD.items():
        for extra in ({}, {"n_fft": 2 * 8193}, {"back": 512} if "back" not in kw else {"W": 65} if "W" not in kw else {}):
            prm = _prm(**{**kw, **extra})
            K = prm.n_fft // 2 + 1
            assert host(p, 4, C.byref(prm), C.byref(out)) == ERR_RANGE, name
            assert dev(p, 4, K, 0, C.byref(prm), C.byref(out), K, None) == ERR_RANGE, name
    # 4. the limits
    for name, kw in OVER.items():
        prm = _prm(**kw)
        K = prm.n_fft // 2 + 1
        assert host(p, 4, C.byref(prm), C.byref(out)) == ERR_UNSUPPORTED, name
        assert dev(p, 4, K, 0, C.byref(prm), C.byref(out), K, None) == ERR_UNSUPPORTED, name
    assert dev(p, 2 ** 30, 33, 0, C.byref(good), C.byref(out), 33, None) == ERR_UNSUPPORTED
    assert dev(p, 2 ** 32, 33, 2 ** 31, C.byref(good), C.byref(out), 33, None) == ERR_UNSUPPORTED
    # the largest parameters are taken: zero rows or nothing wanted is OK, nothing launched, no device asked for
    most = _prm(W=64, back=511, ahead=511, floor=1.0)
    none = DenoiseOut()
    assert dev(p, 0, 33, 0, C.byref(most), C.byref(out), 33, None) == OK
    assert dev(p, 4, 33, 0, C.byref(good), C.byref(none), 33, None) == OK
    assert host(p, 0, C.byref(good), C.byref(out)) == OK and host(p, 4, C.byref(most), C.byref(none)) == OK
    # the signal form: a NULL handle, params, signal or output
    ln = C.c_size_t(77)
    sd = L.vv_dsp_stft_denoise_device
    assert sd(None, C.byref(good), p, 64, 1, 64, p, 64, None, C.byref(ln)) == ERR_NULL
    assert sd(p, None, p, 64, 1, 64, p, 64, None, C.byref(ln)) == ERR_NULL
    assert sd(p, C.byref(good), None, 64, 1, 64, p, 64, None, C.byref(ln)) == ERR_NULL
    assert sd(p, C.byref(good), p, 64, 1, 64, None, 64, None, C.byref(ln)) == ERR_NULL
    assert ln.value == 77
    assert np.all(buf == 0)


def test_defaults(L):
    prm = DenoiseParams()
    assert L.vv_dsp_denoise_params_default(1024, None) == ERR_NULL
    assert L.vv_dsp_denoise_params_default(1024, C.byref(prm)) == OK
    assert (prm.n_fft, prm.smooth_len, prm.back, prm.ahead, prm.mode) == (1024, 8, 48, 48, du.WIENER)
    assert prm.bias == 4.0 and prm.floor == np.float32(0.1)
    import vvdsp_amd as vv
    q = vv.denoise_params(512, mode=vv.DENOISE_GATE, ahead=0)
    assert (q.n_fft, q.smooth_len, q.back, q.ahead, q.mode) == (512, 8, 48, 0, du.GATE)
    assert vv.DENOISE_NAMES == du.NAMES
    assert (vv.DENOISE_GATE, vv.DENOISE_WIENER, vv.DENOISE_SUBTRACT) == (du.GATE, du.WIENER, du.SUBTRACT)
    with pytest.raises(vv.VvError):
        vv.denoise_params(512, window=3)


def test_no_gpu_fails_loudly(L):
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is present")
    p = np.ones((4, 33), np.float32)
    o = np.full((4, 33), -7, np.float32)
    out = DenoiseOut(None, None, o.ctypes.data)
    assert L.vv_dsp_denoise(p.ctypes.data, 4, C.byref(_prm()), C.byref(out)) == ERR_UNSUPPORTED
    assert L.vv_dsp_denoise_device(p.ctypes.data, 4, 33, 0, C.byref(_prm()), C.byref(out), 33, None) == ERR_UNSUPPORTED
    assert np.all(o == -7)


def test_knobs_and_counter_registered():
    import vvdsp_amd as vv
    for name, value in (("DENOISE_SEGMENT", 8), ("DENOISE_MIN", 2), ("DENOISE_GROUP", 3)):
        vv.debug_set(name, value)
        assert vv.debug_get(name) == value and vv.debug_get("VVHIP_" + name) == value
        vv.debug_clear(name)
        assert vv.debug_get(name) == -1
    assert vv.debug_get("STAT_DENOISE") >= 0


def test_fixture_is_what_the_generator_writes():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "make_golden_denoise", os.path.join(os.path.dirname(du.GOLDEN), "make_golden_denoise.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    clean, noise = du.fixture_signal()
    assert clean.shape == noise.shape == (36000,) and clean.dtype == noise.dtype == np.float32
    want_clean, want_noise = gen.make()
    assert np.array_equal(noise, want_noise) and np.allclose(clean, want_clean, atol=1e-6)
    assert np.all(clean[:4000] == 0) and np.all(clean[32000:] == 0) and np.abs(clean[4000:8000]).max() > 0.5
    assert abs(float(noise.std()) - 0.05) < 0.001


def test_model_suppresses_the_fixture_noise():
    """the definition itself, on a float64 STFT of the fixture: the conditions the issue sets
    hold for the model with room (the measured values are in this module's docstring)"""
    clean, noise = du.fixture_signal()
    X, Cl, Nn = (du.stft64(v) for v in ((clean + noise).astype(np.float32), clean, noise))
    power = (np.abs(X) ** 2).astype(np.float32)
    before = du.snr_db(Cl, X)
    after = {}
    for mode in (du.WIENER, du.SUBTRACT, du.GATE):
        g = du.denoise_model(power, du.N_FFT, 8, 48, 48, 4.0, 0.1, mode)["gain"]
        after[mode] = du.snr_db(Cl, X * g)
    pn = np.abs(Nn) ** 2
    floor = du.denoise_model(pn.astype(np.float32), du.N_FFT, 8, 48, 48, 1.0, 0.1, du.WIENER)["noise"]
    ratio = floor / pn.mean(axis=0)
    med, lo, hi = np.median(ratio), *np.percentile(ratio, [5, 95])
    print("snr %.2f dB -> wiener %.2f subtract %.2f gate %.2f; floor / noise power: median %.3f (%.3f .. %.3f)"
          % (before, after[du.WIENER], after[du.SUBTRACT], after[du.GATE], med, lo, hi))
    assert after[du.WIENER] >= before + 4.0
    assert after[du.SUBTRACT] >= before + 3.0
    assert after[du.GATE] > before
    assert 0.2 <= med <= 0.45
