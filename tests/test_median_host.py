"""CPU tests of the running median and HPSS front-ends (include/vv_dsp/filter/median.h,
include/vv_dsp/spectral/hpss.h): the two forms of the numpy model (tests/median_util.py)
agree bit for bit on every case the GPU tests run, every argument check returns its
status in the headers' order through the C ABI before any device work, a valid call with
no GPU returns UNSUPPORTED instead of computing on the CPU, and the model separates the
tone-and-clicks fixture."""
import ctypes as C

import numpy as np
import pytest

import median_util as mu
from median_util import OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_UNSUPPORTED

NAN, INF = float("nan"), float("inf")


class HpssParams(C.Structure):
    _fields_ = [("n_fft", C.c_size_t), ("magnitude", C.c_int), ("win_harm", C.c_int), ("win_perc", C.c_int),
                ("margin_harm", C.c_float), ("margin_perc", C.c_float), ("mask", C.c_int)]


class HpssOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("harm", "perc", "mask_harm", "mask_perc")]


@pytest.fixture(scope="module")
def L(amd_lib_path):
    lib = C.CDLL(amd_lib_path)
    sz, vp = C.c_size_t, C.c_void_p
    lib.vv_dsp_medfilt.argtypes = [vp, sz, C.c_int, C.c_int, vp]
    lib.vv_dsp_medfilt_device.argtypes = [vp, sz, sz, sz, C.c_int, C.c_int, vp, sz, vp]
    lib.vv_dsp_hpss.argtypes = [vp, sz, C.POINTER(HpssParams), C.POINTER(HpssOut)]
    lib.vv_dsp_hpss_device.argtypes = [vp, sz, sz, sz, C.POINTER(HpssParams), C.POINTER(HpssOut), sz, vp]
    lib.vv_dsp_stft_hpss_device.argtypes = [vp, C.POINTER(HpssParams), vp, sz, sz, sz, vp, vp, sz, vp, C.POINTER(sz)]
    lib.vvhip_available.restype = C.c_int
    return lib


def test_symbols_exported(L):
    for name in ("vv_dsp_medfilt", "vv_dsp_medfilt_device", "vv_dsp_hpss", "vv_dsp_hpss_device",
                 "vv_dsp_stft_hpss_device"):
        assert hasattr(L, name), name


def test_key_order_and_round_trip():
    x = np.array([-INF, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, INF, NAN], np.float32)
    k = mu.keys(x)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(mu.bits(mu.unkey(k)), mu.bits(mu.canon(x)))
    assert np.all(mu.keys(mu.SPECIALS[-5:]) == mu.keys(np.float32(NAN)))      # every NaN is the one NaN


def test_fold():
    assert mu.fold(np.arange(-7, 9), 3, mu.REFLECT).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert mu.fold(np.arange(-3, 5), 1, mu.REFLECT).tolist() == [0] * 8
    assert mu.fold(np.arange(-2, 5), 3, mu.NEAREST).tolist() == [0, 0, 0, 1, 2, 2, 2]
    assert mu.fold(np.arange(-2, 5), 3, mu.ZERO).tolist() == [-1, -1, 0, 1, 2, -1, -1]


@pytest.mark.parametrize("n", mu.MEDFILT_N)
def test_model_forms_agree_medfilt(n):
    x = mu.medfilt_rows(n, n)
    for Lw in mu.MEDFILT_L:
        for mode in (mu.REFLECT, mu.NEAREST, mu.ZERO):
            a, b = mu.median_sort(x, Lw, mode), mu.median_count(x, Lw, mode)
            assert np.array_equal(mu.bits(a), mu.bits(b)), (n, Lw, mode)
            if Lw == 1:
                assert np.array_equal(mu.bits(a), mu.bits(mu.canon(x)))


def test_model_known_values():
    x = np.array([5, 1, 4, 2, 3], np.float32)
    assert mu.median_sort(x, 3, mu.REFLECT).tolist() == [1, 4, 2, 3, 2]
    assert mu.median_sort(x, 3, mu.NEAREST).tolist() == [5, 4, 2, 3, 3]
    assert mu.median_sort(x, 3, mu.ZERO).tolist() == [1, 4, 2, 3, 2]
    z = np.array([-0.0, 0.0, -0.0], np.float32)
    assert mu.bits(mu.median_sort(z, 3, mu.NEAREST)).tolist() == [0x80000000, 0x80000000, 0x80000000]
    assert mu.bits(mu.median_sort(z, 3, mu.ZERO)).tolist() == [0, 0x80000000, 0]
    q = np.array([1.0, NAN, NAN], np.float32)
    assert mu.bits(mu.median_sort(-q, 3, mu.NEAREST)).tolist() == [0xBF800000, 0x7FC00000, 0x7FC00000]


@pytest.mark.parametrize("shape", mu.HPSS_SHAPES)
def test_model_forms_agree_hpss(shape):
    n_fft, T = shape
    p = mu.hpss_rows(n_fft, T, T)
    wins = mu.HPSS_WINDOWS + (((127, 127),) if T == 7 else ())
    for wh, wp in wins:
        for rpg in (0, max(1, (T + 2) // 3 + (T > 3))):
            a = mu.hpss_model(p, n_fft, 1, wh, wp, 1.5, 2.0, mu.SOFT, rpg, mu.median_sort)
            b = mu.hpss_model(p, n_fft, 1, wh, wp, 1.5, 2.0, mu.SOFT, rpg, mu.median_count)
            for name in a:
                assert np.array_equal(mu.bits(a[name]), mu.bits(b[name])), (shape, wh, wp, rpg, name)


def test_mask_rules():
    a = np.array([0.0, 1.0, 3.0, NAN, INF, 2.0], np.float32)
    b = np.array([0.0, 1.0, 1.0, 1.0, INF, NAN], np.float32)
    assert mu.mask_of(a, b, 1.0, mu.HARD).tolist() == [0, 0, 1, 0, 0, 0]
    s = mu.mask_of(a, b, 1.0, mu.SOFT)
    assert s[:3].tolist() == [0.5, 0.5, 0.75] and mu.bits(s[3:]).tolist() == [0x7FC00000] * 3
    w = mu.mask_of(a, b, 2.0, mu.WIENER)
    assert w[:3].tolist() == [0.5, np.float32(1 / 5), np.float32(9 / 13)]


def test_medfilt_argument_rules_in_order(L):
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    host, dev = L.vv_dsp_medfilt, L.vv_dsp_medfilt_device
    # 1. NULL pointers, whatever else is wrong
    assert host(None, 0, 2, 9, p) == ERR_NULL and host(p, 0, 2, 9, None) == ERR_NULL
    assert dev(None, 0, 2, 0, 2, 9, p, 0, None) == ERR_NULL and dev(p, 0, 2, 0, 2, 9, None, 0, None) == ERR_NULL
    # 2. n == 0 or a short stride, before the window and the mode
    assert host(p, 0, 2, 9, p) == ERR_SIZE
    assert dev(p, 0, 1, 0, 2, 9, p, 0, None) == ERR_SIZE
    for xs, ys in ((15, 16), (16, 15), (0, 0)):
        assert dev(p, 16, 2, xs, 2, 9, p, ys, None) == ERR_SIZE
        assert dev(p, 16, 2, xs, 129, 0, p, ys, None) == ERR_SIZE
    # 3. the window and the mode, before the limit
    for Lw, mode in ((0, 0), (-3, 0), (4, 0), (128, 0), (3, 3), (3, -1), (129, 7)):
        assert host(p, 16, Lw, mode, p) == ERR_RANGE, (Lw, mode)
        assert dev(p, 16, 2, 16, Lw, mode, p, 16, None) == ERR_RANGE, (Lw, mode)
        assert dev(p, 16, 1, 0, Lw, mode, p, 0, None) == ERR_RANGE, (Lw, mode)     # one row: strides not looked at
    # 4. the limit
    assert host(p, 16, 129, 0, p) == ERR_UNSUPPORTED
    assert dev(p, 16, 2, 16, 129, 2, p, 16, None) == ERR_UNSUPPORTED
    assert dev(p, 16, 2 ** 31, 16, 3, 0, p, 16, None) == ERR_UNSUPPORTED
    # batch == 0: OK, nothing written, no device asked for
    assert dev(p, 16, 0, 0, 3, 0, p, 0, None) == OK
    assert np.all(buf == 0)


def _prm(n_fft=64, magnitude=1, wh=9, wp=9, mh=1.0, mp=1.0, mask=mu.SOFT):
    return HpssParams(n_fft, magnitude, wh, wp, mh, mp, mask)


BAD_HPSS = {"even_harm": dict(wh=8), "zero_perc": dict(wp=0), "negative_harm": dict(wh=-1), "mask_3": dict(mask=3),
            "mask_negative": dict(mask=-1), "margin_below_1": dict(mh=0.5), "margin_nan": dict(mp=NAN),
            "margin_inf": dict(mh=INF)}


def test_hpss_argument_rules_in_order(L):
    buf = np.zeros(33 * 4, np.float32)
    p = buf.ctypes.data
    out = HpssOut(p, p, p, p)
    host, dev = L.vv_dsp_hpss, L.vv_dsp_hpss_device
    good, bad = _prm(), _prm(n_fft=1, wh=8)
    # 1. NULL params, rows or out
    assert host(None, 4, C.byref(bad), C.byref(out)) == ERR_NULL
    assert host(p, 4, None, C.byref(out)) == ERR_NULL and host(p, 4, C.byref(bad), None) == ERR_NULL
    assert dev(None, 4, 0, 0, C.byref(bad), C.byref(out), 0, None) == ERR_NULL
    assert dev(p, 4, 0, 0, None, C.byref(out), 0, None) == ERR_NULL
    assert dev(p, 4, 0, 0, C.byref(bad), None, 0, None) == ERR_NULL
    # 2. n_fft < 2 or a pitch below K, before the windows
    assert host(p, 4, C.byref(bad), C.byref(out)) == ERR_SIZE
    assert dev(p, 4, 33, 0, C.byref(bad), C.byref(out), 33, None) == ERR_SIZE
    for rp, op in ((32, 33), (33, 32)):
        assert dev(p, 4, rp, 0, C.byref(_prm(wh=8)), C.byref(out), op, None) == ERR_SIZE
    # 3. windows, mask and margins, before the limits
    for name, kw in BAD_HPSS.items():
        for extra in ({}, {"n_fft": 2 * 8193}):
            prm = _prm(**{**kw, **extra})
            K = prm.n_fft // 2 + 1
            assert host(p, 4, C.byref(prm), C.byref(out)) == ERR_RANGE, name
            assert dev(p, 4, K, 0, C.byref(prm), C.byref(out), K, None) == ERR_RANGE, name
    assert dev(p, 4, 33, 0, C.byref(_prm(wh=129, wp=4)), C.byref(out), 33, None) == ERR_RANGE
    # 4. the limits
    for prm in (_prm(wh=129), _prm(wp=129), _prm(n_fft=2 * 8193)):
        K = prm.n_fft // 2 + 1
        assert host(p, 4, C.byref(prm), C.byref(out)) == ERR_UNSUPPORTED
        assert dev(p, 4, K, 0, C.byref(prm), C.byref(out), K, None) == ERR_UNSUPPORTED
    assert dev(p, 2 ** 31, 33, 0, C.byref(good), C.byref(out), 33, None) == ERR_UNSUPPORTED
    assert dev(p, 2 ** 32, 33, 2 ** 31, C.byref(good), C.byref(out), 33, None) == ERR_UNSUPPORTED
    # zero rows or nothing wanted: OK, nothing launched, no device asked for
    none = HpssOut()
    assert dev(p, 0, 33, 0, C.byref(good), C.byref(out), 33, None) == OK
    assert dev(p, 4, 33, 0, C.byref(good), C.byref(none), 33, None) == OK
    assert host(p, 0, C.byref(good), C.byref(out)) == OK and host(p, 4, C.byref(good), C.byref(none)) == OK
    # the signal form: a NULL handle, params or signal, or both outputs NULL
    ln = C.c_size_t(77)
    sh = L.vv_dsp_stft_hpss_device
    assert sh(None, C.byref(good), p, 64, 1, 64, p, p, 64, None, C.byref(ln)) == ERR_NULL
    assert sh(p, None, p, 64, 1, 64, p, p, 64, None, C.byref(ln)) == ERR_NULL
    assert sh(p, C.byref(good), None, 64, 1, 64, p, p, 64, None, C.byref(ln)) == ERR_NULL
    assert sh(p, C.byref(good), p, 64, 1, 64, None, None, 64, None, C.byref(ln)) == ERR_NULL
    assert ln.value == 77
    assert np.all(buf == 0)


def test_no_gpu_fails_loudly(L):
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is present")
    x = np.arange(16, dtype=np.float32)
    y = np.full(16, -7, np.float32)
    assert L.vv_dsp_medfilt(x.ctypes.data, 16, 3, 0, y.ctypes.data) == ERR_UNSUPPORTED
    assert L.vv_dsp_medfilt_device(x.ctypes.data, 16, 1, 16, 3, 0, y.ctypes.data, 16, None) == ERR_UNSUPPORTED
    p = np.ones((4, 33), np.float32)
    o = np.full((4, 33), -7, np.float32)
    out = HpssOut(o.ctypes.data, None, None, None)
    assert L.vv_dsp_hpss(p.ctypes.data, 4, C.byref(_prm()), C.byref(out)) == ERR_UNSUPPORTED
    assert L.vv_dsp_hpss_device(p.ctypes.data, 4, 33, 0, C.byref(_prm()), C.byref(out), 33, None) == ERR_UNSUPPORTED
    assert np.all(y == -7) and np.all(o == -7)


def test_knobs_registered():
    import vvdsp_amd as vv
    for name, value in (("MEDIAN_SELECT", 2), ("HPSS_GROUP", 3)):
        vv.debug_set(name, value)
        assert vv.debug_get(name) == value and vv.debug_get("VVHIP_" + name) == value
        vv.debug_clear(name)
        assert vv.debug_get(name) == -1


def test_model_separates_tone_and_clicks():
    """the definition itself, on a float64 STFT of the fixture: the conditions the GPU test
    sets for the library's masks hold for the model with room"""
    tone, clicks, noise = mu.separation_signals()
    mix = (tone + clicks + noise).astype(np.float32)
    power = (np.abs(mu.stft64(mix)) ** 2).astype(np.float32)
    m = mu.hpss_model(power, 256, 1, 9, 9, 1.0, 1.0, mu.WIENER)
    st, sc = mu.stft64(tone), mu.stft64(clicks)
    got = (mu.kept(m["mask_harm"], st), mu.kept(m["mask_harm"], sc), mu.kept(m["mask_perc"], sc),
           mu.kept(m["mask_perc"], st))
    print("kept: harm/tone %.4f harm/clicks %.4f perc/clicks %.4f perc/tone %.4f" % got)
    assert got[0] >= 0.99 and got[1] <= 0.05 and got[2] >= 0.95 and got[3] <= 0.01
