"""CPU tests of the spectral shape front-end (include/vv_dsp/features/spectral_shape.h):
the exported symbols, the argument checks in the header's order with outputs
untouched, the device forms' checks before any device work, -- with no GPU --
UNSUPPORTED instead of a CPU computation, the knob and the counter, the binding's
checks, and the f64 model of the definition (tests/shape_util.py) on known answers,
against plain numpy one-liners and on the case table, where it must leave no row
undecidable."""
import ctypes as C

import numpy as np
import pytest

import shape_util as su
from shape_util import (ShapeApi, Params, params, CASES, CASE_IDS, OK, ERR_NULL, ERR_SIZE, ERR_RANGE,
                        ERR_UNSUPPORTED, untouched)


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return ShapeApi(amd_lib_path)


def bad_params(n_fft=1024):
    """name -> parameters that are OUT_OF_RANGE by rule 4 (the band is good)"""
    inf, nan = float("inf"), float("nan")
    res = {}
    for field in ("sample_rate", "floor"):
        for name, v in (("zero", 0.0), ("negative", -1.0), ("inf", inf), ("nan", nan)):
            p = params(n_fft)
            setattr(p, field, v)
            res[f"{field}_{name}"] = p
    for name, v in (("zero", 0.0), ("negative", -0.5), ("above_one", 1.0001), ("nan", nan), ("inf", inf)):
        p = params(n_fft)
        p.rolloff = v
        res[f"rolloff_{name}"] = p
    return res


def bad_bands(n_fft=1024):
    return {"min_above_max": params(n_fft, band=(5, 4)), "max_past_row": params(n_fft, band=(0, n_fft // 2 + 1)),
            "both": params(n_fft, band=(n_fft, n_fft // 2 + 1))}


def test_symbols_exported(amd_lib_path):
    lib = C.CDLL(amd_lib_path)
    for name in ("vv_dsp_spectral_shape", "vv_dsp_spectral_shape_device", "vv_dsp_stft_spectral_shape_device"):
        assert hasattr(lib, name), name


def test_argument_rules_in_order(api):
    row = np.linspace(0.0, 1.0, 513).astype(np.float32)
    good = params(1024)
    # 1. NULL params, row or out, whatever else is wrong
    for st, v in (api.row(row, good, null_row=True), api.row(row, None), api.row(row, params(0), null_row=True)):
        assert st == ERR_NULL and untouched(v)
    assert api.row(row, good, null_out=True)[0] == ERR_NULL
    # 2. n_fft < 2 comes before the band and the parameters
    for n_fft in (0, 1):
        for p in (params(n_fft), Params(n_fft, -1.0, 0, 9, 3, 7.0, -1.0)):
            st, v = api.row(row, p)
            assert st == ERR_SIZE and untouched(v)
    # 3. the band comes before the parameters and the limit
    for name, p in bad_bands().items():
        p.sample_rate = float("nan")
        st, v = api.row(row, p)
        assert st == ERR_RANGE and untouched(v), name
    st, v = api.row(row, params(40000, band=(3, 2)))
    assert st == ERR_RANGE and untouched(v)
    # 4. sample_rate, floor and rolloff come before the limit
    bad = bad_params()
    assert len(bad) == 13
    for name, p in bad.items():
        st, v = api.row(row, p)
        assert st == ERR_RANGE and untouched(v), name
        p.n_fft, p.k_max = 40000, 20000
        st, v = api.row(np.zeros(20001, np.float32), p)
        assert st == ERR_RANGE and untouched(v), name
    # 5. the kernel's limit: K = 8193 is in, 8194 is out
    st, v = api.row(np.zeros(8194, np.float32), params(16386))
    assert st == ERR_UNSUPPORTED and untouched(v)
    assert b"8193" in api.lib.vv_dsp_amd_last_error()
    assert api.row(np.zeros(8193, np.float32), params(16385))[0] in (OK, ERR_UNSUPPORTED)   # 16385 // 2 + 1 = 8193
    if api.lib.vvhip_available() <= 0:
        assert api.row(np.zeros(8193, np.float32), params(16384))[0] == ERR_UNSUPPORTED      # no device, not the limit
        assert b"no HIP device" in api.lib.vv_dsp_amd_last_error()


def test_device_forms_check_before_any_device_work(amd_lib_path):
    """vv_dsp_spectral_shape_device / vv_dsp_stft_spectral_shape_device decide every argument
    rule before a device is needed (the pointers are host dummies or NULL, never read)."""
    import vvdsp_amd as vv
    L = vv.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    P = vv.SpectralShapeParams

    def conv(q):
        return P(q.n_fft, q.sample_rate, q.magnitude, q.k_min, q.k_max, q.rolloff, q.floor)
    good = conv(params(1024))
    none = vv.SpectralShapeOut()
    full = vv.SpectralShapeOut(*([p] * 10))
    dev = L.vv_dsp_spectral_shape_device
    stf = L.vv_dsp_stft_spectral_shape_device
    vv.debug_clear("STAT_SHAPE_WAVE")
    for out in (none, full):
        o = C.byref(out)
        assert dev(None, 4, 513, 0, C.byref(good), o, None) == ERR_NULL
        assert dev(p, 4, 513, 0, None, o, None) == ERR_NULL
        assert dev(p, 4, 513, 0, C.byref(good), None, None) == ERR_NULL
        assert dev(None, 4, 512, 0, C.byref(conv(params(0))), o, None) == ERR_NULL
        assert dev(p, 4, 513, 0, C.byref(conv(params(1))), o, None) == ERR_SIZE
        assert dev(p, 4, 512, 0, C.byref(good), o, None) == ERR_SIZE                # row_pitch < K
        for name, b in bad_bands().items():
            assert dev(p, 4, 513, 0, C.byref(conv(b)), o, None) == ERR_RANGE, name
            assert dev(p, 4, 512, 0, C.byref(conv(b)), o, None) == ERR_SIZE, name    # the pitch first
        for name, b in bad_params().items():
            assert dev(p, 4, 513, 0, C.byref(conv(b)), o, None) == ERR_RANGE, name
            assert dev(p, 4, 512, 0, C.byref(conv(b)), o, None) == ERR_SIZE, name
            b.n_fft, b.k_max = 40000, 20000
            assert dev(p, 4, 20001, 0, C.byref(conv(b)), o, None) == ERR_RANGE, name   # before the limit
        assert dev(p, 4, 8194, 0, C.byref(conv(params(16386))), o, None) == ERR_UNSUPPORTED
        # the STFT form: its handle is a NULL here, which rule 1 answers
        assert stf(None, C.byref(good), p, 6400, 2, 6400, o, 22, None, None) == ERR_NULL
    # nothing requested, or no rows: OK, and nothing is launched (no device is asked for)
    assert dev(p, 4, 513, 0, C.byref(good), C.byref(none), None) == OK
    assert dev(p, 0, 513, 0, C.byref(good), C.byref(full), None) == OK
    assert np.all(buf == 0)
    assert vv.debug_get("STAT_SHAPE_WAVE") == 0


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    import vvdsp_amd as vv
    L.vvhip_set_error.argtypes = [C.c_char_p]
    L.vvhip_set_error(b"")
    row = su.case_rows(1024, 1, 5)[0]
    st, v = api.row(row, params(1024))
    assert st == ERR_UNSUPPORTED and untouched(v)                  # nothing computed on the CPU
    assert b"no HIP device" in L.vv_dsp_amd_last_error()
    st, v = api.row(row, params(1024), prev=row)
    assert st == ERR_UNSUPPORTED and untouched(v)
    # the device form with every check passed (the pointers are never read: there is no device)
    buf = np.zeros(2052, np.float32)
    p = buf.ctypes.data
    good = vv.SpectralShapeParams(1024, 16000.0, 0, 0, 512, 0.85, 1e-10)
    full = vv.SpectralShapeOut(*([p] * 10))
    assert vv.lib().vv_dsp_spectral_shape_device(p, 4, 513, 0, C.byref(good), C.byref(full), None) == ERR_UNSUPPORTED
    assert np.all(buf == 0)


def test_knob_and_counter_registered():
    import vvdsp_amd as vv
    try:
        vv.debug_set("SHAPE_DWORD", 1)
        assert vv.debug_get("SHAPE_DWORD") == 1 and vv.debug_get("VVHIP_SHAPE_DWORD") == 1
        vv.debug_clear("SHAPE_DWORD")
        assert vv.debug_get("SHAPE_DWORD") == -1
        for stat in ("STAT_SHAPE_WAVE", "STAT_SHAPE_VEC16"):
            vv.debug_clear(stat)
            assert vv.debug_get(stat) == 0
    finally:
        vv.debug_clear(None)


def test_binding_checks_without_gpu():
    """the checks of vvdsp_amd.spectral_shape / Stft.spectral_shape that need no device"""
    import torch
    import vvdsp_amd as vv
    good = vv.SpectralShapeParams(1024, 16000.0, 0, 0, 512, 0.85, 1e-10)
    assert vv.SHAPE_NAMES == su.NAMES
    assert C.sizeof(vv.SpectralShapeParams) == C.sizeof(Params)
    x = torch.zeros((4, 513), dtype=torch.float32)
    for call in (lambda: vv.spectral_shape(x, good, ("centroid",)),                 # not a device tensor
                 lambda: vv.spectral_shape(x[0], good, ("centroid",)),              # one dimension
                 lambda: vv.spectral_shape(x.double(), good, ("centroid",)),
                 lambda: vv.spectral_shape(x, (1024, 16000.0), ("centroid",)),      # not a SpectralShapeParams
                 lambda: vv.Stft.spectral_shape(None, x, good, ("centroid",))):     # not a device signal
        with pytest.raises(vv.VvError):
            call()


# ------------------------------------------------------------- the model
def test_model_known_answers():
    fs = 16000.0
    for n_fft, j, band in ((1024, 100, None), (1024, 100, (50, 300)), (130, 64, None), (4, 2, None)):
        K = n_fft // 2 + 1
        prm = params(n_fft, band=band)
        k0, k1 = prm.k_min, prm.k_max
        B = k1 - k0 + 1
        # one non-zero bin
        row = np.zeros(K, np.float32)
        row[j] = 3.0
        m = su.model_row(row, None, prm)
        hz = np.float32(j * fs / n_fft)
        assert m["centroid"] == hz and m["rolloff"] == hz and m["peak_bin"] == j and m["rolloff_bin"] == j
        assert m["spread"] == 0 and m["skewness"] == 0 and m["kurtosis"] == 0 and m["energy"] == 3.0
        want = np.exp((np.log(3.0) + (B - 1) * np.log(np.float64(np.float32(1e-10)))) / B) / \
            ((3.0 + (B - 1) * np.float64(np.float32(1e-10))) / B)
        assert abs(float(m["flatness"]) - want) <= 1e-6 * want
        assert m["crest"] == np.float32(B)
        # a constant row
        m = su.model_row(np.full(K, 0.25, np.float32), None, prm)
        assert m["centroid"] == np.float32((k0 + k1) / 2.0 * fs / n_fft)
        assert m["flatness"] == 1.0 and m["crest"] == 1.0 and m["peak_bin"] == k0
        # an all-zero row
        z = su.model_row(np.zeros(K, np.float32), None, prm)
        for n in ("energy", "centroid", "spread", "skewness", "kurtosis", "flux", "crest"):
            assert z[n] == 0.0, n
        assert z["flatness"] == 1.0 and z["rolloff_bin"] == k0 and z["peak_bin"] == k0
        assert not z["rolloff_undecidable"]
        # identical rows: flux 0
        r = su.case_rows(n_fft, 1, 3)[0]
        assert su.model_row(r, r, prm)["flux"] == 0.0 and su.model_row(r, r * np.float32(0.5), prm)["flux"] > 0
    # a NaN and a negative power poison the f64 class of their row
    r = su.case_rows(1024, 1, 4)[0].copy()
    r[7] = np.nan
    m = su.model_row(r, None, params(1024))
    assert all(np.isnan(m[n]) for n in ("energy", "centroid", "spread", "skewness", "kurtosis", "flatness", "crest"))
    assert m["peak_undecidable"]
    r[7] = -1.0
    assert np.isnan(su.model_row(r, None, params(1024, magnitude=1))["energy"])


def test_model_against_numpy_one_liners():
    for n_fft, mag, seed in ((1024, 0, 1), (1024, 1, 2), (130, 0, 3), (16384, 1, 4)):
        K = n_fft // 2 + 1
        rows = su.case_rows(n_fft, 2, seed)
        prm = params(n_fft, magnitude=mag, band=(1, K - 2) if K > 3 else None)
        k0, k1 = prm.k_min, prm.k_max
        m = su.model_rows(rows, prm)
        w = (np.sqrt(rows) if mag else rows).astype(np.float64)[:, k0:k1 + 1]
        k = np.arange(k0, k1 + 1, dtype=np.float64)
        s = 16000.0 / n_fft
        S0 = np.sum(w, axis=1)
        c = np.sum(k * w, axis=1) / S0
        sd = np.sqrt(np.sum((k - c[:, None]) ** 2 * w, axis=1) / S0)
        wf = np.maximum(w, np.float64(np.float32(1e-10)))
        want = {
            "energy": S0, "centroid": c * s, "spread": sd * s,
            "skewness": np.sum((k - c[:, None]) ** 3 * w, axis=1) / S0 / sd ** 3,
            "kurtosis": np.sum((k - c[:, None]) ** 4 * w, axis=1) / S0 / sd ** 4,
            "flatness": np.exp(np.mean(np.log(wf), axis=1)) / np.mean(wf, axis=1),
            "flux": np.array([0.0, np.sqrt(np.sum((w[1] - w[0]) ** 2))]),
            "crest": np.max(w, axis=1) / np.mean(w, axis=1),
        }
        for n, v in want.items():
            # the model's f64 value against the one-liner at 1e-12 relative ...
            assert np.all(np.abs(m[n + "_f64"] - v) <= 1e-12 * np.abs(v)), (n, m[n + "_f64"], v)
            # ... and its stored float is that value rounded once
            assert np.array_equal(m[n], m[n + "_f64"].astype(np.float32)), n
            assert np.all(np.abs(m[n].astype(np.float64) - v) <= 2.0 ** -24 * np.abs(v) + 1e-12 * np.abs(v)), n
        assert np.array_equal(m["peak_bin"], k0 + np.argmax(w, axis=1))
        kr = np.array([np.searchsorted(np.cumsum(w[r]), 0.85 * S0[r]) for r in range(2)])
        assert np.array_equal(m["rolloff_bin"], k0 + kr)
    # unrounded: the model's f64 centroid against the one-liner at 1e-12
    rows = su.case_rows(1024, 1, 9)
    w = rows[0].astype(np.float64)
    k = np.arange(513.0)
    c = su._fsum(k * w) / su._fsum(w)
    assert abs(c - np.sum(k * w) / np.sum(w)) <= 1e-12 * c


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case_table_leaves_no_row_undecidable(i):
    """every exact-class decision of the model on the case table rests on a gap far above
    what another f64 summation order moves: no GPU test can hide a wrong decision behind
    "undecidable".  The cap is zero."""
    case = CASES[i]
    rows, m = su.case_model(i)
    K = case[0] // 2 + 1
    assert rows.shape == (case[1], K) and np.all(rows > 0)
    assert su.case_pitch(case) >= K
    assert int(np.sum(m["rolloff_undecidable"])) == 0
    assert int(np.sum(m["peak_undecidable"])) == 0
    assert np.all(m["skew_bound"] < 1e-10)
    assert np.all(np.isfinite(m["energy"])) and np.all(m["energy"] > 0)
    if case[1] > 1:
        assert np.all(m["flux"][1:] > 0) and m["flux"][0] == 0


def test_case_table_covers_the_issue():
    assert sorted({c[0] for c in CASES}) == [2, 4, 126, 128, 130, 256, 512, 1024, 16384]
    for n_fft in {c[0] for c in CASES}:
        assert {c[1] for c in CASES if c[0] == n_fft} >= ({1, 2, 7} if n_fft > 4 else {7})
    assert {c[4] for c in CASES} == {"all", "lo1", "hi2", "one"}
    assert {c[5] for c in CASES} == {0, 1} and {c[6] for c in CASES} == {0.5, 0.85, 1.0}
    assert any(c[0] == 1024 and c[2] == 544 for c in CASES) and any(c[3] == 1 for c in CASES)
    assert any(c[2] == 1 for c in CASES) and any(c[2] == 0 for c in CASES)
