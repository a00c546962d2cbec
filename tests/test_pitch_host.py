"""CPU tests of the pitch front-end (include/vv_dsp/features/pitch.h): the argument
checks in the header's order with outputs untouched, vv_dsp_pitch_lag_range
against the table of cases, the device forms' checks before any device work,
-- with no GPU -- UNSUPPORTED instead of a CPU computation, the binding's checks,
and the f64 model of the definition (tests/pitch_util.py) on known answers and
on the fixture, where it must leave no frame undecidable."""
import ctypes as C

import numpy as np
import pytest

import pitch_util as pu
from pitch_util import (PitchApi, Params, params, CASES, CASE_IDS, SENTINEL, SENTINEL_LAG, OK, ERR_NULL, ERR_SIZE,
                        ERR_RANGE, ERR_UNSUPPORTED)


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return PitchApi(amd_lib_path)


GOOD = (16000.0, 80.0, 400.0, 0.15)


def bad_params():
    """name -> parameters that are OUT_OF_RANGE"""
    inf, nan = float("inf"), float("nan")
    res = {}
    for i, field in enumerate(("sample_rate", "fmin", "fmax")):
        for name, v in (("zero", 0.0), ("negative", -1.0), ("inf", inf), ("nan", nan)):
            p = list(GOOD)
            p[i] = v
            res[f"{field}_{name}"] = Params(*p)
    res["fmin_equals_fmax"] = Params(16000.0, 200.0, 200.0, 0.15)
    res["fmin_above_fmax"] = Params(16000.0, 400.0, 80.0, 0.15)
    res["fmax_above_nyquist"] = Params(16000.0, 80.0, 8000.5, 0.15)
    res["threshold_zero"] = Params(16000.0, 80.0, 400.0, 0.0)
    res["threshold_negative"] = Params(16000.0, 80.0, 400.0, -0.1)
    res["threshold_above_one"] = Params(16000.0, 80.0, 400.0, 1.0001)
    res["threshold_nan"] = Params(16000.0, 80.0, 400.0, nan)
    return res


def test_argument_rules_in_order(api):
    x = np.linspace(-1.0, 1.0, 400).astype(np.float32)
    good = Params(*GOOD)

    def untouched(res):
        return res[1] == SENTINEL and res[2] == SENTINEL

    # 1. NULL x or params, whatever else is wrong
    for res in (api.yin(x, good, null_x=True), api.yin(x, None), api.yin(x, None, n=0),
                api.yin(x, Params(0.0, 0.0, 0.0, 0.0), n=0, null_x=True)):
        assert res[0] == ERR_NULL and untouched(res)
    # 2. n == 0 comes before the parameters
    for p in (good, Params(-1.0, 80.0, 400.0, 0.15), Params(16000.0, 80.0, 400.0, 7.0)):
        res = api.yin(x, p, n=0)
        assert res[0] == ERR_SIZE and untouched(res)
    # 3. OUT_OF_RANGE comes before the frame's size and the kernel's limits
    bad = bad_params()
    assert len(bad) == 19
    for name, p in bad.items():
        for n in (400, 3, 100000):
            res = api.yin(np.zeros(n, np.float32), p)
            assert res[0] == ERR_RANGE and untouched(res), (name, n)
            assert api.lag_range(p, n) == (ERR_RANGE,) + (SENTINEL_LAG,) * 3, (name, n)
    # (tau_min >= tau_max cannot be reached once fmin < fmax <= fs / 2 holds: the narrowest range
    # at the top still spans two lags)
    assert api.lag_range(Params(16000.0, 7999.5, 8000.0, 0.15), 64)[:3] == (OK, 2, 3)
    # threshold 1 is inside (0, 1]
    assert api.lag_range(Params(16000.0, 80.0, 400.0, 1.0), 400)[0] == OK
    # 4. W < 1: frame_len <= tau_max, before the limits
    for n in (1, 200):
        res = api.yin(x[:n], good)
        assert res[0] == ERR_SIZE and untouched(res), n
    assert api.lag_range(good, 200) == (ERR_SIZE,) + (SENTINEL_LAG,) * 3
    assert api.lag_range(good, 201)[0] == OK
    assert api.lag_range(Params(16000.0, 1.0, 400.0, 0.15), 16000)[0] == ERR_SIZE     # tau_max 16000 > 8191 too
    # 5. the kernel's limits
    assert api.lag_range(good, 16384)[0] == OK
    assert api.lag_range(good, 16385) == (ERR_UNSUPPORTED,) + (SENTINEL_LAG,) * 3
    p = Params(16000.0, 16000.0 / 8191.0, 400.0, 0.15)
    tau_max = pu.lag_range(16000.0, p.fmin, 400.0, 16384)[1]
    assert tau_max in (8191, 8192)
    assert api.lag_range(p, 16384)[0] == (OK if tau_max == 8191 else ERR_UNSUPPORTED)
    assert api.lag_range(Params(16000.0, 1.95, 400.0, 0.15), 16384)[0] == ERR_UNSUPPORTED   # tau_max 8206
    res = api.yin(np.zeros(16385, np.float32), good)
    assert res[0] == ERR_UNSUPPORTED and untouched(res)
    assert b"16384" in api.lib.vv_dsp_amd_last_error()


def test_lag_range_matches_the_table(api):
    for (frame, hop, lo, hi, center, win, thr), want in CASES:
        assert api.lag_range(params(lo, hi, thr), frame) == (OK,) + want
        assert pu.lag_range(pu.FS, lo, hi, frame) == want
    L = api.lib
    good = Params(*GOOD)
    assert L.vv_dsp_pitch_lag_range(None, 400, None, None, None) == ERR_NULL
    assert L.vv_dsp_pitch_lag_range(C.byref(good), 0, None, None, None) == ERR_SIZE
    assert L.vv_dsp_pitch_lag_range(C.byref(good), 400, None, None, None) == OK       # every output is optional
    w = C.c_size_t(0)
    assert L.vv_dsp_pitch_lag_range(C.byref(good), 400, None, None, C.byref(w)) == OK and w.value == 200


def test_device_forms_check_before_any_device_work(amd_lib_path):
    """vv_dsp_pitch_device / _frames_device decide every argument rule before a device is
    needed (the pointers are host dummies or NULL, never read)."""
    import vvdsp_amd as vv
    L = vv.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    good = vv.PitchParams(*GOOD)
    none = vv.PitchOut()
    full = vv.PitchOut(p, p, p, p)
    dev = L.vv_dsp_pitch_device
    frm = L.vv_dsp_pitch_frames_device
    for out in (none, full):
        o = C.byref(out)
        assert dev(None, 400, 2, 400, C.byref(good), o, 201, None) == ERR_NULL
        assert dev(p, 400, 2, 400, None, o, 201, None) == ERR_NULL
        assert dev(p, 400, 2, 400, C.byref(good), None, 201, None) == ERR_NULL
        assert dev(None, 0, 2, 400, C.byref(good), o, 201, None) == ERR_NULL
        assert dev(p, 0, 2, 400, C.byref(good), o, 201, None) == ERR_SIZE
        assert dev(p, 200, 2, 400, C.byref(good), o, 201, None) == ERR_SIZE
        assert dev(p, 16385, 2, 16385, C.byref(good), o, 201, None) == ERR_UNSUPPORTED
        assert frm(None, 6400, 2, 6400, 400, 160, 0, None, C.byref(good), o, 38, 38 * 201, None) == ERR_NULL
        assert frm(p, 6400, 2, 6400, 400, 160, 0, None, None, o, 38, 38 * 201, None) == ERR_NULL
        assert frm(p, 6400, 2, 6400, 400, 0, 0, None, C.byref(good), o, 38, 38 * 201, None) == ERR_SIZE
        assert frm(p, 6400, 2, 6400, 0, 160, 0, None, C.byref(good), o, 38, 38 * 201, None) == ERR_SIZE
        assert frm(p, 6400, 2, 6400, 200, 160, 0, None, C.byref(good), o, 38, 38 * 201, None) == ERR_SIZE
        assert frm(p, 99999, 2, 99999, 16385, 160, 0, None, C.byref(good), o, 38, 38, None) == ERR_UNSUPPORTED
        for name, bad in bad_params().items():
            b = vv.PitchParams(bad.sample_rate, bad.fmin, bad.fmax, bad.threshold)
            assert dev(p, 400, 2, 400, C.byref(b), o, 201, None) == ERR_RANGE, name
            assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(b), o, 38, 38 * 201, None) == ERR_RANGE, name
            assert dev(p, 0, 2, 400, C.byref(b), o, 201, None) == ERR_SIZE, name          # n == 0 first
    # nothing requested: OK, and nothing is launched (no device is asked for)
    assert dev(p, 400, 2, 400, C.byref(good), C.byref(none), 0, None) == OK
    assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(good), C.byref(none), 0, 0, None) == OK
    # strides shorter than what they step over
    assert dev(p, 400, 2, 399, C.byref(good), C.byref(full), 201, None) == ERR_SIZE
    assert dev(p, 400, 2, 400, C.byref(good), C.byref(full), 200, None) == ERR_SIZE
    assert frm(p, 6400, 2, 6399, 400, 160, 0, None, C.byref(good), C.byref(full), 38, 38 * 201, None) == ERR_SIZE
    assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(good), C.byref(full), 37, 38 * 201, None) == ERR_SIZE
    assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(good), C.byref(full), 38, 38 * 201 - 1, None) == ERR_SIZE
    assert np.all(buf == 0)
    assert vv.debug_get("STAT_PITCH_WAVE") == 0


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    L.vvhip_set_error.argtypes = [C.c_char_p]
    x = np.sin(2 * np.pi * 200.0 * np.arange(400) / 16000.0).astype(np.float32)
    L.vvhip_set_error(b"")
    st, f0, ap = api.yin(x, Params(*GOOD))
    assert st == ERR_UNSUPPORTED
    assert f0 == SENTINEL and ap == SENTINEL                       # nothing computed on the CPU
    assert b"no HIP device" in L.vv_dsp_amd_last_error()
    # no output wanted: nothing to compute, OK
    assert L.vv_dsp_pitch_yin(x.ctypes.data_as(C.POINTER(C.c_float)), 400, C.byref(Params(*GOOD)), None, None) == OK


def test_knob_and_counter_registered():
    import vvdsp_amd as vv
    try:
        vv.debug_set("PITCH_F32", 1)
        assert vv.debug_get("PITCH_F32") == 1 and vv.debug_get("VVHIP_PITCH_F32") == 1
        vv.debug_clear("PITCH_F32")
        assert vv.debug_get("PITCH_F32") == -1
        vv.debug_clear("STAT_PITCH_WAVE")
        assert vv.debug_get("STAT_PITCH_WAVE") == 0
    finally:
        vv.debug_clear(None)


def test_binding_checks_without_gpu():
    """the checks of vvdsp_amd.pitch / pitch_frames / pitch_lag_range that need no device"""
    import torch
    import vvdsp_amd as vv
    good = vv.PitchParams(*GOOD)
    x = torch.zeros((2, 400), dtype=torch.float32)
    assert vv.pitch_lag_range(good, 400) == (40, 200, 200)
    assert vv.PITCH_NAMES == ("f0", "aperiodicity", "lag", "cmnd")
    for call in (lambda: vv.pitch(x, good, ("f0",)),                              # not a device tensor
                 lambda: vv.pitch_frames(x, 400, 160, good, ("f0",)),
                 lambda: vv.pitch_frames(x, 400, 0, good, ("f0",)),
                 lambda: vv.pitch_lag_range(good, 200),                           # W < 1
                 lambda: vv.pitch_lag_range(vv.PitchParams(16000.0, 400.0, 80.0, 0.15), 400),
                 lambda: vv.pitch_lag_range((16000.0, 80.0, 400.0, 0.15), 400)):  # not a PitchParams
        with pytest.raises(vv.VvError):
            call()


# ------------------------------------------------------------- the model
def test_model_known_answers():
    """three-harmonic tones: the definition finds the fundamental to 1e-3 relative (twice
    the worst a CPU prototype of this model measured: 4.7e-4 at n = 400, 3.0e-4 at 1024).
    This guards the definition, not the kernel."""
    rng = np.random.default_rng(7)
    for n in (400, 1024):
        worst = 0.0
        for f in (82.4, 100.0, 123.4, 220.5, 311.1, 399.0):
            for phase in (0.0, 1.3):
                m = pu.model_rows(pu.tone(f, phase, n, rng)[None], 80.0, 400.0, 0.15)
                assert m["f0"][0] > 0, (n, f, phase)
                worst = max(worst, abs(float(m["f0"][0]) - f) / f)
        print(f"n={n}: worst relative error {worst:.3g}")
        assert worst <= 1e-3, (n, worst)


def test_model_noise_and_silence():
    rng = np.random.default_rng(11)
    noise = rng.standard_normal((8, 400)).astype(np.float32)
    m = pu.model_rows(noise, 80.0, 400.0, 0.15)
    assert np.all(m["f0"] == 0) and np.all(m["aperiodicity"] >= 0.15)
    assert np.all((m["lag"] >= 40) & (m["lag"] <= 200))
    for row in (np.zeros(400, np.float32), np.full(400, 0.1, np.float32)):
        z = pu.model_rows(row[None], 80.0, 400.0, 0.15)
        assert (z["f0"][0], z["aperiodicity"][0], z["lag"][0]) == (0.0, 1.0, 40)
        assert np.all(z["cmnd"] == 1.0)
    bad = noise[0].copy()
    bad[399] = np.nan
    z = pu.model_rows(bad[None], 80.0, 400.0, 0.15)
    assert z["f0"][0] == 0 and np.isnan(z["aperiodicity"][0]) and z["lag"][0] == 0
    # a square wave of period 50: d(50) = 0 exactly, so lag 50 and aperiodicity 0.  d(49) == d(51),
    # but d' weighs them by tau / c(tau): a = d'(49) < c = d'(51), the parabola's vertex sits left
    # of 50 by (c - a) / (2 (a + c)) and f0 is that much above 16000 / 50
    z = pu.model_rows(pu.square_wave(400, 50)[None], 80.0, 400.0, 0.15)
    assert (z["aperiodicity"][0], z["lag"][0]) == (0.0, 50)
    a, c = np.float64(z["cmnd"][0][49]), np.float64(z["cmnd"][0][51])
    assert c > a > 0 and abs(float(z["f0"][0]) - 16000.0 / (50.0 + (a - c) / (2.0 * (a + c)))) < 1e-3
    assert 320.0 < z["f0"][0] < 320.1


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_fixture_leaves_no_frame_undecidable(i):
    """every decision of the model on the fixture rests on a gap far above what another
    f64 summation order moves: an edited fixture cannot hollow out the GPU comparison"""
    case = CASES[i][0]
    rows = pu.case_rows(case)
    assert rows.shape[0] == 2 and rows.shape[1] == pu.num_frames(6400, case[0], case[1], case[4]) >= 13
    m = pu.case_model(i)
    print(f"{CASE_IDS[i]}: {m['margin'].size} frames, smallest margin {m['margin'].min():.3g}, "
          f"{int(np.sum(m['f0'] > 0))} voiced")
    assert np.sum(m["margin"] < pu.MARGIN) == 0
    assert np.sum(m["f0"] > 0) >= 10 and np.sum(m["f0"] == 0) >= 3          # both branches are exercised
    # another summation order (strict sequential) decides the same and rounds the same
    r2 = rows.reshape(-1, rows.shape[2])
    s = pu.model_rows(r2, case[2], case[3], case[6], sequential=True)
    assert np.array_equal(s["lag"], m["lag"].reshape(-1))
    for k in ("f0", "aperiodicity", "cmnd"):
        assert pu.f32_ulps(s[k], m[k].reshape(s[k].shape)).max() <= 1, k
