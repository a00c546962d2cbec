"""CPU tests of the statistics front-end (include/vv_dsp/core/stats.h): argument
checks in the reference's order with the statuses recorded from it
(tests/golden/stats_args.npz), the reference's `*out = 0` writes and outputs
otherwise untouched, the knob and counters of the route choice, and -- with no
GPU -- UNSUPPORTED instead of a CPU computation."""
import ctypes as C

import numpy as np
import pytest

from stats_util import (StatsApi, load, STAT_NAMES, COUNT_NAMES, MIN_LEN, SENTINEL, SENTINEL_IDX, ERR_NULL, ERR_SIZE,
                        ERR_UNSUPPORTED, OK)


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return StatsApi(amd_lib_path)


def test_argument_cases_match_reference(api):
    z = load("stats_args")
    want = dict(zip((str(s) for s in z["arg_names"]), (int(s) for s in z["arg_status"])))
    got = api.argument_cases(device=False)
    assert len(got) >= 60
    for name, st in got.items():
        assert st == want[name], (name, st, want[name])
    # the quirks, spelled out: n == 0 is a NULL_POINTER, pointers come before sizes
    assert got["sum_n0"] == ERR_NULL and got["var_null_x_short"] == ERR_NULL and got["var_short"] == ERR_SIZE
    assert got["auto_rlen0"] == ERR_SIZE and got["auto_null_r_rlen0"] == ERR_NULL
    assert got["peak_no_outputs"] == OK and got["peak_n0_no_outputs"] == ERR_NULL


def test_size_rules_write_zero_and_nothing_else(api):
    x = np.linspace(-1.0, 1.0, 8).astype(np.float32)
    for name, least in MIN_LEN.items():
        for n in range(1, least):
            st, v = api.stat(name, x, n)
            assert st == ERR_SIZE and v == 0.0 and v != SENTINEL, (name, n)   # the reference's *out = 0
    # a refused call leaves its output alone
    for name in STAT_NAMES:
        st, v = api.stat(name, x, 0)
        assert st == ERR_NULL and v == (SENTINEL_IDX if name in COUNT_NAMES else SENTINEL), name
    st, r = api.autocorrelation(x, 0, 0)
    assert st == ERR_SIZE
    r = np.full(4, SENTINEL, np.float32)
    fp = C.POINTER(C.c_float)
    assert api.lib.vv_dsp_cross_correlation(x.ctypes.data_as(fp), 8, x.ctypes.data_as(fp), 0, r.ctypes.data_as(fp),
                                            4) == ERR_NULL
    assert np.all(r == SENTINEL)


def test_device_forms_check_before_any_device_work(amd_lib_path):
    """vv_dsp_stats_device / _frames_device: no output wanted is OK, a size rule or a zero
    hop / frame_len is INVALID_SIZE -- decided before a device is needed (the pointers are
    host dummies, never read)."""
    import vvdsp_amd as vv
    L = vv.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    none = vv.StatsOut()
    assert L.vv_dsp_stats_device(p, 8, 2, 8, C.byref(none), None) == OK
    assert L.vv_dsp_stats_device(None, 8, 2, 8, C.byref(none), None) == ERR_NULL
    assert L.vv_dsp_stats_device(p, 8, 2, 8, None, None) == ERR_NULL
    assert L.vv_dsp_stats_frames_device(p, 64, 1, 64, 8, 4, 0, None, C.byref(none), 15, None) == OK
    for name, least in MIN_LEN.items():
        o = vv.StatsOut()
        setattr(o, name, p)
        assert L.vv_dsp_stats_device(p, least - 1, 2, 8, C.byref(o), None) == ERR_SIZE, name
        assert L.vv_dsp_stats_frames_device(p, 64, 1, 64, least - 1, 1, 0, None, C.byref(o), 64, None) == ERR_SIZE
    o = vv.StatsOut()
    o.rms = p
    assert L.vv_dsp_stats_device(p, 0, 2, 8, C.byref(o), None) == ERR_SIZE
    assert L.vv_dsp_stats_frames_device(p, 64, 1, 64, 8, 0, 0, None, C.byref(o), 15, None) == ERR_SIZE
    assert L.vv_dsp_stats_frames_device(p, 64, 1, 64, 0, 4, 0, None, C.byref(o), 15, None) == ERR_SIZE
    assert L.vv_dsp_autocorrelation_device(p, 8, 1, 0, 0, p, None) == ERR_SIZE
    assert L.vv_dsp_autocorrelation_device(p, 0, 1, 4, 0, p, None) == ERR_NULL
    assert L.vv_dsp_cross_correlation_device(p, 8, None, 8, 1, 4, p, None) == ERR_NULL
    assert np.all(buf == 0)


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    L.vvhip_last_error.restype = C.c_char_p
    L.vvhip_set_error.argtypes = [C.c_char_p]
    x = np.linspace(-1.0, 1.0, 64).astype(np.float32)
    calls = {name: (lambda name=name: api.stat(name, x)) for name in STAT_NAMES}
    calls["peak"] = lambda: api.peak(x)
    calls["peak_min_only"] = lambda: api.peak(x, True, False)
    calls["autocorrelation"] = lambda: api.autocorrelation(x, 8, 1)
    calls["cross_correlation"] = lambda: api.cross_correlation(x, x[:40], 8)
    for name, call in calls.items():
        L.vvhip_set_error(b"")
        res = call()
        assert res[0] == ERR_UNSUPPORTED, name
        for out in res[1:]:                                  # nothing computed on the CPU
            assert np.all(np.asarray(out) == (SENTINEL_IDX if name in COUNT_NAMES else SENTINEL)), name
        assert b"no HIP device" in L.vvhip_last_error(), name


def test_stats_knob_and_counters():
    import vvdsp_amd as vv
    try:
        vv.debug_set("STATS_LONG", 1)
        assert vv.debug_get("STATS_LONG") == 1 and vv.debug_get("VVHIP_STATS_LONG") == 1
        vv.debug_clear("STATS_LONG")
        assert vv.debug_get("STATS_LONG") == -1
        for st in ("STAT_STATS_WAVE", "STAT_STATS_LONG"):
            vv.debug_clear(st)
            assert vv.debug_get(st) == 0
    finally:
        vv.debug_clear(None)


def test_binding_checks_without_gpu():
    """the checks of vvdsp_amd.stats / stats_frames / the correlations that need no device"""
    import torch
    import vvdsp_amd as vv
    x = torch.zeros((2, 8), dtype=torch.float32)
    for call in (lambda: vv.stats(x, ("rms",)),                                   # not a device tensor
                 lambda: vv.stats_frames(x, 4, 2, ("rms",)),
                 lambda: vv.autocorrelation(x, 4),
                 lambda: vv.cross_correlation(x, x, 4)):
        with pytest.raises(vv.VvError):
            call()
