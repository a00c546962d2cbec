"""CPU tests of the LPC front-end (include/vv_dsp/envelope/lpc.h, envelope.h):
argument checks in the reference's order with the statuses recorded from it
(tests/golden/lpc_cases.npz), outputs untouched where the reference leaves
them, the knob and counters of the kernel choice, and -- with no GPU --
UNSUPPORTED instead of a CPU computation."""
import ctypes as C

import numpy as np
import pytest

from lpc_util import LpcApi, load, SENTINEL, ERR_INTERNAL, ERR_UNSUPPORTED, OK


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return LpcApi(amd_lib_path)


@pytest.fixture(scope="module")
def cases():
    return load("lpc_cases")


def test_argument_cases_match_reference(api, cases):
    want = dict(zip((str(s) for s in cases["arg_names"]), (int(s) for s in cases["arg_status"])))
    got = api.argument_cases(device=False)
    assert len(got) >= 19
    for name, st in got.items():
        assert st == want[name], (name, st, want[name])


def test_degenerate_levinson_leaves_outputs_untouched(api, cases):
    for r in cases["deg_r"]:
        st, a, err = api.levinson(r)
        assert st == ERR_INTERNAL
        assert np.all(a == SENTINEL) and err == SENTINEL


def test_lpspec_nfft0_writes_nothing(api):
    a = np.array([1.0, 0.5], np.float32)
    mag = np.full(4, SENTINEL, np.float32)
    fp = C.POINTER(C.c_float)
    assert api.lib.vv_dsp_lpspec(a.ctypes.data_as(fp), 1, 1.0, 0, mag.ctypes.data_as(fp)) == OK
    assert np.all(mag == SENTINEL)


def test_envelope_dummy(api):
    assert api.lib.vv_dsp_envelope_dummy() == 5


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    L.vvhip_last_error.restype = C.c_char_p
    L.vvhip_set_error.argtypes = [C.c_char_p]
    x = np.linspace(-1.0, 1.0, 64).astype(np.float32)
    calls = {
        "autocorr": lambda: api.autocorr(x, 4),
        "levinson": lambda: api.levinson(np.array([2.0, 1.0, 0.5], np.float32)),
        "lpc": lambda: api.lpc(x, 4),
        "lpspec": lambda: api.lpspec(np.array([1.0, -0.5], np.float32), 1.0, 16),
    }
    for name, call in calls.items():
        L.vvhip_set_error(b"")
        res = call()
        assert res[0] == ERR_UNSUPPORTED, name
        assert np.all(res[1] == SENTINEL), name    # nothing computed on the CPU
        assert b"no HIP device" in L.vvhip_last_error(), name


def test_lpc_knob_and_counters():
    import vvdsp_amd as vv
    try:
        vv.debug_set("LPC_GENERIC", 1)
        assert vv.debug_get("LPC_GENERIC") == 1 and vv.debug_get("VVHIP_LPC_GENERIC") == 1
        vv.debug_clear("LPC_GENERIC")
        assert vv.debug_get("LPC_GENERIC") == -1
        for st in ("STAT_LPC_WAVE", "STAT_LPC_GENERIC"):
            vv.debug_clear(st)
            assert vv.debug_get(st) == 0
    finally:
        vv.debug_clear(None)
