"""CPU tests of the interpolation front-end (include/vv_dsp/resample/interpolate.h,
vv_dsp/resample.h and the batched forms of vv_dsp_amd.h): the float32 model
against the reference's recorded outputs (tests/golden/interp_ref.npz), argument
checks in the reference's order with the statuses recorded from it, the device
forms' checks before any device work, the knob and counters of the rows route,
the bindings' checks, the umbrella header alone under a C and a C++ compiler,
and -- with no GPU -- UNSUPPORTED instead of a CPU computation."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from interp_util import (InterpApi, load, model, same, row, special_row, positions, METHODS, ROW_N, SPECIAL_N, SENTINEL,
                         LINEAR, CUBIC, OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_UNSUPPORTED)


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return InterpApi(amd_lib_path)


@pytest.fixture(scope="module")
def golden():
    return load("interp_ref")


def test_model_equals_reference(golden):
    total = 0
    for n in ROW_N:
        for method in METHODS:
            want = golden[f"n{n}_{method}"]
            assert np.all(np.isfinite(want))
            assert same(model(row(n), positions(n), method), want), (n, method)
            total += want.size
    for kind in ("inf", "nan"):
        for method in METHODS:
            want = golden[f"{kind}_{method}"]
            got = model(special_row(kind), positions(SPECIAL_N), method)
            finite = np.isfinite(want)
            assert 0 < np.sum(~finite) < want.size
            assert same(got[finite], want[finite]), (kind, method)
            assert same(got, want, nan_equal=True), (kind, method)
            total += want.size
    assert total > 40000


def test_model_defines_nan_and_inf_positions():
    x = row(5)
    pos = np.array([np.nan, np.inf, -np.inf, 1.5], np.float32)
    for method in METHODS:
        y = model(x, pos, method)
        assert np.isnan(y[0]) and y[1] == x[4] and y[2] == x[0] and np.isfinite(y[3])
    assert model(x[:1], pos, "cubic").tolist() == [x[0]] * 4      # the cubic's n < 2 rule comes first
    assert np.isnan(model(x[:1], pos, "linear")[0])


def test_argument_cases_match_reference(api, golden):
    want = dict(zip((str(s) for s in golden["arg_names"]), (int(s) for s in golden["arg_status"])))
    got = api.argument_cases(device=False)
    assert len(got) == 10
    for name, st in got.items():
        assert st == want[name], (name, st, want[name])
    assert got["linear_null_x_n0"] == ERR_NULL and got["cubic_n0"] == ERR_SIZE
    # a refused call leaves its output alone
    for method in METHODS:
        st, v = api.one(method, row(5), 1.5, n=0)
        assert st == ERR_SIZE and v == SENTINEL


def test_device_forms_check_before_any_device_work(amd_lib_path):
    """every check is decided before a device is needed: the pointers are host dummies,
    never read, and nothing is written"""
    import vvdsp_amd as vv
    L = vv.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    dev, uni, host = L.vv_dsp_interpolate_device, L.vv_dsp_interpolate_uniform_device, L.vv_dsp_interpolate_real_batch
    # pointers first, then n == 0
    assert dev(None, 8, 2, 8, p, 4, 0, LINEAR, p, 4, None) == ERR_NULL
    assert dev(p, 8, 2, 8, None, 4, 0, LINEAR, p, 4, None) == ERR_NULL
    assert dev(p, 8, 2, 8, p, 4, 0, LINEAR, None, 4, None) == ERR_NULL
    assert dev(None, 0, 2, 8, p, 4, 0, LINEAR, p, 4, None) == ERR_NULL
    assert dev(p, 0, 2, 8, p, 4, 0, LINEAR, p, 4, None) == ERR_SIZE
    assert dev(p, 0, 0, 8, p, 0, 0, LINEAR, p, 4, None) == ERR_SIZE
    assert uni(None, 8, 2, 8, 0.0, 1.0, 4, LINEAR, p, 4, None) == ERR_NULL
    assert uni(p, 8, 2, 8, 0.0, 1.0, 4, LINEAR, None, 4, None) == ERR_NULL
    assert uni(p, 0, 2, 8, 0.0, 1.0, 4, LINEAR, p, 4, None) == ERR_SIZE
    assert host(None, 8, p, 4, LINEAR, p) == ERR_NULL
    assert host(p, 8, None, 4, LINEAR, p) == ERR_NULL
    assert host(p, 8, p, 4, LINEAR, None) == ERR_NULL
    assert host(p, 0, p, 4, LINEAR, p) == ERR_SIZE
    # nothing to do
    assert dev(p, 8, 2, 8, p, 0, 0, LINEAR, p, 4, None) == OK
    assert dev(p, 8, 0, 8, p, 4, 0, LINEAR, p, 4, None) == OK
    assert uni(p, 8, 2, 8, 0.0, 1.0, 0, CUBIC, p, 4, None) == OK
    assert uni(p, 8, 0, 8, 0.0, 1.0, 4, CUBIC, p, 4, None) == OK
    assert host(p, 8, p, 0, CUBIC, p) == OK
    # a non-zero stride shorter than its row
    assert dev(p, 8, 2, 7, p, 4, 0, LINEAR, p, 4, None) == ERR_SIZE
    assert dev(p, 8, 2, 8, p, 4, 3, LINEAR, p, 4, None) == ERR_SIZE
    assert dev(p, 8, 2, 8, p, 4, 0, LINEAR, p, 3, None) == ERR_SIZE
    assert dev(p, 8, 2, 8, p, 4, 0, LINEAR, p, 0, None) == ERR_SIZE      # two rows onto one
    assert uni(p, 8, 2, 7, 0.0, 1.0, 4, LINEAR, p, 4, None) == ERR_SIZE
    assert uni(p, 8, 2, 8, 0.0, 1.0, 4, LINEAR, p, 3, None) == ERR_SIZE
    # an unknown method
    for bad in (2, -1, 7):
        assert dev(p, 8, 2, 8, p, 4, 0, bad, p, 4, None) == ERR_RANGE
        assert uni(p, 8, 2, 8, 0.0, 1.0, 4, bad, p, 4, None) == ERR_RANGE
        assert host(p, 8, p, 4, bad, p) == ERR_RANGE
    # n >= 2^31, as the resampler
    big = 1 << 31
    assert dev(p, big, 1, big, p, 4, 0, LINEAR, p, 4, None) == ERR_SIZE
    assert uni(p, big, 1, big, 0.0, 1.0, 4, CUBIC, p, 4, None) == ERR_SIZE
    assert host(p, big, p, 4, LINEAR, p) == ERR_SIZE
    assert np.all(buf == 0)


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    import vvdsp_amd as vv
    L.vvhip_last_error.restype = C.c_char_p
    L.vvhip_set_error.argtypes = [C.c_char_p]
    x = row(257)
    for method in METHODS:
        for pos in (-1.0, 3.25, 1e30):                     # the end clamps are not answered on the CPU either
            L.vvhip_set_error(b"")
            st, v = api.one(method, x, pos)
            assert st == ERR_UNSUPPORTED and v == SENTINEL, (method, pos)
            assert b"no HIP device" in L.vvhip_last_error(), method
    pos = positions(257)[:64].copy()
    out = np.full(64, SENTINEL, np.float32)
    for m in (LINEAR, CUBIC):
        L.vvhip_set_error(b"")
        st = vv.lib().vv_dsp_interpolate_real_batch(x.ctypes.data, len(x), pos.ctypes.data, len(pos), m, out.ctypes.data)
        assert st == ERR_UNSUPPORTED and np.all(out == SENTINEL)
        assert b"no HIP device" in L.vvhip_last_error()
        L.vvhip_set_error(b"")
        assert vv.lib().vv_dsp_interpolate_device(x.ctypes.data, 257, 1, 257, pos.ctypes.data, 64, 0, m, out.ctypes.data,
                                                   64, None) == ERR_UNSUPPORTED
        assert vv.lib().vv_dsp_interpolate_uniform_device(x.ctypes.data, 257, 1, 257, 0.0, 0.5, 64, m, out.ctypes.data, 64,
                                                           None) == ERR_UNSUPPORTED
        assert np.all(out == SENTINEL) and b"no HIP device" in L.vvhip_last_error()


def test_resample_module_link_check(amd_lib_path):
    L = C.CDLL(amd_lib_path)
    assert L.vv_dsp_resample_dummy() == 3
    L.vvhip_interp_run_length.restype = C.c_size_t
    run = L.vvhip_interp_run_length()
    assert run >= 256 and run % 256 == 0


def test_interp_knob_and_counters():
    import vvdsp_amd as vv
    try:
        vv.debug_set("INTERP_ROWS", 1)
        assert vv.debug_get("INTERP_ROWS") == 1 and vv.debug_get("VVHIP_INTERP_ROWS") == 1
        vv.debug_clear("INTERP_ROWS")
        assert vv.debug_get("INTERP_ROWS") == -1
        for st in ("STAT_INTERP_ONE", "STAT_INTERP_ROWS"):
            vv.debug_clear(st)
            assert vv.debug_get(st) == 0
    finally:
        vv.debug_clear(None)


def test_binding_checks_without_gpu():
    """the checks of vvdsp_amd.interpolate / interpolate_uniform that need no device"""
    import torch
    import vvdsp_amd as vv
    x = torch.zeros((2, 8), dtype=torch.float32)
    pos = torch.zeros(4, dtype=torch.float32)
    for call in (lambda: vv.interpolate(x, pos),                                  # not device tensors
                 lambda: vv.interpolate_uniform(x, 0.0, 1.0, 4),
                 lambda: vv.interpolate(x, pos, method="quintic"),
                 lambda: vv.interpolate(x, pos, method=2),
                 lambda: vv.interpolate_uniform(x, 0.0, 1.0, 4, method=None),
                 lambda: vv.interpolate(x.double(), pos),
                 lambda: vv.interpolate(x, pos.double()),
                 lambda: vv.interpolate(x, torch.zeros((2, 2, 2))),
                 lambda: vv.interpolate(x[:, ::2], pos),                          # sample stride 2
                 lambda: vv.interpolate_uniform(x, 0.0, 1.0, -1)):
        with pytest.raises(vv.VvError):
            call()
    assert vv.interp_run_length() == vv.lib().vvhip_interp_run_length()


@pytest.mark.parametrize("compiler,flags", [("gcc", ["-std=c99"]), ("g++", [])])
def test_umbrella_header_compiles_alone(tmp_path, compiler, flags):
    if shutil.which(compiler) is None:
        pytest.fail(f"{compiler} not found")
    src = tmp_path / ("only_resample." + ("c" if compiler == "gcc" else "cpp"))
    src.write_text('#include "vv_dsp/resample.h"\nint main(void) { return vv_dsp_resample_dummy() == 3 ? 0 : 1; }\n')
    r = subprocess.run([compiler, *flags, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
