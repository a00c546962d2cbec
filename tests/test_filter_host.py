"""CPU tests of the filter module's front-end (include/vv_dsp/filter.h, filter/iir.h,
filter/savgol.h): the Savitzky-Golay coefficient design bit for bit against the
rows recorded from the reference (tests/golden/savgol_coeffs.npz), argument
checks in the reference's order with its statuses, the float32 cascade model of
tests/filter_util.py against the reference's recorded outputs, a C program that
includes only the umbrella header, and -- with no GPU -- UNSUPPORTED instead of
a CPU computation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from filter_util import (FilterApi, Biquad, load, cascade_model, make_cascades, make_iir_signal, make_savgol_signal,
                         make_bad_row, savgol_model, savgol_lengths, IIR_N, IIR_CASCADES, SAVGOL_CASES, SAVGOL_MODES,
                         SENTINEL, OK, ERR_NULL, ERR_RANGE, ERR_UNSUPPORTED)


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return FilterApi(amd_lib_path)


def _coeffs(lib, m, p, deriv, delta):
    lib.vv_dsp_savgol_coeffs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
    h = np.full(max(m, 1), SENTINEL, np.float32)
    return lib.vv_dsp_savgol_coeffs(m, p, deriv, delta, h.ctypes.data), h


def test_savgol_coeffs_bit_identical_to_reference(api):
    want = load("savgol_coeffs")
    for i, (m, p, deriv, delta) in enumerate(SAVGOL_CASES):
        st, h = _coeffs(api.lib, m, p, deriv, delta)
        assert st == OK, (m, p, deriv, delta, st)
        assert np.array_equal(h, want[f"h{i}"]), (m, p, deriv, delta, np.abs(h - want[f"h{i}"]).max())


def test_savgol_coeffs_argument_checks(api):
    for args, want in (((5, 2, 0, 1.0), OK), ((4, 2, 0, 1.0), ERR_RANGE), ((0, 0, 0, 1.0), ERR_RANGE),
                       ((5, -1, 0, 1.0), ERR_RANGE), ((5, 2, -1, 1.0), ERR_RANGE), ((5, 2, 3, 1.0), ERR_RANGE),
                       ((5, 2, 1, 0.0), ERR_RANGE), ((5, 2, 0, 0.0), OK), ((259, 3, 0, 1.0), ERR_RANGE),
                       ((33, 16, 0, 1.0), ERR_RANGE), ((257, 15, 0, 1.0), OK)):
        assert _coeffs(api.lib, *args)[0] == want, args
    api.lib.vv_dsp_savgol_coeffs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
    assert api.lib.vv_dsp_savgol_coeffs(5, 2, 0, 1.0, None) == ERR_NULL


def test_fixture_inputs_are_reproducible():
    assert np.array_equal(make_iir_signal(), load("iir_signal")["x"])
    sg = load("savgol_signal")
    assert np.array_equal(make_savgol_signal(), sg["x"])
    assert np.array_equal(make_bad_row(sg["x"]), sg["bad"], equal_nan=True)
    ref = load("iir_ref")
    for name, sos in make_cascades().items():
        assert np.array_equal(sos, ref[name + "_sos"])


def test_float32_model_is_the_reference_bit_for_bit():
    """the model the GPU tests compare batched rows against reproduces the
    recorded reference outputs and final states"""
    x, ref = load("iir_signal")["x"], load("iir_ref")
    for name in IIR_CASCADES:
        y, z = cascade_model(ref[name + "_sos"], x[:IIR_N])
        assert np.array_equal(y, ref[name + "_y"]) and np.array_equal(z, ref[name + "_z"]), name


def test_savgol_model_is_the_reference_bit_for_bit():
    """the padding and convolution model the GPU tests compare batched rows
    against reproduces every recorded reference output"""
    x, coeffs = load("savgol_signal")["x"], load("savgol_coeffs")
    for mode in SAVGOL_MODES:
        rec = load(f"savgol_mode{mode}")
        for i, (m, _, _, _) in enumerate(SAVGOL_CASES):
            for n in savgol_lengths(m):
                assert np.array_equal(savgol_model(x[:n], coeffs[f"h{i}"], mode), rec[f"c{i}_n{n}"]), (mode, i, n)


def test_argument_cases_match_reference(api):
    for what, got in (("iir_ref", api.iir_argument_cases(device=False)),
                      ("savgol_misc", api.savgol_argument_cases(device=False))):
        rec = load(what)
        want = dict(zip((str(s) for s in rec["arg_names"]), (int(s) for s in rec["arg_status"])))
        assert len(got) >= 8
        for name, st in got.items():
            assert st == want[name], (what, name, st, want[name])


def test_device_entry_argument_checks_need_no_gpu(api):
    """vv_dsp_iir_apply_device / vv_dsp_savgol_device reject bad arguments before
    any device work (the pointers are host dummies, never read)"""
    L = api.lib
    vp, sz = C.c_void_p, C.c_size_t
    L.vv_dsp_iir_apply_device.argtypes = [vp, sz, vp, vp, vp, sz, sz, sz, sz, vp]
    L.vv_dsp_savgol_device.argtypes = [vp, sz, sz, sz, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, sz, vp]
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    assert L.vv_dsp_iir_apply_device(p, 1, None, None, p, 8, 1, 8, 8, None) == ERR_NULL
    assert L.vv_dsp_iir_apply_device(p, 1, None, p, None, 8, 1, 8, 8, None) == ERR_NULL
    assert L.vv_dsp_iir_apply_device(None, 1, None, p, p, 8, 1, 8, 8, None) == ERR_NULL
    assert L.vv_dsp_iir_apply_device(None, 0, None, p, p, 0, 1, 8, 8, None) == OK
    assert L.vv_dsp_savgol_device(None, 32, 1, 32, 5, 2, 0, 1.0, 0, p, 32, None) == ERR_NULL
    assert L.vv_dsp_savgol_device(p, 0, 1, 32, 5, 2, 0, 1.0, 0, p, 32, None) == 2
    assert L.vv_dsp_savgol_device(p, 32, 1, 32, 6, 2, 0, 1.0, 0, p, 32, None) == ERR_RANGE
    assert L.vv_dsp_savgol_device(p, 4, 1, 32, 5, 2, 0, 1.0, 0, p, 32, None) == 2
    assert L.vv_dsp_savgol_device(p, 32, 1, 32, 5, 2, 1, 0.0, 0, p, 32, None) == ERR_RANGE


def test_setters_and_dummy(api):
    L = api.lib
    bq = Biquad()
    bq.z1, bq.z2 = 3.0, 4.0
    assert L.vv_dsp_biquad_init(C.byref(bq), 1.0, 2.0, 3.0, 4.0, 5.0) == OK
    assert (bq.b0, bq.b1, bq.b2, bq.a1, bq.a2, bq.z1, bq.z2) == (1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 0.0)
    bq.z1, bq.z2 = 3.0, 4.0
    L.vv_dsp_biquad_reset(C.byref(bq))
    assert (bq.b0, bq.a2, bq.z1, bq.z2) == (1.0, 5.0, 0.0, 0.0)
    L.vv_dsp_biquad_reset(None)
    assert L.vv_dsp_filter_dummy() == int(load("iir_ref")["dummy"]) == 7


def test_iir_n0_touches_nothing(api):
    sos = make_cascades()["c"]
    bq = api.biquads(sos, state=[[0.25, -0.5]])
    y = np.full(4, SENTINEL, np.float32)
    fp = C.POINTER(C.c_float)
    assert api.lib.vv_dsp_iir_apply(C.byref(bq), 1, y.ctypes.data_as(fp), y.ctypes.data_as(fp), 0) == OK
    assert np.all(y == SENTINEL) and (bq[0].z1, bq[0].z2) == (0.25, -0.5)


UMBRELLA_C = r"""
#include "vv_dsp/filter.h"
int main(void) {
    vv_dsp_biquad bq;
    vv_dsp_real h[8], x[8] = {0}, y[8];
    vv_dsp_fir_state st;
    int bad = 0;
    bad += vv_dsp_biquad_init(&bq, 1, 0, 0, 0, 0) != VV_DSP_OK;                        /* filter/iir.h */
    bad += vv_dsp_fir_design_lowpass(h, 8, 0.25f, VV_DSP_WINDOW_HAMMING) != VV_DSP_OK; /* filter/fir.h */
    bad += vv_dsp_fir_state_init(&st, 0) != VV_DSP_ERROR_INVALID_SIZE;
    bad += vv_dsp_filtfilt_fir(0, 8, x, y, 8) != VV_DSP_ERROR_NULL_POINTER;            /* filter/common.h */
    bad += vv_dsp_savgol(x, 8, 4, 2, 0, 1, VV_DSP_SAVGOL_MODE_WRAP, y) != VV_DSP_ERROR_OUT_OF_RANGE; /* savgol.h */
    bad += vv_dsp_filter_dummy() != 7;
    return bad;
}
"""


def test_umbrella_header_compiles_and_links(amd_lib_path, tmp_path):
    src = tmp_path / "umbrella.c"
    src.write_text(UMBRELLA_C)
    exe = tmp_path / "umbrella"
    libdir = os.path.dirname(amd_lib_path)
    rocm_lib = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")   # the library's own dependencies
    cc = subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                         str(exe), "-L", libdir, "-lvvdsp_amd", f"-Wl,-rpath,{libdir}", f"-Wl,-rpath-link,{rocm_lib}",
                         f"-Wl,-rpath,{rocm_lib}"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    L.vvhip_last_error.restype = C.c_char_p
    L.vvhip_set_error.argtypes = [C.c_char_p]
    x = np.linspace(-1.0, 1.0, 64).astype(np.float32)
    sos = make_cascades()["a"]
    calls = {
        "iir_apply": lambda: api.iir(sos, x)[:2],
        "iir_apply_copy": lambda: api.iir(sos[:0], x)[:2],
        "savgol": lambda: api.savgol(x, 5, 2, 0, 1.0, 0),
    }
    for name, call in calls.items():
        L.vvhip_set_error(b"")
        st, y = call()
        assert st == ERR_UNSUPPORTED, name
        assert np.all(y == SENTINEL), name          # nothing computed on the CPU
        assert b"no HIP device" in L.vvhip_last_error(), name
    # one sample: NaN, the state untouched, the error text set
    bq = api.biquads(sos[:1], state=[[0.25, -0.5]])
    L.vvhip_set_error(b"")
    assert np.isnan(api.process(bq, 0.5))
    assert (bq[0].z1, bq[0].z2) == (0.25, -0.5)
    assert b"no HIP device" in L.vvhip_last_error()


def test_iir_knob_and_counters():
    import vvdsp_amd as vv
    try:
        for v in (0, 33, 1024):
            vv.debug_set("IIR_CHUNK", v)
            assert vv.debug_get("IIR_CHUNK") == v and vv.debug_get("VVHIP_IIR_CHUNK") == v
        vv.debug_clear("IIR_CHUNK")
        assert vv.debug_get("IIR_CHUNK") == -1
        for st in ("STAT_IIR_EXACT", "STAT_IIR_CHUNKED"):
            vv.debug_clear(st)
            assert vv.debug_get(st) == 0
    finally:
        vv.debug_clear(None)
