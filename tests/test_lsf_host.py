"""CPU tests of the LSF front-end (include/vv_dsp/envelope/lsf.h): the two forms of
the numpy model (tests/lsf_util.py) against each other, bit for bit, on every
case the GPU tests run; the model against independent truth (np.roots); the
grid; the argument checks in the header's order; and -- with no GPU --
UNSUPPORTED instead of a CPU computation."""
import ctypes as C
import math

import numpy as np
import pytest

import lsf_util as lu
from lsf_util import OK, ERR_NULL, ERR_SIZE, ERR_UNSUPPORTED, LsfApi, SENT


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return LsfApi(amd_lib_path)


@pytest.fixture(scope="module")
def table():
    """order -> (names, rows [B, order + 1], vectorised model outputs)"""
    x = lu.grid()
    out = {}
    for p in lu.ORDERS:
        cs = lu.cases(p)
        names = list(cs)
        A = np.stack([cs[n] for n in names])
        lsf, rc, flags = lu.lpc_to_lsf_vec(A, x)
        out[p] = (names, A, lsf, rc, flags, lu.lsf_to_lpc_vec(lsf))
    return out


def test_grid_and_constant():
    assert lu.header_cg() == math.cos(math.pi / 256)          # the nearest double (this libm and numpy agree on it)
    assert lu.header_cg() == float(np.cos(np.float64(np.pi) / 256))
    x = lu.grid()
    assert x[0] == 1.0 and x[lu.G] == -1.0 and np.all(np.diff(x) < 0)
    # the issue's figure: 5.6e-13 against cos(pi i / G)
    assert np.abs(x - np.cos(np.pi * np.arange(lu.G + 1) / lu.G)).max() < 5.7e-13


@pytest.mark.parametrize("p", lu.ORDERS)
def test_model_forms_agree(table, p):
    """row-wise == vectorised, bit for bit, NaN fills included, on the whole case table"""
    names, A, lsf, rc, flags, back = table[p]
    x = lu.grid()
    for r, n in enumerate(names):
        l, k, f = lu.lpc_to_lsf_row(A[r], x)
        assert np.array_equal(lu.bits(l), lu.bits(lsf[r])), (p, n)
        assert np.array_equal(lu.bits(k), lu.bits(rc[r])), (p, n)
        assert f == flags[r], (p, n)
        assert np.array_equal(lu.bits(lu.lsf_to_lpc_row(l)), lu.bits(back[r])), (p, n)


def test_special_rows(table):
    for p in lu.ORDERS:
        names, A, lsf, rc, flags, back = table[p]
        row = dict(zip(names, range(len(names))))
        # A = 1: uniform LSFs at even and odd order, rc = 0, and the way back gives A = 1
        u = row["unit"]
        assert flags[u] == lu.STABLE | lu.COMPLETE
        assert np.abs(lsf[u].astype(np.float64) - np.pi * np.arange(1, p + 1) / (p + 1)).max() < 1e-6
        assert np.all(rc[u] == 0.0) and np.abs(back[u] - A[u]).max() < 1e-6
        # a root outside the unit circle: not stable
        assert not flags[row["outside"]] & lu.STABLE
        # NaN / Inf rows: not stable; rc keeps k where the recursion stopped, quiet NaN below
        for n in ("nan", "inf"):
            r = row[n]
            assert not flags[r] & lu.STABLE
            stop = max(m for m in range(1, p + 1) if not abs(rc[r][m - 1]) < 1.0)
            assert np.all(lu.bits(rc[r])[:stop - 1] == 0x7FC00000)
            assert not np.any(lu.bits(rc[r]) == 0xFFC00000)   # a NaN k is stored as the quiet NaN
            if not flags[r] & lu.COMPLETE:
                assert np.all(lu.bits(lsf[r]) == 0x7FC00000)
        # neighbouring LSFs 1e-3 apart are resolved
        if "twotone" in row:
            t = row["twotone"]
            assert flags[t] == lu.STABLE | lu.COMPLETE
            d = np.diff(lsf[t].astype(np.float64))
            assert np.all(d > 0) and abs(d.min() - 1e-3) < 1e-5


def test_model_against_np_roots(table):
    """The model against independent truth on the ordinary rows (the LPC fixture's frames and the
    two-tone row), every order.  Measured on the CPU: LSF against the angles of np.roots(P) and
    np.roots(Q) 1.47e-12 rad; lsf_to_lpc(lpc_to_lsf(a)) against a 4.24e-6 (the float rounding of
    the LSFs); the bounds are 10x those.  STABLE equals max |np.roots(a)| < 1 on every such row."""
    x = lu.grid()
    gap_lsf = gap_back = 0.0
    for p in lu.ORDERS:
        names, A, lsf, rc, flags, back = table[p]
        for r, n in enumerate(names):
            if not lu.ordinary(n):
                continue
            info = {}
            lu.lpc_to_lsf_row(A[r], x, info)
            assert info["complete"], (p, n)
            a = A[r].astype(np.float64)
            ad = np.concatenate([a, [0.0]])
            ang = np.concatenate([np.angle(np.roots(ad + ad[::-1])), np.angle(np.roots(ad - ad[::-1]))])
            truth = np.sort(ang[(ang > 1e-9) & (ang < np.pi - 1e-9)])
            assert len(truth) == p, (p, n)
            mine = np.sort(np.concatenate([np.arccos(info["u"]), np.arccos(info["v"])]))
            gap_lsf = max(gap_lsf, np.abs(mine - truth).max())
            gap_back = max(gap_back, np.abs(back[r].astype(np.float64) - a).max())
            assert bool(flags[r] & lu.STABLE) == bool(np.abs(np.roots(a)).max() < 1.0), (p, n)
            # decidability: no sign class at a bracket's grid points hangs on a zero
            assert min(info["ends"]) > 0.0, (p, n)
    print(f"lsf gap {gap_lsf:.3e} rad, round trip {gap_back:.3e}")
    assert gap_lsf < 1.5e-11
    assert gap_back < 4.3e-5


def test_argument_rules_in_order(api):
    L = api.lib
    a = np.array([1.0, -0.5, 0.25], np.float32)
    big = np.zeros(40, np.float32)
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))
    buf, fl = np.zeros(40, np.float32), np.zeros(1, np.int32)
    # 1. NULL pointers and an all-NULL output set, whatever else is wrong
    assert L.vv_dsp_lpc_to_lsf(None, 0, fp(buf), fp(buf), ip(fl)) == ERR_NULL
    assert L.vv_dsp_lpc_to_lsf(fp(a), 99, None, None, None) == ERR_NULL
    assert L.vv_dsp_lsf_to_lpc(None, 0, fp(buf)) == ERR_NULL
    assert L.vv_dsp_lsf_to_lpc(fp(a), 99, None) == ERR_NULL
    # 2. order < 1: INVALID_SIZE
    st, lsf, rc, flags = api.lpc_to_lsf(a, order=0)
    assert st == ERR_SIZE and np.all(lsf == SENT) and np.all(rc == SENT) and flags[0] == -77
    assert api.lsf_to_lpc(a, order=0)[0] == ERR_SIZE
    # 4. order > 32: UNSUPPORTED, outputs untouched
    st, lsf, rc, flags = api.lpc_to_lsf(big, order=33)
    assert st == ERR_UNSUPPORTED and np.all(lsf == SENT) and flags[0] == -77
    assert b"32" in L.vv_dsp_amd_last_error()
    assert api.lsf_to_lpc(big[:33], order=33)[0] == ERR_UNSUPPORTED
    # in range: reaches the device, or its absence
    assert api.lpc_to_lsf(a)[0] in (OK, ERR_UNSUPPORTED)
    assert api.lpc_to_lsf(big[:33])[0] in (OK, ERR_UNSUPPORTED)
    # the device forms, on dummy pointers that are never read
    p = a.ctypes.data
    dev, inv, frm = L.vv_dsp_lpc_to_lsf_device, L.vv_dsp_lsf_to_lpc_device, L.vv_dsp_lsf_frames_device
    assert dev(None, 2, 1, 3, p, p, p, None) == ERR_NULL
    assert dev(p, 0, 1, 0, None, None, None, None) == ERR_NULL            # pointers come first
    assert dev(p, 0, 1, 3, p, None, None, None) == ERR_SIZE
    assert dev(p, 2, 1, 2, p, None, None, None) == ERR_SIZE               # a pitch below order + 1
    assert dev(p, 33, 1, 33, p, None, None, None) == ERR_SIZE             # the pitch comes before the limit
    assert dev(p, 33, 1, 34, p, None, None, None) == ERR_UNSUPPORTED
    assert dev(p, 2, 0, 3, p, None, None, None) == OK                     # zero rows: nothing launched
    assert inv(None, 2, 1, p, 3, None) == ERR_NULL and inv(p, 2, 1, None, 3, None) == ERR_NULL
    assert inv(p, 0, 1, p, 3, None) == ERR_SIZE and inv(p, 2, 1, p, 2, None) == ERR_SIZE
    assert inv(p, 33, 1, p, 34, None) == ERR_UNSUPPORTED and inv(p, 2, 0, p, 3, None) == OK
    assert frm(None, 2000, 1, 2000, 400, 160, 0, None, 16, p, p, p, p, None) == ERR_NULL
    assert frm(p, 2000, 1, 2000, 0, 160, 0, None, 16, None, None, None, None, None) == ERR_NULL
    for frame, hop, order in ((0, 160, 16), (400, 0, 16), (400, 160, 0), (16, 160, 16)):
        assert frm(p, 2000, 1, 2000, frame, hop, 0, None, order, p, None, None, None, None) == ERR_SIZE
    assert frm(p, 2000, 1, 2000, 400, 160, 0, None, 33, p, None, None, None, None) == ERR_UNSUPPORTED
    assert frm(p, 300, 1, 300, 400, 160, 0, None, 16, p, None, None, None, None) == OK   # no frames


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    a = np.array([1.0, -0.5, 0.25], np.float32)
    st, lsf, rc, flags = api.lpc_to_lsf(a)
    assert st == ERR_UNSUPPORTED and np.all(lsf == SENT) and np.all(rc == SENT) and flags[0] == -77
    assert b"no HIP device" in L.vv_dsp_amd_last_error()
    st, back = api.lsf_to_lpc(a[:2])
    assert st == ERR_UNSUPPORTED and np.all(back == SENT)
    p = a.ctypes.data
    assert L.vv_dsp_lpc_to_lsf_device(p, 2, 1, 3, p, None, None, None) == ERR_UNSUPPORTED
    assert L.vv_dsp_lsf_to_lpc_device(p, 2, 1, p, 3, None) == ERR_UNSUPPORTED
    assert L.vv_dsp_lsf_frames_device(p, 2000, 1, 2000, 400, 160, 0, None, 16, p, None, None, None,
                                      None) == ERR_UNSUPPORTED


def test_knob_and_counters_registered():
    import vvdsp_amd as vv
    assert vv.debug_get("STAT_LSF") >= 0 and vv.debug_get("STAT_FORMANT") >= 0
    vv.debug_set("LSF_GROUP", 3)
    assert vv.debug_get("LSF_GROUP") == 3
    vv.debug_clear("LSF_GROUP")
