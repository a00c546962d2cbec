"""CPU tests of the LPC residual and synthesis filters
(include/vv_dsp/envelope/lpc_filter.h): the forms of the numpy model
(tests/lpc_filter_util.py) against each other on every case the GPU tests run;
the model against scipy.signal.lfilter where one row governs; the fixture's round
trip; the argument checks in the header's order; and -- with no GPU --
UNSUPPORTED instead of a CPU computation."""
import ctypes as C

import numpy as np
import pytest
from scipy.signal import lfilter

import lpc_filter_util as fu
from lpc_filter_util import OK, ERR_NULL, ERR_SIZE, ERR_UNSUPPORTED, LpcFilterApi, SENT


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return LpcFilterApi(amd_lib_path)


def test_fixture_is_what_its_script_writes():
    fix, made = fu.fixture(), fu.make_fixture()
    assert sorted(fix) == ["a", "gain", "signal"]
    assert fix["signal"].shape == (fu.FIX_N,) and fix["a"].shape == (fu.FIX_ROWS, 17) and fix["gain"].shape == (fu.FIX_ROWS,)
    assert np.array_equal(fix["signal"], made["signal"])
    # the rows go through np.dot sums: equal to rounding, not to the bit, on another BLAS
    assert np.abs(fix["a"] - made["a"]).max() < 1e-5
    assert np.all(fix["a"][:, 0] == 1.0) and np.all(fix["gain"] > 0)
    assert all(np.abs(np.roots(r.astype(np.float64))).max() < 1.0 for r in fix["a"])


@pytest.mark.parametrize("name", fu.CASE_IDS)
def test_residual_forms_agree(name):
    """sample by sample == vectorised, bit for bit, states included (two channels of the wide cases)"""
    d = fu.expected(name)
    c = d["case"]
    k = min(c["nch"], 2)
    a = d["a"] if c["shared"] else d["a"][:k]
    g = None if d["gain"] is None else d["gain"] if c["shared"] else d["gain"][:k]
    s = None if d["state"] is None else d["state"][:k]
    e, st = fu.residual_seq(d["x"][:k], a, c["seg_len"], c["offset"], g, s)
    fu.assert_bits(e, d["res"][0][:k], name)
    fu.assert_bits(st, d["res"][1][:k], (name, "state"))


def test_model_against_lfilter():
    """One governing row: the model is scipy's lfilter in f64, synthesis lfilter([g], a, e) and
    residual lfilter(a, [g], x), to 1e-12 of the peak (f64 sums of at most 33 terms on stable rows)."""
    seen = 0
    for name in fu.CASE_IDS:
        d = fu.expected(name)
        c = d["case"]
        rows = np.unique(fu.row_index(c["n"], c["seg_len"], c["offset"], c["frames"]))
        if len(rows) != 1 or d["state"] is not None:
            continue
        seen += 1
        f = rows[0]
        for ch in range(c["nch"]):
            a = d["a"][0 if c["shared"] else ch][f].astype(np.float64)
            a[0] = 1.0
            g = 1.0 if d["gain"] is None else float(d["gain"][0 if c["shared"] else ch][f])
            Y = lfilter([g], a, d["exc"][ch].astype(np.float64))
            assert np.abs(d["syn"][1][ch] - Y).max() <= 1e-12 * max(np.abs(Y).max(), 1e-300), name
            E = lfilter(a, [g], d["x"][ch].astype(np.float64))
            assert np.abs(d["res"][0][ch] - E.astype(np.float32)).max() <= 1e-12 * np.abs(E).max() + \
                fu.half_ulp32(E).max(), name
    # every row of the fixture, held for the whole signal
    fix = fu.fixture()
    for f in range(fu.FIX_ROWS):
        a = fix["a"][f].astype(np.float64)
        _, Y, _ = fu.synth_seq(fix["signal"], fix["a"][f:f + 1], 1, 0, fix["gain"][f:f + 1])
        ref = lfilter([float(fix["gain"][f])], a, fix["signal"].astype(np.float64))
        assert np.abs(Y[0] - ref).max() <= 1e-12 * np.abs(ref).max()
        seen += 1
    assert seen >= fu.FIX_ROWS + 2


@pytest.mark.parametrize("L", fu.CHUNKS)
@pytest.mark.parametrize("name", fu.CHUNK_IDS)
def test_chunked_form_against_sequential(name, L):
    """The three passes in numpy against the recursion.  Measured here: D between 2.6e-14 and
    2.7e-13 of the peak, and 0 or 1 of the case's 2400, 4800 or 7200 floats differ.  The GPU test reuses D."""
    r = fu.chunk_expected(name, L)
    d = fu.expected(name)
    print(f"{name} chunk {L}: D = {r['D']:.3e}, floats differing {r['differ']} of {d['syn'][0].size}")
    assert r["D"] < 1e-10
    assert r["differ"] <= 0.01 * d["syn"][0].size


def test_fixture_round_trip():
    """synth(residual(x)) against x through the fixture's own rows and gains.  The only loss is the
    rounding of e to float: the bound is 8 x the response of the filter to half an ulp of e at every
    sample.  Measured: error 2.1e-8 against a propagated half ulp of 3.2e-8 (peak of x: 0.5)."""
    fix = fu.fixture()
    x, a, g = fix["signal"], fix["a"], fix["gain"]
    e, _ = fu.residual_vec(x, a, fu.FIX_HOP, fu.FIX_HOP // 2, g)
    _, Y, _ = fu.synth_seq(e, a, fu.FIX_HOP, fu.FIX_HOP // 2, g)
    delta = fu.half_ulp32(e[0].astype(np.float64)).astype(np.float32)
    _, R, _ = fu.synth_seq(delta, a, fu.FIX_HOP, fu.FIX_HOP // 2, g)
    err, prop = np.abs(Y[0] - x.astype(np.float64)).max(), np.abs(R).max()
    print(f"round trip error {err:.3e}, propagated half ulp {prop:.3e}")
    assert err <= 8 * prop
    assert prop < 1e-6   # the bound itself is a float rounding, not a loose figure


def test_state_splits_the_model():
    """the model itself: one call == two pieces with the state carried and offset advanced"""
    d = fu.expected("vowel65")
    c = d["case"]
    x, a, s = d["exc"][:3], d["a"][:3], d["state"][:3]
    for cut in (1, 7, 1000):
        y1, _, s1 = fu.synth_seq(x[:, :cut], a, c["seg_len"], c["offset"], None, s)
        y2, _, s2 = fu.synth_seq(x[:, cut:], a, c["seg_len"], c["offset"] + cut, None, s1)
        fu.assert_bits(np.concatenate([y1, y2], axis=1), d["syn"][0][:3], cut)
        fu.assert_bits(s2, d["syn"][2][:3], (cut, "state"))
        e1, t1 = fu.residual_vec(x[:, :cut], a, c["seg_len"], c["offset"], None, s)
        e2, t2 = fu.residual_vec(x[:, cut:], a, c["seg_len"], c["offset"] + cut, None, t1)
        whole = fu.residual_vec(x, a, c["seg_len"], c["offset"], None, s)
        fu.assert_bits(np.concatenate([e1, e2], axis=1), whole[0], (cut, "residual"))
        fu.assert_bits(t2, whole[1], (cut, "residual state"))


def test_argument_rules_in_order(api):
    L = api.lib
    x = np.linspace(-1, 1, 20).astype(np.float32)
    a = np.array([[1.0, -0.5, 0.25], [1.0, -0.4, 0.2]], np.float32)
    big = np.zeros((1, 34), np.float32)
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
    buf = np.full(20, SENT, np.float32)
    for which in ("residual", "synth"):
        fn = getattr(L, f"vv_dsp_lpc_{which}")
        # 1. NULL pointers, whatever else is wrong
        assert fn(None, 20, fp(a), 0, 0, 0, 0, None, None, fp(buf)) == ERR_NULL
        assert fn(fp(x), 20, None, 2, 2, 5, 0, None, None, fp(buf)) == ERR_NULL
        assert fn(fp(x), 20, fp(a), 99, 2, 0, 0, None, None, None) == ERR_NULL
        # 2. order < 1, seg_len == 0, frames == 0: INVALID_SIZE, before the order limit, outputs untouched
        for order, frames, seg in ((0, 2, 5), (2, 0, 5), (2, 2, 0), (33, 1, 0), (33, 0, 5)):
            st, out, _ = api.run(which, x, big if order == 33 else a, seg, order=order, frames=frames)
            assert st == ERR_SIZE and np.all(out == SENT), (which, order, frames, seg)
        # 3. order > 32: UNSUPPORTED
        st, out, s = api.run(which, x, big, 5, state=np.ones(33))
        assert st == ERR_UNSUPPORTED and np.all(out == SENT) and np.all(s == 1.0)
        assert b"32" in L.vv_dsp_amd_last_error()
        # 4. n == 0: OK, nothing written, the state untouched
        st, out, s = api.run(which, x, a, 5, state=np.ones(2), n=0)
        assert st == OK and np.all(out == SENT) and np.all(s == 1.0)
        # in range: reaches the device, or its absence
        assert api.run(which, x, a, 5)[0] in (OK, ERR_UNSUPPORTED)
        # the device form, on dummy pointers that are never read
        dev = getattr(L, f"vv_dsp_lpc_{which}_device")
        p = x.ctypes.data
        args = dict(x=p, n=20, nch=2, xs=20, a=p, order=2, frames=2, pitch=3, ach=6, g=None, gch=0, seg=5, off=0,
                    state=None, y=p, ys=20, stream=None)
        call = lambda **kw: dev(*{**args, **kw}.values())
        assert call(x=None) == ERR_NULL and call(a=None, order=0) == ERR_NULL and call(y=None, seg=0) == ERR_NULL
        for kw in (dict(order=0), dict(seg=0), dict(frames=0), dict(pitch=2), dict(ach=5), dict(xs=19), dict(ys=19),
                   dict(g=p, gch=1), dict(order=33, pitch=33)):
            assert call(**kw) == ERR_SIZE, (which, kw)
        assert call(order=33, pitch=34, ach=68) == ERR_UNSUPPORTED
        assert call(ach=0) in (OK, ERR_UNSUPPORTED) and call(g=p, gch=0) in (OK, ERR_UNSUPPORTED)
        assert call(n=0, xs=0, ys=0) == OK and call(nch=0) == OK   # nothing to do comes before the device
        assert call(order=33, pitch=34, ach=68, n=0) == ERR_UNSUPPORTED   # and after the order limit
    frm = L.vv_dsp_lpc_residual_frames_device
    p = x.ctypes.data
    assert frm(None, 2000, 1, 2000, 400, 160, 0, None, 16, None, 0, None, 0, p, 2000, None) == ERR_NULL
    assert frm(p, 2000, 1, 2000, 0, 160, 0, None, 16, None, 0, None, 0, None, 2000, None) == ERR_NULL
    for frame, hop, order in ((0, 160, 16), (400, 0, 16), (400, 160, 0), (16, 160, 16)):
        assert frm(p, 2000, 1, 2000, frame, hop, 0, None, order, None, 0, None, 0, p, 2000, None) == ERR_SIZE
    assert frm(p, 2000, 1, 2000, 400, 160, 0, None, 16, p, 16, None, 0, p, 2000, None) == ERR_SIZE   # a rows overlap
    assert frm(p, 2000, 1, 2000, 400, 160, 0, None, 16, None, 0, None, 0, p, 1999, None) == ERR_SIZE
    assert frm(p, 2000, 1, 2000, 400, 160, 0, None, 33, None, 0, None, 0, p, 2000, None) == ERR_UNSUPPORTED
    assert frm(p, 300, 1, 300, 400, 160, 0, None, 16, None, 0, None, 0, p, 300, None) == OK   # no frames


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    x = np.linspace(-1, 1, 20).astype(np.float32)
    a = np.array([[1.0, -0.5, 0.25]], np.float32)
    for which in ("residual", "synth"):
        st, out, s = api.run(which, x, a, 5, state=np.ones(2))
        assert st == ERR_UNSUPPORTED and np.all(out == SENT) and np.all(s == 1.0)
        assert b"no HIP device" in L.vv_dsp_amd_last_error()
        p = x.ctypes.data
        assert getattr(L, f"vv_dsp_lpc_{which}_device")(p, 20, 1, 20, p, 2, 1, 3, 0, None, 0, 5, 0, None, p, 20,
                                                        None) == ERR_UNSUPPORTED
    p = x.ctypes.data
    assert L.vv_dsp_lpc_residual_frames_device(p, 2000, 1, 2000, 400, 160, 0, None, 16, None, 0, None, 0, p, 2000,
                                               None) == ERR_UNSUPPORTED


def test_knob_and_counters_registered():
    import vvdsp_amd as vv
    for name in ("STAT_LPC_RESIDUAL", "STAT_LPC_SYNTH_EXACT", "STAT_LPC_SYNTH_CHUNKED"):
        assert vv.debug_get(name) >= 0
    for name in ("LPC_SYNTH_CHUNK", "LPC_FILTER_GROUP"):
        vv.debug_set(name, 3)
        assert vv.debug_get(name) == 3
        vv.debug_clear(name)
        assert vv.debug_get(name) == -1


def test_constants_match_the_header():
    import re
    import os
    with open(os.path.join(fu.ROOT, "include", "vv_dsp", "envelope", "lpc_filter.h")) as f:
        text = f.read()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))
    assert val("VV_DSP_LPC_FILTER_MAX_ORDER") == fu.MAX_ORDER
    assert val("VV_DSP_LPC_SYNTH_EXACT_MAX") == fu.EXACT_MAX
    assert val("VV_DSP_LPC_SYNTH_CHUNK") > 0
