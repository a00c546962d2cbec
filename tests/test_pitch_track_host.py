"""CPU tests of the pitch-tracking front-end (include/vv_dsp/features/pitch_track.h):
the argument checks in the header's order, each reached with later arguments also
bad and with the outputs untouched; vv_dsp_pitch_track_params_default against
vv_dsp_pitch_lag_range; -- with no GPU -- UNSUPPORTED instead of a CPU
computation; the two forms of the f64 model (tests/track_util.py) against each
other on every case the GPU test runs; and the behaviour the tracker exists for,
on the model alone: plain YIN puts frames of the fixture an octave off, the
tracked path puts none."""
import ctypes as C

import numpy as np
import pytest

import pitch_util as pu
import track_util as tu
from track_util import OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_UNSUPPORTED, TrackApi, TrackOut, tparams


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return TrackApi(amd_lib_path)


def untouched(res):
    return (np.all(res["lag"] == 987654321) and np.all(res["f0"] == -123.0) and
            np.all(res["aperiodicity"] == -123.0) and res["cost"][0] == -123.0)


def bad_range():
    """name -> parameters that are OUT_OF_RANGE"""
    return {k: tu.TrackParams(*v) for k, v in tu.bad_range_fields().items()}


def test_argument_rules_in_order(api):
    q = np.zeros((6, 90), np.float32)
    good = tparams(20, 84)
    L = api.lib
    # 1. NULL pointers, whatever else is wrong
    out = TrackOut()
    assert L.vv_dsp_pitch_track(None, 6, 90, C.byref(good), C.byref(out)) == ERR_NULL
    assert L.vv_dsp_pitch_track(q.ctypes.data, 6, 90, None, C.byref(out)) == ERR_NULL
    assert L.vv_dsp_pitch_track(q.ctypes.data, 6, 90, C.byref(good), None) == ERR_NULL
    assert L.vv_dsp_pitch_track(None, 0, 3, C.byref(tparams(0, 0, lam=-1.0, max_step=999)), C.byref(out)) == ERR_NULL
    # 2. F == 0: OK, nothing written, before the parameters, the stride and the limits
    for p in (good, tparams(0, 0), tparams(20, 84, lam=float("nan")), tparams(20, 84, max_step=999)):
        st, res = api.track(q, p, frames=0, row_stride=3)
        assert st == OK and untouched(res)
    # 3. OUT_OF_RANGE before the stride and the limits
    bad = bad_range()
    assert len(bad) == 19
    for name, p in bad.items():
        for stride, step in ((90, 8), (3, 8), (90, 999), (3, 999)):
            p.max_step = step
            st, res = api.track(q, p, row_stride=stride)
            assert st == ERR_RANGE and untouched(res), (name, stride, step)
    # zero costs and lambda are in range (reaching the device, or its absence)
    st, _ = api.track(q, tparams(20, 84, lam=0.0, jump=0.0, switch=0.0, unvoiced=0.0))
    assert st in (OK, ERR_UNSUPPORTED)
    # 4. a row stride below tau_max + 1, before the limits
    for p in (good, tparams(20, 84, max_step=127), tparams(1, 5000)):
        st, res = api.track(q, p, row_stride=int(p.tau_max))
        assert st == ERR_SIZE and untouched(res)
    # 5. the kernel's limits: max_step 126 and 4096 states
    wide = np.zeros((2, 4200), np.float32)
    for p in (tparams(20, 84, max_step=127), tparams(1, 4097), tparams(100, 4196)):
        st, res = api.track(wide, p)
        assert st == ERR_UNSUPPORTED and untouched(res)
        assert b"126" in L.vv_dsp_amd_last_error()
    # 6. nothing wanted: OK, no device asked for
    st, res = api.track(q, good, what=())
    assert st == OK and untouched(res)
    st, res = api.track(wide, tparams(1, 4096, max_step=126), what=())          # the limits themselves are supported
    assert st == OK


def test_device_forms_check_before_any_device_work(amd_lib_path):
    """vv_dsp_pitch_track_device / _frames_device decide every argument rule before a
    device is needed (the pointers are host dummies or NULL, never read)."""
    import vvdsp_amd as vv
    L = vv.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    good = vv.PitchTrackParams(16000.0, 20, 84, 4.0, 0.5, 0.3, 0.35, 8)
    pg = vv.PitchParams(16000.0, 80.0, 400.0, 0.15)                 # lags 40 .. 200 on frames of 400
    tg = vv.pitch_track_params(pg, 400)
    none, full = vv.PitchTrackOut(), vv.PitchTrackOut(p, p, p, p)
    dev, frm = L.vv_dsp_pitch_track_device, L.vv_dsp_pitch_track_frames_device
    vv.debug_clear("STAT_PITCH_TRACK")
    vv.debug_clear("STAT_PITCH_WAVE")
    for out in (none, full):
        o = C.byref(out)
        assert dev(None, 6, 2, 85, 600, C.byref(good), o, 6, None) == ERR_NULL
        assert dev(p, 6, 2, 85, 600, None, o, 6, None) == ERR_NULL
        assert dev(p, 6, 2, 85, 600, C.byref(good), None, 6, None) == ERR_NULL
        assert dev(p, 0, 2, 3, 3, C.byref(vv.PitchTrackParams(0.0, 0, 0, -1.0, 0, 0, 0, 999)), o, 0, None) == OK
        for name, b in tu.bad_range_fields().items():
            bp = vv.PitchTrackParams(*b)
            assert dev(p, 6, 2, 3, 3, C.byref(bp), o, 0, None) == ERR_RANGE, name
            assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(pg), C.byref(bp), o, 0, None) == ERR_RANGE, name
        assert dev(p, 6, 2, 84, 600, C.byref(good), o, 6, None) == ERR_SIZE
        assert dev(p, 6, 2, 85, 5 * 85 + 84, C.byref(good), o, 6, None) == ERR_SIZE
        big = vv.PitchTrackParams(16000.0, 20, 84, 4.0, 0.5, 0.3, 0.35, 127)
        assert dev(p, 6, 2, 85, 600, C.byref(big), o, 6, None) == ERR_UNSUPPORTED
        assert dev(p, 6, 2, 84, 600, C.byref(big), o, 6, None) == ERR_SIZE             # the stride comes first
        assert frm(None, 6400, 2, 6400, 400, 160, 0, None, C.byref(pg), C.byref(tg), o, 38, None) == ERR_NULL
        assert frm(p, 6400, 2, 6400, 400, 160, 0, None, None, C.byref(tg), o, 38, None) == ERR_NULL
        assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(pg), None, o, 38, None) == ERR_NULL
        assert frm(p, 6400, 2, 6400, 400, 0, 0, None, C.byref(pg), C.byref(tg), o, 38, None) == ERR_SIZE
        assert frm(p, 6400, 2, 6400, 0, 160, 0, None, C.byref(pg), C.byref(tg), o, 38, None) == ERR_SIZE
        assert frm(p, 6400, 2, 6400, 200, 160, 0, None, C.byref(pg), C.byref(tg), o, 38, None) == ERR_SIZE   # W < 1
        assert frm(p, 6400, 2, 6399, 400, 160, 0, None, C.byref(pg), C.byref(tg), o, 38, None) == ERR_SIZE
        wide = vv.PitchTrackParams(16000.0, 40, 201, 4.0, 0.5, 0.3, 0.35, 8)           # past the curves' last lag
        assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(pg), C.byref(wide), o, 38, None) == ERR_SIZE
        tg127 = vv.pitch_track_params(pg, 400)
        tg127.max_step = 127
        assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(pg), C.byref(tg127), o, 38, None) == ERR_UNSUPPORTED
        assert frm(p, 300, 2, 300, 400, 160, 0, None, C.byref(pg), C.byref(tg127), o, 0, None) == OK   # no frames
    assert dev(p, 6, 2, 85, 600, C.byref(good), C.byref(full), 5, None) == ERR_SIZE
    assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(pg), C.byref(tg), C.byref(full), 37, None) == ERR_SIZE
    # nothing wanted, or no channel: OK, nothing launched
    assert dev(p, 6, 2, 85, 600, C.byref(good), C.byref(none), 0, None) == OK
    assert dev(p, 6, 0, 85, 600, C.byref(good), C.byref(full), 6, None) == OK
    assert frm(p, 6400, 2, 6400, 400, 160, 0, None, C.byref(pg), C.byref(tg), C.byref(none), 0, None) == OK
    assert np.all(buf == 0)
    assert vv.debug_get("STAT_PITCH_TRACK") == 0 and vv.debug_get("STAT_PITCH_WAVE") == 0


def test_params_default_against_lag_range(amd_lib_path):
    import vvdsp_amd as vv
    L = vv.lib()
    for (frame, hop, lo, hi, center, win, thr), (tau_min, tau_max, W) in pu.CASES:
        pp = vv.PitchParams(pu.FS, lo, hi, thr)
        assert vv.pitch_lag_range(pp, frame)[:2] == (tau_min, tau_max)
        tp = vv.pitch_track_params(pp, frame)
        assert (tp.sample_rate, tp.tau_min, tp.tau_max, tp.max_step) == (pu.FS, tau_min, tau_max, 8)
        want = [np.float32(v) for v in tu.DEFAULT_COSTS[:4]]
        assert [tp.lambda_, tp.jump_cost, tp.switch_cost, tp.unvoiced_cost] == want
    # vv_dsp_pitch_lag_range's checks and statuses, nothing written on failure
    tp = vv.PitchTrackParams(1.0, 2, 3, 4.0, 5.0, 6.0, 7.0, 9)
    good = vv.PitchParams(16000.0, 80.0, 400.0, 0.15)
    fn = L.vv_dsp_pitch_track_params_default
    assert fn(None, 400, C.byref(tp)) == ERR_NULL and fn(C.byref(good), 400, None) == ERR_NULL
    for pp, frame, want in ((good, 0, ERR_SIZE), (good, 200, ERR_SIZE), (good, 16385, ERR_UNSUPPORTED),
                            (vv.PitchParams(16000.0, 400.0, 80.0, 0.15), 400, ERR_RANGE)):
        assert fn(C.byref(pp), frame, C.byref(tp)) == want
        assert (tp.sample_rate, tp.tau_min, tp.tau_max, tp.lambda_, tp.max_step) == (1.0, 2, 3, 4.0, 9)
    with pytest.raises(vv.VvError):
        vv.pitch_track_params((16000.0, 80.0, 400.0, 0.15), 400)


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    L.vvhip_set_error.argtypes = [C.c_char_p]
    L.vvhip_set_error(b"")
    q, p = tu.case_inputs(0)
    st, res = api.track(q, p)
    assert st == ERR_UNSUPPORTED and untouched(res)                 # nothing computed on the CPU
    assert b"no HIP device" in L.vv_dsp_amd_last_error()
    # the device form, on dummy pointers that are never read
    out = TrackOut(q.ctypes.data, None, None, None)
    assert L.vv_dsp_pitch_track_device(q.ctypes.data, 2, 1, q.shape[1], 2 * q.shape[1], C.byref(p), C.byref(out), 2,
                                       None) == ERR_UNSUPPORTED


def test_knob_and_counter_registered():
    import vvdsp_amd as vv
    try:
        vv.debug_set("PTRACK_GROUP", 3)
        assert vv.debug_get("PTRACK_GROUP") == 3 and vv.debug_get("VVHIP_PTRACK_GROUP") == 3
        vv.debug_clear("PTRACK_GROUP")
        assert vv.debug_get("PTRACK_GROUP") == -1
        vv.debug_clear("STAT_PITCH_TRACK")
        assert vv.debug_get("STAT_PITCH_TRACK") == 0
    finally:
        vv.debug_clear(None)


def test_binding_checks_without_gpu():
    import torch
    import vvdsp_amd as vv
    pg = vv.PitchParams(16000.0, 80.0, 400.0, 0.15)
    tg = vv.pitch_track_params(pg, 400)
    assert vv.TRACK_NAMES == ("lag", "f0", "aperiodicity", "cost")
    q = torch.zeros((2, 10, 201), dtype=torch.float32)
    for call in (lambda: vv.pitch_track(q, tg, ("lag",)),                          # not a device tensor
                 lambda: vv.pitch_track_frames(torch.zeros(2, 6400), 400, 160, pg, tg, ("lag",)),
                 lambda: vv.pitch_track_frames(torch.zeros(2, 6400), 400, 0, pg, tg, ("lag",))):
        with pytest.raises(vv.VvError):
            call()


# ------------------------------------------------------------- the model
@pytest.mark.parametrize("i", range(len(tu.CASES)), ids=tu.CASE_IDS)
def test_the_two_forms_of_the_model_agree(i):
    """the vectorised form (+inf padding, codes) and the naive scalar form (clipped band,
    Python floats, predecessors as states) give the same bits: lags, f0, aperiodicity, cost"""
    q, p = tu.case_inputs(i)
    a, b = tu.case_model(i), tu.model_naive(q, p)
    assert tu.same(a, b), tu.CASE_IDS[i]
    name, S, F, B, kind, costs = tu.CASES[i]
    assert len(a["lag"]) == F and (p.tau_max - p.tau_min + 1, p.max_step) == (S, B)
    if kind == "contour" and F >= 40 and costs is None:
        assert 0 < np.count_nonzero(a["lag"]) < F                    # both kinds of state on the path


def test_ties_are_decided_by_the_stated_order():
    """hand-made ties: equal curves everywhere, so every comparison is between equal values"""
    q = np.full((4, 40), 0.25, np.float32)
    # voiced costs 0.25 a frame, unvoiced 0.25: the path starts from U and a voiced end must be
    # strictly smaller, so the path is unvoiced throughout
    r = tu.model(q, tparams(16, 39, lam=8.0, jump=0.5, switch=0.25, unvoiced=0.25, max_step=4))
    assert np.all(r["lag"] == 0) and r["cost"] == 1.0
    assert tu.same(r, tu.model_naive(q, tparams(16, 39, lam=8.0, jump=0.5, switch=0.25, unvoiced=0.25, max_step=4)))
    # unvoiced dearer: the voiced minimum is attained by every lag, the lowest is taken, and with
    # lambda 0 every band candidate ties: the first examined (tau - B, clipped) is the predecessor
    p = tparams(16, 39, lam=0.0, jump=0.5, switch=0.25, unvoiced=0.5, max_step=4)
    r = tu.model(q, p)
    assert list(r["lag"]) == [16, 16, 16, 16] and r["cost"] == 1.0
    assert tu.same(r, tu.model_naive(q, p))
    # a cheaper lag in the last frame only: reached by the band's first tying candidate each step
    q2 = q.copy()
    q2[3, 30] = 0.0
    r = tu.model(q2, p)
    assert list(r["lag"]) == [18, 22, 26, 30] and r["cost"] == 0.75
    assert tu.same(r, tu.model_naive(q2, p))


def test_behaviour_on_the_model():
    """the fixture: a glide whose fundamental fades under its second harmonic, with a gap of
    noise.  Plain YIN (pitch_util.model_rows) decides at least 10 voiced frames clear of the
    gap more than a factor 1.5 from the true period; the tracked path decides none so, no
    frame inside the gap voiced and no frame clear of it unvoiced."""
    sig, f_true, gap = tu.behaviour_signal()
    b = tu.BEHAVIOUR
    rows = pu.frames_of(sig, b["frame"], b["hop"], 0, None)
    m = pu.model_rows(rows, b["fmin"], b["fmax"], b["threshold"])
    tau_min, tau_max, _ = pu.lag_range(b["fs"], b["fmin"], b["fmax"], b["frame"])
    period, clear, inside = tu.frame_truth(f_true, gap, b["frame"], b["hop"], b["fs"])
    assert clear.sum() >= 60 and inside.sum() >= 3

    def off(lag):
        ratio = np.where(lag > 0, lag / period, 1.0)
        return (lag > 0) & clear & ((ratio > 1.5) | (ratio < 1.0 / 1.5))

    yin_lag = np.where(m["f0"] > 0, m["lag"], 0)
    r = tu.model(m["cmnd"], tparams(tau_min, tau_max))
    lag = r["lag"].astype(np.int64)
    print(f"yin: {int(off(yin_lag).sum())} of {int(((yin_lag > 0) & clear).sum())} voiced frames off; "
          f"tracked: {int(off(lag).sum())} off, {int(((lag > 0) & inside).sum())} voiced in the gap, "
          f"{int(((lag == 0) & clear).sum())} unvoiced clear of it")
    assert off(yin_lag).sum() >= 10
    assert off(lag).sum() == 0
    assert np.count_nonzero((lag > 0) & inside) == 0 and np.count_nonzero((lag == 0) & clear) == 0
