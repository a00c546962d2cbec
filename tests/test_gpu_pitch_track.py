"""f0 tracking over the YIN curves on the GPU (include/vv_dsp/features/pitch_track.h,
csrc/hip/pitch_track_kernels.hip) against the f64 model of the definition
(tests/track_util.py).  The definition has no sum whose order is free, so every
comparison is exact: lags, the bits of f0 and aperiodicity (NaN equal to NaN) and
the bits of the cost.  The cases are tu.CASES (the CPU suite runs the same cases
through both forms of the model): state counts around a lane, a wave and the
one-wave / workgroup switch, frame counts around the backtrace block, bands 0 to
beyond the state count, ties, NaN and +inf curves, zero costs."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pitch_util as pu
import track_util as tu

pytestmark = pytest.mark.gpu

POISON_F, POISON_I = np.float32(-7.0e7), 0x5A5A5A5A


def vv_params(vv, p):
    return vv.PitchTrackParams(*(getattr(p, f) for f, _ in p._fields_))


def run_device(vv, q3, p, what=("lag", "f0", "aperiodicity", "cost"), row_pad=0, ch_pad=0, out_pad=0):
    """vv_dsp_pitch_track_device on curves [nch][F][W] laid out with padded strides, the gaps
    poisoned; checks the gaps and the curves after the call; -> dict of [nch][F] planes, cost [nch]"""
    import torch
    q3 = np.asarray(q3, np.float32)
    nch, F, W = q3.shape
    row, ostr = W + row_pad, F + out_pad
    chs = F * row + ch_pad
    host = np.full(nch * chs, POISON_F, np.float32)
    for c in range(nch):
        host[c * chs:c * chs + F * row].reshape(F, row)[:, :W] = q3[c]
    dq = torch.from_numpy(host).cuda()
    planes = {"lag": torch.full((nch, ostr), POISON_I, dtype=torch.int32, device="cuda"),
              "f0": torch.full((nch, ostr), float(POISON_F), dtype=torch.float32, device="cuda"),
              "aperiodicity": torch.full((nch, ostr), float(POISON_F), dtype=torch.float32, device="cuda"),
              "cost": torch.full((nch,), float(POISON_F), dtype=torch.float64, device="cuda")}
    out = vv.PitchTrackOut(*(planes[k].data_ptr() if k in what else None for k in vv.TRACK_NAMES))
    tp = vv_params(vv, p)
    st = vv.lib().vv_dsp_pitch_track_device(C.c_void_p(dq.data_ptr()), F, nch, row, chs, C.byref(tp), C.byref(out),
                                            ostr, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, (st, vv.lib().vvhip_last_error())
    assert np.array_equal(dq.cpu().numpy().view(np.uint32), host.view(np.uint32)), "curves or their gaps written"
    res = {}
    for k, t in planes.items():
        a = t.cpu().numpy()
        if k not in what:
            assert np.all(a == (POISON_I if k == "lag" else POISON_F)), f"{k} written though not wanted"
            continue
        if k != "cost":
            assert np.all(a[:, F:] == (POISON_I if k == "lag" else POISON_F)), f"{k}: the gap between channels written"
            a = a[:, :F]
        res[k] = a.view(np.uint32) if k == "lag" else a
    return res


def assert_same(got, want, c=None, what=("lag", "f0", "aperiodicity", "cost")):
    """got: planes of run_device (channel c) or a model-shaped dict; want: the model"""
    for k in what:
        g = got[k] if c is None else got[k][c]
        if k == "lag":
            assert np.array_equal(g, want[k]), (k, np.flatnonzero(g != want[k])[:8])
        elif k == "cost":
            assert np.float64(g).view(np.uint64) == np.float64(want[k]).view(np.uint64), (k, g, want[k])
        else:
            gb, wb = np.asarray(g, np.float32).view(np.uint32), np.asarray(want[k], np.float32).view(np.uint32)
            nan = np.isnan(g) & np.isnan(want[k])
            assert np.array_equal(gb[~nan], wb[~nan]) and np.array_equal(np.isnan(g), np.isnan(want[k])), k


@pytest.mark.parametrize("i", range(len(tu.CASES)), ids=tu.CASE_IDS)
def test_cases_equal_the_model(vdev, i):
    q, p = tu.case_inputs(i)
    vdev.debug_clear("STAT_PITCH_TRACK")
    got = run_device(vdev, q[None], p)
    assert vdev.debug_get("STAT_PITCH_TRACK") == 1
    assert_same(got, tu.case_model(i), 0)


@pytest.mark.parametrize("S,F,B", [(2048, 6, 64), (4096, 4, 126), (4096, 31, 8)], ids=["S2048-B64", "S4096-B126", "S4096-F31"])
def test_the_stated_limits(vdev, S, F, B):
    """the sizes the header promises (2048 states with max_step 64) and its limits (4096 states,
    max_step 126: sixteen waves, both D vectors past 64 KiB of LDS, backtrace blocks of 14 frames),
    against the vectorised model (the scalar form would take minutes here)"""
    p = tu.tparams(20, 20 + S - 1, max_step=B)
    q = tu.curves(F, 20, 20 + S - 1, 77 + S + B, "nan" if B == 8 else "contour")
    assert_same(run_device(vdev, q[None], p), tu.model(q, p), 0)


@pytest.mark.parametrize("nch", [1, 5, 33])
def test_channels_and_padded_strides(vdev, nch):
    """channels of different cases' curves side by side, rows, channels and planes padded, the
    gaps poisoned: every channel equals its own model, whatever stands next to it"""
    S, F, tau_min = 129, 70, 20
    p = tu.tparams(tau_min, tau_min + S - 1)
    qs = [tu.curves(F, tau_min, tau_min + S - 1, 500 + (c % 5), "nan" if c % 5 == 4 else "contour") for c in range(nch)]
    models = [tu.model(qs[c], p) for c in range(min(nch, 5))]
    got = run_device(vdev, np.stack(qs), p, row_pad=3, ch_pad=11, out_pad=5)
    for c in range(nch):
        assert_same(got, models[c % 5], c)
    # and the grouping of channels changes nothing
    if nch > 1:
        with vdev.knobs(PTRACK_GROUP=2):
            vdev.debug_clear("STAT_PITCH_TRACK")
            again = run_device(vdev, np.stack(qs), p, row_pad=3, ch_pad=11, out_pad=5)
            assert vdev.debug_get("STAT_PITCH_TRACK") == (nch + 1) // 2
        for c in range(nch):
            assert_same(again, models[c % 5], c)


def test_every_subset_of_outputs_and_the_host_entry(vdev, amd_lib_path):
    i = tu.CASE_IDS.index("nan")
    q, p = tu.case_inputs(i)
    want = tu.case_model(i)
    names = ("lag", "f0", "aperiodicity", "cost")
    for n in range(1, 5):
        for what in itertools.combinations(names, n):
            assert_same(run_device(vdev, q[None], p, what=what), want, 0, what)
    api = tu.TrackApi(amd_lib_path)
    for what in (names, ("f0",), ("cost",), ("lag", "aperiodicity")):
        st, res = api.track(q, p, what=what)
        assert st == tu.OK
        assert_same({k: (res[k][0] if k == "cost" else res[k]) for k in what}, want, None, what)
        for k in names:
            if k not in what:
                assert np.all(res[k] == (987654321 if k == "lag" else -123.0))
    # host rows with a padded stride: only the curves go up
    wide = np.full((q.shape[0], q.shape[1] + 7), POISON_F, np.float32)
    wide[:, :q.shape[1]] = q
    st, res = api.track(wide, p)
    assert st == tu.OK
    assert_same({k: (res[k][0] if k == "cost" else res[k]) for k in names}, want)


@pytest.mark.parametrize("ci", [0, 6, 7], ids=[pu.CASE_IDS[i] for i in (0, 6, 7)])
def test_fused_entry_equals_the_two_calls(vdev, ci):
    """signal -> tracked planes (vv_dsp_pitch_track_frames_device) against pitch_frames (cmnd)
    followed by pitch_track, bit for bit, with the channel groups forced to one channel so that
    the fixture's two channels cross a group boundary; and against the model on the exported curves"""
    import torch
    frame, hop, lo, hi, center, win, thr = pu.CASES[ci][0]
    sig = torch.from_numpy(pu.signals()).cuda()
    w = None if win is None else torch.from_numpy(pu.hann(frame)).cuda()
    pp = vdev.PitchParams(pu.FS, lo, hi, thr)
    tp = vdev.pitch_track_params(pp, frame)
    cm = vdev.pitch_frames(sig, frame, hop, pp, ("cmnd",), window=w, center=bool(center))["cmnd"]
    two = vdev.pitch_track(cm, tp, vdev.TRACK_NAMES)
    for group in (None, 1):
        vdev.debug_clear("STAT_PITCH_TRACK")
        if group:
            with vdev.knobs(PTRACK_GROUP=group):
                one = vdev.pitch_track_frames(sig, frame, hop, pp, tp, vdev.TRACK_NAMES, window=w, center=bool(center))
        else:
            one = vdev.pitch_track_frames(sig, frame, hop, pp, tp, vdev.TRACK_NAMES, window=w, center=bool(center))
        torch.cuda.synchronize()
        assert vdev.debug_get("STAT_PITCH_TRACK") == (2 if group else 1)
        for k in vdev.TRACK_NAMES:
            a, b = one[k].cpu().numpy(), two[k].cpu().numpy()
            assert np.array_equal(a.view(np.uint64 if k == "cost" else np.uint32),
                                  b.view(np.uint64 if k == "cost" else np.uint32)), (k, group)
    curves = cm.cpu().numpy()
    mp = tu.TrackParams(*(getattr(tp, f) for f, _ in tp._fields_))
    for c in range(2):
        want = tu.model(curves[c], mp)
        got = {k: (two[k].cpu().numpy()[c].view(np.uint32) if k == "lag" else two[k].cpu().numpy()[c])
               for k in vdev.TRACK_NAMES}
        assert_same(got, want)


def test_behaviour_end_to_end(vdev):
    """the fixture through the fused entry on the GPU: the tracked lags equal the model run on the
    GPU's own exported curves (exact: the tracker reads float32 curves), and no frame clear of the
    gap is an octave off, none inside it voiced, none clear of it unvoiced"""
    import torch
    sig, f_true, gap = tu.behaviour_signal()
    b = tu.BEHAVIOUR
    d = torch.from_numpy(sig).cuda()
    pp = vdev.PitchParams(b["fs"], b["fmin"], b["fmax"], b["threshold"])
    tp = vdev.pitch_track_params(pp, b["frame"])
    got = vdev.pitch_track_frames(d, b["frame"], b["hop"], pp, tp, vdev.TRACK_NAMES)
    curves = vdev.pitch_frames(d, b["frame"], b["hop"], pp, ("cmnd",))["cmnd"].cpu().numpy()
    want = tu.model(curves, tu.TrackParams(*(getattr(tp, f) for f, _ in tp._fields_)))
    assert_same({k: (v.cpu().numpy().view(np.uint32) if k == "lag" else v.cpu().numpy()) for k, v in got.items()}, want)
    lag = got["lag"].cpu().numpy().astype(np.int64)
    period, clear, inside = tu.frame_truth(f_true, gap, b["frame"], b["hop"], b["fs"])
    ratio = np.where(lag > 0, lag / period, 1.0)
    assert np.count_nonzero((lag > 0) & clear & ((ratio > 1.5) | (ratio < 1.0 / 1.5))) == 0
    assert np.count_nonzero((lag > 0) & inside) == 0 and np.count_nonzero((lag == 0) & clear) == 0
    f0 = got["f0"].cpu().numpy()
    assert np.all((f0 > 0) == (lag > 0)) and np.all(np.abs(f0[clear] - b["fs"] / period[clear]) < 6.0)
