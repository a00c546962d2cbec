"""GPU tests of the one framed-row rule (frame_src.hpp) at the sizes where it can
go wrong: signals shorter than half a frame, so that centred frames reflect
past a whole period of 2 n (the far branch of reflect_index), and frames asked
for past the signal's end (zero padding at the tail).

Every case runs for statistics, LPC and pitch, and each fused entry point is
compared bit for bit with vv_dsp_fetch_frames_device followed by the row entry
point -- the assertion of the "is the pipeline" tests, at sizes those do not
reach.  Two channels ch_stride = n + 3 apart with NaN in the gap: a sample read
from the gap would show in every output.
"""
import ctypes as C

import numpy as np
import pytest

from frames_util import fetch_frames, hamming
from stats_util import valid_names

pytestmark = pytest.mark.gpu

OK = 0
PITCH_NAMES = ("f0", "aperiodicity", "lag", "cmnd")
PITCH_MIN_FRAME = 9          # sample_rate 16000, fmin 2000, fmax 8000: lags 2 .. 8
_vp, _sz = C.c_void_p, C.c_size_t


def two_channels(n):
    """(2, n) view of a (2, n + 3) buffer, NaN in the gap"""
    import torch
    x = np.random.default_rng(n).uniform(-1.0, 1.0, (2, n)).astype(np.float32)
    buf = torch.full((2, n + 3), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :n] = torch.from_numpy(x).cuda()
    return buf[:, :n]


def lpc_orders(frame):
    return (1, min(32, frame - 1))


def pitch_params(vdev):
    return vdev.PitchParams(16000.0, 2000.0, 8000.0, 0.15)


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rows_results(vdev, rows, frame):
    """the row entry points on gathered frames: {key: tensor}"""
    want = {("stats", k): v for k, v in vdev.stats(rows, valid_names(frame)).items()}
    for order in lpc_orders(frame):
        want[("lpc", order, "a")], want[("lpc", order, "err")] = vdev.lpc(rows, order)
    if frame >= PITCH_MIN_FRAME:
        want.update({("pitch", k): v for k, v in vdev.pitch(rows, pitch_params(vdev), PITCH_NAMES).items()})
    return want


def check(vdev, got, sig, frame, hop, center, win, frames=None):
    """got[key][c] against the row entry points on channel c's gathered frames"""
    for c in range(sig.shape[0]):
        rows = fetch_frames(vdev, sig[c].contiguous(), frame, hop, center, win, frames)
        want = rows_results(vdev, rows, frame)
        assert set(want) == set(got)
        for key in want:
            assert same(got[key][c], want[key]), (c, key)


def wrapper_results(vdev, sig, frame, hop, center, win):
    """the fused entry points through the binding: {key: (2, frames, ..) tensor}"""
    got = {("stats", k): v for k, v in
           vdev.stats_frames(sig, frame, hop, valid_names(frame), window=win, center=center).items()}
    for order in lpc_orders(frame):
        got[("lpc", order, "a")], got[("lpc", order, "err")] = vdev.lpc_frames(sig, frame, hop, order, window=win,
                                                                                 center=center)
    if frame >= PITCH_MIN_FRAME:
        got.update({("pitch", k): v for k, v in
                    vdev.pitch_frames(sig, frame, hop, pitch_params(vdev), PITCH_NAMES, window=win,
                                      center=center).items()})
    return got


@pytest.mark.parametrize("windowed", [0, 1])
@pytest.mark.parametrize("frame,hop", [(8, 3), (64, 64), (130, 7)])
@pytest.mark.parametrize("n", [1, 2, 5, 37])
def test_centred_frames_longer_than_the_signal(vdev, n, frame, hop, windowed):
    import torch
    sig = two_channels(n)
    assert sig.stride(0) == n + 3
    win = torch.from_numpy(hamming(frame)).cuda() if windowed else None
    fr = vdev.num_frames(n, frame, hop, True)
    assert fr >= 1
    got = wrapper_results(vdev, sig, frame, hop, True, win)
    assert all(v.shape[:2] == (2, fr) for v in got.values())
    check(vdev, got, sig, frame, hop, True, win)


@pytest.mark.parametrize("windowed", [0, 1])
def test_frames_past_the_end_are_zero_padded(vdev, windowed):
    """not centred: what num_frames gives through the binding, then two frames more at the C level"""
    import torch
    n, frame, hop = 37, 16, 5
    sig = two_channels(n)
    win = torch.from_numpy(hamming(frame)).cuda() if windowed else None
    fr = vdev.num_frames(n, frame, hop, False)
    assert fr == 5
    check(vdev, wrapper_results(vdev, sig, frame, hop, False, win), sig, frame, hop, False, win)

    more = fr + 2            # frame 5 covers samples 25 .. 40, frame 6 samples 30 .. 45 of 37
    assert (more - 1) * hop < n < (more - 2) * hop + frame
    L = vdev.lib()
    s = torch.cuda.current_stream().cuda_stream
    wp = None if win is None else win.data_ptr()
    head = (sig.data_ptr(), n, 2, n + 3, frame, hop, more, 0, wp)
    got = {}

    names = valid_names(frame)
    sout = vdev.StatsOut()
    for k in names:
        got[("stats", k)] = torch.empty((2, more), dtype=torch.int32 if k in vdev.STATS_COUNTS else torch.float32,
                                        device="cuda")
        setattr(sout, k, got[("stats", k)].data_ptr())
    L.vvhip_stats_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _vp, _sz, _vp]
    assert L.vvhip_stats_frames_device(*head, C.byref(sout), more, s) == OK

    L.vvhip_lpc_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _sz, _vp, _sz, _vp, _sz, _vp]
    for order in lpc_orders(frame):
        a = torch.empty((2, more, order + 1), dtype=torch.float32, device="cuda")
        err = torch.empty((2, more), dtype=torch.float32, device="cuda")
        assert L.vvhip_lpc_frames_device(*head, order, a.data_ptr(), more * (order + 1), err.data_ptr(), more, s) == OK
        got[("lpc", order, "a")], got[("lpc", order, "err")] = a, err

    p = pitch_params(vdev)
    _, tau_max, _ = vdev.pitch_lag_range(p, frame)
    pout = vdev.PitchOut()
    for k in PITCH_NAMES:
        got[("pitch", k)] = torch.empty((2, more, tau_max + 1) if k == "cmnd" else (2, more),
                                        dtype=torch.int32 if k == "lag" else torch.float32, device="cuda")
        setattr(pout, k, got[("pitch", k)].data_ptr())
    L.vvhip_pitch_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _vp, _vp, _sz, _sz, _vp]
    assert L.vvhip_pitch_frames_device(*head, C.byref(p), C.byref(pout), more, more * (tau_max + 1), s) == OK

    check(vdev, got, sig, frame, hop, False, win, frames=more)
