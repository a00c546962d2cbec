"""GPU tests of spectral noise suppression (include/vv_dsp/spectral/denoise.h) against the
numpy model of tests/denoise_util.py, bit for bit (uint32 patterns): the running mean is W
f64 adds in a fixed order, the floor a selection and the gain single f64 operations, so
nothing is approximate.  The signal form is held to the sequence of public calls that
defines it, and to what it is for: on the noisy-bursts fixture the float64 numpy chain
lifts the time-domain SNR from 14.70 dB to 22.02 dB (the test prints both), and the
library must lie within 0.1 dB of it.

K = n_fft // 2 + 1 with n_fft >= 2, so the narrowest row the library takes has two bins."""
import ctypes as C

import numpy as np
import pytest
import torch

import denoise_util as du
from denoise_util import bits

pytestmark = pytest.mark.gpu

POISON_IN, POISON_OUT = np.float32(np.inf), np.float32(-12345.0)
ALL = du.NAMES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def params(vv, c):
    return vv.DenoiseParams(c["n_fft"], c["W"], c["back"], c["ahead"], c["bias"], c["floor"], c["mode"])


def same(got, want, what):
    for name in want:
        if name in got:
            g = got[name].cpu().numpy() if torch.is_tensor(got[name]) else got[name]
            assert np.array_equal(bits(g), bits(want[name])), (what, name)


def launches(vv):
    return vv.debug_get("STAT_DENOISE")


@pytest.mark.parametrize("c", du.ALL_CASES, ids=du.case_id)
def test_planes_equal_the_model(vdev, c):
    """every shape and setting: with the segment length forced where the case forces it and
    with the knob unset, the direct and the blockwise minimum each forced, and the default"""
    p = du.case_rows(c)
    dp, prm = dev(p), params(vdev, c)
    want = du.denoise_model(p, *du.model_args(c))
    n0 = launches(vdev)
    runs = 0
    for seg in {c["seg"], 0}:
        for how in (0, 1, 2):
            knobs = {}
            if seg:
                knobs["DENOISE_SEGMENT"] = seg
            if how:
                knobs["DENOISE_MIN"] = how
            with vdev.knobs(**knobs):
                got = vdev.denoise(dp, prm, ALL, rows_per_group=c["rpg"])
            runs += 1
            assert set(got) == set(ALL)
            same(got, want, (seg, how))
    assert launches(vdev) - n0 == runs                       # one fused launch per call
    g = want["gain"]
    assert np.all(g >= np.float32(c["floor"])) and np.all(g <= 1)


def test_pitched_rows_and_poisoned_pads(vdev):
    """pitch 544 for K = 513 on both sides: the input pads hold +inf, which would reach the
    neighbouring tile's lanes if read; the output pads hold a sentinel that must survive"""
    n_fft, T, K, pitch = 1024, 150, 513, 544
    p = du.power_rows(n_fft, T, 9)
    wide = np.full((T, pitch), POISON_IN, np.float32)
    wide[:, :K] = p
    L = vdev.lib()
    prm = vdev.denoise_params(n_fft)
    planes = {name: torch.full((T, pitch), float(POISON_OUT), dtype=torch.float32, device="cuda") for name in ALL}
    out = vdev.DenoiseOut(*(planes[name].data_ptr() for name in ALL))
    dw = dev(wide)
    st = L.vv_dsp_denoise_device(C.c_void_p(dw.data_ptr()), T, pitch, 0, C.byref(prm), C.byref(out), pitch,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    want = du.denoise_model(p, n_fft, 8, 48, 48, 4.0, 0.1, du.WIENER)
    for name in ALL:
        g = planes[name].cpu().numpy()
        assert np.array_equal(bits(g[:, :K]), bits(want[name])), name
        assert np.all(g[:, K:] == POISON_OUT), name
    # the binding's pitched view and packed rows give the same planes
    same(vdev.denoise(dw[:, :K], prm, ALL), want, "pitched view")
    same(vdev.denoise(dev(p), prm, ALL), want, "packed")
    with vdev.knobs(DENOISE_SEGMENT=37):
        same(vdev.denoise(dw[:, :K], prm, ALL), want, "pitched view, seams every 37 rows")


def test_groups_two_full_and_a_short_one(vdev):
    n_fft, T = 64, 23
    p = du.power_rows(n_fft, T, 11)
    prm = vdev.DenoiseParams(n_fft, 8, 5, 3, 4.0, 0.1, du.SUBTRACT)
    args = (n_fft, 8, 5, 3, 4.0, 0.1, du.SUBTRACT)
    want = du.denoise_model(p, *args, 9)
    for seg in (0, 4):
        with vdev.knobs(**({"DENOISE_SEGMENT": seg} if seg else {})):
            same(vdev.denoise(dev(p), prm, ALL, rows_per_group=9), want, ("groups of 9", seg))
    whole = du.denoise_model(p, *args)
    assert not np.array_equal(bits(want["smooth"]), bits(whole["smooth"]))
    assert not np.array_equal(bits(want["noise"]), bits(whole["noise"]))
    # the rows of one group alone give the same bits
    for r0 in (0, 9, 18):
        alone = vdev.denoise(dev(p[r0:r0 + 9]), prm, ALL)
        same(alone, {k: v[r0:r0 + 9] for k, v in want.items()}, ("alone", r0))
    # a (ch, frames, K) tensor is one group per channel; a long group spans several segments
    q = np.stack([du.power_rows(n_fft, 300, s) for s in (1, 2)])
    got3 = vdev.denoise(dev(q), prm, ALL)
    for c in range(2):
        same({k: v[c] for k, v in got3.items()}, du.denoise_model(q[c], *args), ("channel", c))


@pytest.mark.parametrize("mode", (du.GATE, du.WIENER, du.SUBTRACT))
def test_hostile_powers(vdev, mode):
    p = du.hostile_rows(128, 40, 7)
    for floor, seg in ((0.0, 0), (0.1, 16)):
        prm = vdev.DenoiseParams(128, 8, 5, 3, 4.0, floor, mode)
        with vdev.knobs(**({"DENOISE_SEGMENT": seg} if seg else {})):
            got = vdev.denoise(dev(p), prm, ALL, rows_per_group=15)
        same(got, du.denoise_model(p, 128, 8, 5, 3, 4.0, floor, mode, 15), (mode, floor))
        g = got["gain"].cpu().numpy()
        assert not np.isnan(g).any() and g.min() >= np.float32(floor) and g.max() <= 1


def test_single_outputs_equal_the_planes_of_all(vdev):
    n_fft, T, K = 256, 70, 129
    dp = dev(du.power_rows(n_fft, T, 3))
    L = vdev.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for mode in (du.GATE, du.WIENER, du.SUBTRACT):
        prm = vdev.DenoiseParams(n_fft, 8, 12, 10, 4.0, 0.1, mode)
        allp = vdev.denoise(dp, prm, ALL)
        for what in ALL + (("smooth", "gain"), ("noise", "gain"), ("smooth", "noise")):
            names = (what,) if isinstance(what, str) else what
            # the planes that are not wanted stand next to the wanted ones and must stay as they are
            guard = torch.full((3, T, K), float(POISON_OUT), dtype=torch.float32, device="cuda")
            out = vdev.DenoiseOut(*(guard[i].data_ptr() if name in names else None for i, name in enumerate(ALL)))
            n0 = launches(vdev)
            assert L.vv_dsp_denoise_device(C.c_void_p(dp.data_ptr()), T, K, 0, C.byref(prm), C.byref(out), K, s) == 0
            assert launches(vdev) - n0 == 1
            for i, name in enumerate(ALL):
                if name in names:
                    assert torch.equal(guard[i].view(torch.int32), allp[name].view(torch.int32)), (mode, what, name)
                else:
                    assert torch.all(guard[i] == float(POISON_OUT)), (mode, what, name)
        n0 = launches(vdev)
        assert vdev.denoise(dp, prm, ()) == {} and launches(vdev) == n0       # nothing wanted: nothing launched


def test_host_entry_equals_device_entry(vdev):
    L = vdev.lib()
    n_fft, T, K = 64, 40, 33
    p = du.power_rows(n_fft, T, 2)
    for (W, back, ahead), mode in (((8, 5, 3), du.WIENER), ((64, 48, 48), du.SUBTRACT)):
        prm = vdev.DenoiseParams(n_fft, W, back, ahead, 4.0, 0.1, mode)
        host = {name: np.full((T, K), POISON_OUT, np.float32) for name in ALL}
        out = vdev.DenoiseOut(*(host[name].ctypes.data for name in ALL))
        assert L.vv_dsp_denoise(p.ctypes.data, T, C.byref(prm), C.byref(out)) == 0
        same(vdev.denoise(dev(p), prm, ALL), host, ("host", W))
        same(host, du.denoise_model(p, n_fft, W, back, ahead, 4.0, 0.1, mode), ("host model", W))
        # one plane alone: the others stay untouched
        g2 = np.full((T, K), POISON_OUT, np.float32)
        out2 = vdev.DenoiseOut(None, None, g2.ctypes.data)
        assert L.vv_dsp_denoise(p.ctypes.data, T, C.byref(prm), C.byref(out2)) == 0
        assert np.array_equal(bits(g2), bits(host["gain"]))


# ---- the signal path ------------------------------------------------------------------
N_FFT, HOP = du.N_FFT, du.HOP


@pytest.fixture(scope="module")
def fixture_signal():
    clean, noise = du.fixture_signal()
    return clean, (clean + noise).astype(np.float32)


def by_public_calls(vv, st, sig, prm):
    """numpy (nch, out_len) of the definition's sequence of public calls"""
    nch, n = sig.shape
    T, K = st.frames(n), N_FFT // 2 + 1
    ln = (T - 1) * HOP + N_FFT
    gain = vv.denoise(st.power(sig), prm, "gain")["gain"].cpu().numpy()
    spec = st.spectrogram(sig, complex_out=True).cpu().numpy()              # (nch, T, n_fft) complex64
    fold = np.where(np.arange(N_FFT) < K, np.arange(N_FFT), N_FFT - np.arange(N_FFT))
    m = gain[:, :, fold]                                                     # the mirror bin's gain
    rows = (spec.view(np.float32).reshape(nch, T, N_FFT, 2) * m[..., None]).astype(np.float32)
    rows = np.ascontiguousarray(rows).view(np.complex64).reshape(nch, T, N_FFT)
    y = np.zeros((nch, ln), np.float32)
    for c in range(nch):
        out = torch.zeros(ln, dtype=torch.float32, device="cuda")
        norm = torch.zeros(ln, dtype=torch.float32, device="cuda")
        st.reconstruct(dev(rows[c]), out, norm)
        o, w = out.cpu().numpy(), norm.cpu().numpy()
        with np.errstate(all="ignore"):
            y[c] = np.where(w > np.float32(1e-8), o / w, np.float32(0))
    return y


def test_signal_form_equals_the_public_calls(vdev, fixture_signal):
    mix = fixture_signal[1]
    n = 6000                                                                 # 90 frames: the window of 97 is clipped
    buf = np.full((3, n + 48), POISON_IN, np.float32)
    buf[0, :n] = mix[3000:3000 + n]
    buf[1, :n] = mix[20000:20000 + n][::-1]
    buf[2, :n] = mix[10000:10000 + n] * np.float32(0.5)
    sig = dev(buf)[:, :n]                                                    # ch_stride > n
    st = vdev.Stft(N_FFT, HOP, vdev.WIN_HANN)
    T = st.frames(n)
    for prm in (vdev.denoise_params(N_FFT), vdev.denoise_params(N_FFT, mode=du.SUBTRACT, back=20, ahead=0, floor=0.0)):
        want = by_public_calls(vdev, st, sig.contiguous(), prm)
        y = st.denoise(sig, prm)
        assert y.shape == (3, (T - 1) * HOP + N_FFT)
        assert np.array_equal(bits(y.cpu().numpy()), bits(want))
        for group in (1, 2):
            with vdev.knobs(DENOISE_GROUP=group):
                y2 = st.denoise(sig, prm)
            assert torch.equal(y2.view(torch.int32), y.view(torch.int32)), group
        # one channel, (n,) in and out
        y1 = st.denoise(sig[1].contiguous(), prm)
        assert y1.dim() == 1 and torch.equal(y1.view(torch.int32), y[1].view(torch.int32))
    # a signal shorter than one frame is one zero-padded frame
    short = sig[0, :100].contiguous()
    prm = vdev.denoise_params(N_FFT)
    ys = st.denoise(short, prm)
    assert ys.shape == (N_FFT,)
    assert np.array_equal(bits(ys.cpu().numpy()), bits(by_public_calls(vdev, st, short[None], prm)[0]))


def test_signal_form_checks(vdev):
    st = vdev.Stft(N_FFT, HOP, vdev.WIN_HANN)
    L = vdev.lib()
    x = torch.zeros((2, 1000), dtype=torch.float32, device="cuda")
    T = st.frames(1000)
    ln = (T - 1) * HOP + N_FFT
    y = torch.zeros((2, ln), dtype=torch.float32, device="cuda")
    xp, yp, s = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = C.c_size_t(77)
    good = vdev.denoise_params(N_FFT)
    call = lambda prm, n, nch, cs, os_: L.vv_dsp_stft_denoise_device(st.h, C.byref(prm), xp, n, nch, cs, yp, os_, s,
                                                                     C.byref(got))
    bad_w = vdev.denoise_params(N_FFT, smooth_len=0)
    assert call(vdev.denoise_params(128), 1000, 2, 1000, ln) == du.ERR_SIZE          # not the handle's size
    assert call(bad_w, 1000, 2, 999, ln) == du.ERR_SIZE                              # stride before smooth_len
    assert call(good, 1000, 1, 0, ln - 1) == du.ERR_SIZE                             # one channel too
    assert call(bad_w, 1000, 2, 1000, ln) == du.ERR_RANGE
    assert call(vdev.denoise_params(N_FFT, back=512, bias=0.0), 1000, 2, 1000, ln) == du.ERR_RANGE
    assert call(vdev.denoise_params(N_FFT, back=512), 1000, 2, 1000, ln) == du.ERR_UNSUPPORTED
    assert got.value == 77
    assert call(good, 1000, 0, 1000, ln) == du.OK and got.value == ln
    assert torch.all(y == 0)


def test_denoise_lifts_the_snr_of_the_fixture(vdev, fixture_signal):
    clean, mix = fixture_signal
    n = len(mix)
    st = vdev.Stft(N_FFT, HOP, vdev.WIN_HANN)
    prm = vdev.denoise_params(N_FFT)
    y = st.denoise(dev(mix), prm).cpu().numpy().astype(np.float64)
    # the same chain in float64 numpy: STFT, the model's gain of the float32 powers, overlap-add
    X = du.stft64(mix)
    gain = du.denoise_model((np.abs(X) ** 2).astype(np.float32), N_FFT, 8, 48, 48, 4.0, 0.1, du.WIENER)["gain"]
    y64, covered = du.istft64(X * gain)
    assert y.shape == y64.shape
    keep = covered & (np.arange(len(y64)) < n)               # norm is full and the clean part exists
    assert keep.sum() > n - 2 * N_FFT
    ref = np.zeros(len(y64))
    ref[:n] = clean
    noisy = np.zeros(len(y64))
    noisy[:n] = mix
    before, after, after64 = (du.snr_db(ref[keep], v[keep]) for v in (noisy, y, y64))
    print("time-domain snr %.2f dB -> %.2f dB (float64 numpy chain %.2f dB)" % (before, after, after64))
    assert after > before
    assert abs(after - after64) <= 0.1
