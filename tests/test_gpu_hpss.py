"""GPU tests of harmonic-percussive separation (include/vv_dsp/spectral/hpss.h) against
the numpy model of tests/median_util.py, bit for bit (uint32 patterns): the two medians
are selections and the masks are single f64 operations, so nothing is approximate.  The
signal form is held to the sequence of public calls that defines it, and the masks to
the separation they are for: on the tone-and-clicks fixture the numpy model alone keeps
0.9990 of the tone and 0.0134 of the clicks under the harmonic mask, 0.9828 of the
clicks and 0.0002 of the tone under the percussive one (test_median_host.py prints
them); the limits asserted here are 0.99 / 0.05 / 0.95 / 0.01."""
import ctypes as C

import numpy as np
import pytest
import torch

import median_util as mu

pytestmark = pytest.mark.gpu

POISON_IN, POISON_OUT = np.float32(np.inf), np.float32(-12345.0)
ALL = ("harm", "perc", "mask_harm", "mask_perc")
# (mask kind, margin_harm, margin_perc, magnitude): every kind, margins 1, 1.5 and 2, both weights
SETTINGS = ((mu.SOFT, 1.0, 1.0, 1), (mu.WIENER, 1.5, 2.0, 1), (mu.HARD, 2.0, 1.5, 0), (mu.WIENER, 1.0, 1.5, 0),
            (mu.SOFT, 2.0, 1.0, 0), (mu.HARD, 1.0, 1.0, 1))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def params(vv, n_fft, wh, wp, setting):
    kind, mh, mp, mag = setting
    return vv.HpssParams(n_fft, mag, wh, wp, mh, mp, kind)


def model(p, n_fft, wh, wp, setting, rpg=0):
    kind, mh, mp, mag = setting
    return mu.hpss_model(p, n_fft, mag, wh, wp, mh, mp, kind, rpg)


def same(got, want, what):
    for name in want:
        if name in got:
            g = got[name].cpu().numpy() if torch.is_tensor(got[name]) else got[name]
            assert np.array_equal(mu.bits(g), mu.bits(want[name])), (what, name)


@pytest.mark.parametrize("shape", mu.HPSS_SHAPES, ids=lambda s: "%dx%d" % s)
def test_planes_equal_the_model(vdev, shape):
    n_fft, T = shape
    p = mu.hpss_rows(n_fft, T, T)
    dp = dev(p)
    wins = mu.HPSS_WINDOWS + (((127, 127),) if T == 7 else ())
    i = 0
    for wh, wp in wins:
        for _ in range(2):
            setting = SETTINGS[i % len(SETTINGS)]
            i += 1
            got = vdev.hpss(dp, params(vdev, n_fft, wh, wp, setting), ALL)
            want = model(p, n_fft, wh, wp, setting)
            assert set(got) == set(ALL)
            same(got, want, (shape, wh, wp, setting))
            # the fixture's zero column: with windows of 1 both medians are zero there, a mask of 0.5
            if (wh, wp) == (1, 1) and n_fft > 2:
                assert setting[0] != mu.HARD
                for name in ("mask_harm", "mask_perc"):
                    assert np.all(got[name].cpu().numpy()[:, (n_fft // 2 + 1) // 2] == 0.5), (shape, name)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "k%d_%g_%g_m%d" % s)
def test_every_setting(vdev, setting):
    n_fft, T = 256, 28
    p = mu.hpss_rows(n_fft, T, 5)
    got = vdev.hpss(dev(p), params(vdev, n_fft, 9, 9, setting), ALL)
    same(got, model(p, n_fft, 9, 9, setting), setting)


def test_pitched_rows_and_poisoned_pads(vdev):
    """pitch 544 for K = 513 on both sides: the input pads hold +inf, which would change a
    frequency median if read; the output pads hold a sentinel that must survive"""
    n_fft, T, K, pitch = 1024, 200, 513, 544
    p = mu.hpss_rows(n_fft, T, 9)
    wide = np.full((T, pitch), POISON_IN, np.float32)
    wide[:, :K] = p
    L = vdev.lib()
    prm = params(vdev, n_fft, 31, 17, SETTINGS[1])
    planes = {name: torch.full((T, pitch), float(POISON_OUT), dtype=torch.float32, device="cuda") for name in ALL}
    out = vdev.HpssOut(*(planes[name].data_ptr() for name in ALL))
    dw = dev(wide)
    st = L.vv_dsp_hpss_device(C.c_void_p(dw.data_ptr()), T, pitch, 0, C.byref(prm), C.byref(out), pitch,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    want = model(p, n_fft, 31, 17, SETTINGS[1])
    for name in ALL:
        g = planes[name].cpu().numpy()
        assert np.array_equal(mu.bits(g[:, :K]), mu.bits(want[name])), name
        assert np.all(g[:, K:] == POISON_OUT), name
    # the binding's pitched view gives the same planes, packed
    same(vdev.hpss(dw[:, :K], prm, ALL), want, "pitched view")


def test_groups_two_full_and_a_short_one(vdev):
    n_fft, T = 64, 23
    p = mu.hpss_rows(n_fft, T, 11)
    prm = params(vdev, n_fft, 9, 9, SETTINGS[0])
    got = vdev.hpss(dev(p), prm, ALL, rows_per_group=9)
    want = model(p, n_fft, 9, 9, SETTINGS[0], 9)
    same(got, want, "groups of 9")
    assert not np.array_equal(mu.bits(want["harm"]), mu.bits(model(p, n_fft, 9, 9, SETTINGS[0])["harm"]))
    # a (ch, frames, K) tensor is one group per channel; a long group spans several runs of rows
    q = np.stack([mu.hpss_rows(n_fft, 150, s) for s in (1, 2)])
    got3 = vdev.hpss(dev(q), prm, ALL)
    for c in range(2):
        same({k: v[c] for k, v in got3.items()}, model(q[c], n_fft, 9, 9, SETTINGS[0]), ("channel", c))


def test_single_outputs_equal_the_planes_of_all(vdev):
    n_fft, T = 256, 28
    dp = dev(mu.hpss_rows(n_fft, T, 3))
    for setting in SETTINGS[:3]:
        prm = params(vdev, n_fft, 31, 17, setting)
        allp = vdev.hpss(dp, prm, ALL)
        for what in ALL + (("harm", "mask_perc"), ("perc", "mask_harm"), ("mask_harm", "mask_perc")):
            one = vdev.hpss(dp, prm, what)
            assert set(one) == set((what,) if isinstance(what, str) else what)
            for name in one:
                assert torch.equal(one[name].view(torch.int32), allp[name].view(torch.int32)), (setting, what, name)


def test_host_entry_equals_device_entry(vdev):
    L = vdev.lib()
    n_fft, T, K = 64, 7, 33
    p = mu.hpss_rows(n_fft, T, 2)
    for wins, setting in (((9, 9), SETTINGS[1]), ((127, 127), SETTINGS[0])):
        prm = params(vdev, n_fft, wins[0], wins[1], setting)
        host = {name: np.full((T, K), POISON_OUT, np.float32) for name in ALL}
        out = vdev.HpssOut(*(host[name].ctypes.data for name in ALL))
        assert L.vv_dsp_hpss(p.ctypes.data, T, C.byref(prm), C.byref(out)) == 0
        same(vdev.hpss(dev(p), prm, ALL), host, ("host", wins))
        same(host, model(p, n_fft, wins[0], wins[1], setting), ("host model", wins))
        # one plane alone: the others stay untouched
        h2 = np.full((T, K), POISON_OUT, np.float32)
        out2 = vdev.HpssOut(None, None, h2.ctypes.data, None)
        assert L.vv_dsp_hpss(p.ctypes.data, T, C.byref(prm), C.byref(out2)) == 0
        assert np.array_equal(mu.bits(h2), mu.bits(host["mask_harm"]))


# ---- the signal path ------------------------------------------------------------------
N_FFT, HOP = 256, 64


@pytest.fixture(scope="module")
def fixture_signal():
    tone, clicks, noise = mu.separation_signals()
    mix = (tone + clicks + noise).astype(np.float32)
    return tone, clicks, mix


def signal_params(vv):
    return vv.HpssParams(N_FFT, 1, 9, 9, 1.0, 1.0, mu.WIENER)


def by_public_calls(vv, st, sig):
    """(harm, perc) numpy (nch, out_len) of the definition's sequence of public calls"""
    nch, n = sig.shape
    T, K = st.frames(n), N_FFT // 2 + 1
    ln = (T - 1) * HOP + N_FFT
    masks = vv.hpss(st.power(sig), signal_params(vv), ("mask_harm", "mask_perc"))
    spec = st.spectrogram(sig, complex_out=True).cpu().numpy()              # (nch, T, n_fft) complex64
    fold = np.where(np.arange(N_FFT) < K, np.arange(N_FFT), N_FFT - np.arange(N_FFT))
    res = []
    for name in ("mask_harm", "mask_perc"):
        m = masks[name].cpu().numpy()[:, :, fold]                            # the mirror bin's mask
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
        res.append(y)
    return res


def test_signal_form_equals_the_public_calls(vdev, fixture_signal):
    mix = fixture_signal[2]
    buf = np.full((2, mu.SIG_N + 48), POISON_IN, np.float32)
    buf[0, :mu.SIG_N] = mix
    buf[1, :mu.SIG_N] = mix[::-1]
    sig = dev(buf)[:, :mu.SIG_N]                                             # ch_stride > N
    st = vdev.Stft(N_FFT, HOP, vdev.WIN_HANN)
    T = st.frames(mu.SIG_N)
    assert T == 29        # 1 + (2000 - 256 + 64) // 64: the last frame is zero-padded past the signal
    want_h, want_p = by_public_calls(vdev, st, sig.contiguous())
    prm = signal_params(vdev)
    h, p = st.hpss(sig, prm)
    assert h.shape == p.shape == (2, (T - 1) * HOP + N_FFT)
    assert np.array_equal(mu.bits(h.cpu().numpy()), mu.bits(want_h))
    assert np.array_equal(mu.bits(p.cpu().numpy()), mu.bits(want_p))
    # either output alone, and one channel per group
    h1, none = st.hpss(sig, prm, perc=False)
    assert none is None and torch.equal(h1.view(torch.int32), h.view(torch.int32))
    none, p1 = st.hpss(sig, prm, harm=False)
    assert none is None and torch.equal(p1.view(torch.int32), p.view(torch.int32))
    with vdev.knobs(HPSS_GROUP=1):
        h2, p2 = st.hpss(sig, prm)
    assert torch.equal(h2.view(torch.int32), h.view(torch.int32))
    assert torch.equal(p2.view(torch.int32), p.view(torch.int32))
    # one channel, (n,) in and out
    h3, p3 = st.hpss(sig[0].contiguous(), prm)
    assert h3.dim() == 1 and torch.equal(h3.view(torch.int32), h[0].view(torch.int32))
    assert torch.equal(p3.view(torch.int32), p[0].view(torch.int32))
    # the parts do what they are for: the tone is in the harmonic signal, the clicks in the other
    tone, clicks = (a.astype(np.float64) for a in fixture_signal[:2])
    hp, pp = (a.cpu().numpy()[0, :mu.SIG_N].astype(np.float64) for a in (h, p))
    print("projections: harm on tone %.4f, perc on clicks %.4f" % (hp @ tone / (tone @ tone),
                                                                  pp @ clicks / (clicks @ clicks)))
    assert hp @ tone / (tone @ tone) > 0.9 and pp @ clicks / (clicks @ clicks) > 0.7


def test_signal_form_checks(vdev):
    st = vdev.Stft(N_FFT, HOP, vdev.WIN_HANN)
    L = vdev.lib()
    x = torch.zeros((2, 1000), dtype=torch.float32, device="cuda")
    T = st.frames(1000)
    ln = (T - 1) * HOP + N_FFT
    y = torch.zeros((2, ln), dtype=torch.float32, device="cuda")
    xp, yp, s = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = C.c_size_t(77)
    good = signal_params(vdev)
    call = lambda prm, n, nch, cs, os_: L.vv_dsp_stft_hpss_device(st.h, C.byref(prm), xp, n, nch, cs, yp, yp, os_, s,
                                                                  C.byref(got))
    assert call(vdev.HpssParams(128, 1, 9, 9, 1.0, 1.0, 2), 1000, 2, 1000, ln) == mu.ERR_SIZE    # not the handle's size
    assert call(vdev.HpssParams(N_FFT, 1, 8, 9, 1.0, 1.0, 2), 1000, 2, 999, ln) == mu.ERR_SIZE   # stride before window
    assert call(good, 1000, 1, 0, ln - 1) == mu.ERR_SIZE                                         # one channel too
    assert call(vdev.HpssParams(N_FFT, 1, 8, 9, 1.0, 1.0, 2), 1000, 2, 1000, ln) == mu.ERR_RANGE
    assert call(vdev.HpssParams(N_FFT, 1, 9, 129, 1.0, 1.0, 2), 1000, 2, 1000, ln) == mu.ERR_UNSUPPORTED
    assert got.value == 77
    assert call(good, 1000, 0, 1000, ln) == mu.OK and got.value == ln
    # a signal shorter than one frame is one zero-padded frame
    h, p = st.hpss(x[0, :100].contiguous(), good)
    assert h.shape == (N_FFT,) and torch.all(h == 0) and torch.all(p == 0)


def test_masks_separate_tone_and_clicks(vdev, fixture_signal):
    tone, clicks, mix = fixture_signal
    st = vdev.Stft(N_FFT, HOP, vdev.WIN_HANN)
    m = vdev.hpss(st.power(dev(mix)), signal_params(vdev), ("mask_harm", "mask_perc"))
    mh, mp = m["mask_harm"].cpu().numpy(), m["mask_perc"].cpu().numpy()
    stone, sclicks = mu.stft64(tone), mu.stft64(clicks)
    got = (mu.kept(mh, stone), mu.kept(mh, sclicks), mu.kept(mp, sclicks), mu.kept(mp, stone))
    print("kept: harm/tone %.4f harm/clicks %.4f perc/clicks %.4f perc/tone %.4f" % got)
    assert got[0] >= 0.99 and got[1] <= 0.05
    assert got[2] >= 0.95 and got[3] <= 0.01
