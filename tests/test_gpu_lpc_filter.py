"""The LPC residual and synthesis filters on the GPU
(include/vv_dsp/envelope/lpc_filter.h, csrc/hip/lpc_filter_kernels.hip) against
the numpy model of the definition (tests/lpc_filter_util.py; the CPU suite holds
its forms equal on the same case table).  The residual and the exact synthesis
are compared bit for bit, states included; the chunked synthesis against the
model's f64 values within the bound the CPU suite's D gives."""
import numpy as np
import pytest

import lpc_filter_util as fu
from frames_util import hamming

pytestmark = pytest.mark.gpu

POISON = np.float32(-7.0e7)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(arr, extra):
    """a device view of arr whose rows are `extra` floats further apart, the padding poisoned"""
    import torch
    arr = np.asarray(arr, np.float32)
    buf = torch.full(arr.shape[:-1] + (arr.shape[-1] + extra,), float(POISON), dtype=torch.float32, device="cuda")
    buf[..., :arr.shape[-1]] = dev(arr)
    return buf, buf[..., :arr.shape[-1]]


def run(vdev, which, d, inp=None, state=None, offset=None, gain=True, pad=None, out_is_in=False):
    """one call of lpc_residual / lpc_synth on a case's planes -> (out [nch, n], state [nch, p] or None)"""
    import torch
    c = d["case"]
    inp = (d["x"] if which == "residual" else d["exc"]) if inp is None else inp
    nch = inp.shape[0]
    pad = c["pad"] if pad is None else pad
    xbuf, xv = padded(inp, 5 if pad else 0)
    abuf, av = padded(d["a"][:1 if c["shared"] else nch], 4 if pad else 0)
    a = av[0] if c["shared"] else av
    g = gbuf = None
    if gain and d["gain"] is not None:
        gbuf, gv = padded(d["gain"][:1 if c["shared"] else nch], 2 if pad else 0)
        g = gv[0] if c["shared"] else gv
    state = d["state"] if state is None else state
    st = None if state is None else dev(np.array(state, np.float64)[:nch])
    obuf, ov = (xbuf, xv) if out_is_in else padded(np.full(inp.shape, POISON, np.float32), 3 if pad else 0)
    fn = vdev.lpc_residual if which == "residual" else vdev.lpc_synth
    fn(xv, a, c["seg_len"], c["offset"] if offset is None else offset, gain=g, state=st, out=ov)
    torch.cuda.synchronize()
    bufs = [(xbuf, inp.shape[-1]), (abuf, c["order"] + 1), (obuf, inp.shape[-1])]
    if gbuf is not None:
        bufs.append((gbuf, d["gain"].shape[-1]))
    for buf, width in bufs:
        assert np.all(buf[..., width:].cpu().numpy() == POISON), "padding written"
    if not out_is_in:
        assert np.array_equal(xv.cpu().numpy().view(np.uint32), inp.view(np.uint32)), "input written"
    return ov.cpu().numpy(), None if st is None else st.cpu().numpy()


@pytest.mark.parametrize("name", fu.CASE_IDS)
def test_residual_equals_the_model(vdev, name):
    d = fu.expected(name)
    vdev.debug_clear("STAT_LPC_RESIDUAL")
    e, st = run(vdev, "residual", d)
    assert vdev.debug_get("STAT_LPC_RESIDUAL") == 1
    fu.assert_bits(e, d["res"][0], name)
    if st is not None:
        fu.assert_bits(st, d["res"][1], (name, "state"))


@pytest.mark.parametrize("name", fu.CASE_IDS)
def test_exact_synthesis_equals_the_model(vdev, name):
    d = fu.expected(name)
    assert d["case"]["n"] <= fu.EXACT_MAX
    for k in ("STAT_LPC_SYNTH_EXACT", "STAT_LPC_SYNTH_CHUNKED"):
        vdev.debug_clear(k)
    y, st = run(vdev, "synth", d)
    assert vdev.debug_get("STAT_LPC_SYNTH_EXACT") == 1 and vdev.debug_get("STAT_LPC_SYNTH_CHUNKED") == 0
    fu.assert_bits(y, d["syn"][0], name)
    if st is not None:
        fu.assert_bits(st, d["syn"][2], (name, "state"))


def chunk_bound(Y, D):
    """per row: half a float ulp of Y + 8 D max |Y| of that row"""
    return fu.half_ulp32(Y) + 8.0 * D * np.abs(Y).max(axis=-1, keepdims=True)


@pytest.mark.parametrize("L", fu.CHUNKS)
@pytest.mark.parametrize("name", fu.CHUNK_IDS)
def test_chunked_synthesis_within_the_bound(vdev, knob, name, L):
    """|y_gpu - Y_model| <= half a float ulp of Y_model + 8 D max |Y_model|, Y_model the model's f64
    output and D the chunked model form's relative distance from the sequential one (CPU suite);
    at most 1 % of the floats differ from the model's.  Observed on the MI355X: 0 of 2400, 0 of 4800 and
    at most 1 of 7200 floats differed, as in the model's own chunked form."""
    d = fu.expected(name)
    D = fu.chunk_expected(name, L)["D"]
    y_m, Y_m, s_m = d["syn"]
    knob("LPC_SYNTH_CHUNK", L)
    for group in (0, 1):
        if group:
            knob("LPC_FILTER_GROUP", group)
        for k in ("STAT_LPC_SYNTH_EXACT", "STAT_LPC_SYNTH_CHUNKED"):
            vdev.debug_clear(k)
        y, st = run(vdev, "synth", d)
        assert vdev.debug_get("STAT_LPC_SYNTH_CHUNKED") == 1 and vdev.debug_get("STAT_LPC_SYNTH_EXACT") == 0
        gap = np.abs(y.astype(np.float64) - Y_m)
        differ = int(np.sum(fu.bits(y) != fu.bits(y_m)))
        print(f"{name} chunk {L} group {group}: D = {D:.3e}, worst gap / bound "
              f"{(gap / chunk_bound(Y_m, D)).max():.3f}, floats differing {differ} of {y.size}")
        assert np.all(gap <= chunk_bound(Y_m, D))
        assert differ <= 0.01 * y.size
        if st is not None:
            assert np.all(np.abs(st - s_m) <= 8.0 * D * np.abs(Y_m).max(axis=-1, keepdims=True))


@pytest.mark.parametrize("name", ("vowel65", "order32long", "o10s1"))
def test_split_with_state_equals_one_call(vdev, knob, name):
    """two pieces with the state carried and the offset advanced == one call: bit for bit for the
    residual and the exact synthesis, within the chunked bound on the chunked route"""
    d = fu.expected(name)
    c = d["case"]
    p, nch = c["order"], c["nch"]
    s0 = d["state"] if d["state"] is not None else np.zeros((nch, p))
    for which, whole in (("residual", d["res"]), ("synth", (d["syn"][0], d["syn"][2]))):
        inp = d["x"] if which == "residual" else d["exc"]
        for cut in (1, p - 1, 1001):
            o1, s1 = run(vdev, which, d, inp=inp[:, :cut], state=s0)
            o2, s2 = run(vdev, which, d, inp=inp[:, cut:], state=s1, offset=c["offset"] + cut)
            fu.assert_bits(np.concatenate([o1, o2], axis=1), whole[0], (name, which, cut))
            fu.assert_bits(s2, whole[1], (name, which, cut, "state"))


def test_split_on_the_chunked_route(vdev, knob):
    """the same with chunks of 64: within the chunked bound, D the CPU suite's figure for this case"""
    name, L, cut = "chunk_vowel3", 64, 1001
    d = fu.expected(name)
    c = d["case"]
    D = fu.chunk_expected(name, L)["D"]
    knob("LPC_SYNTH_CHUNK", L)
    _, Y_m, s_m = d["syn"]
    vdev.debug_clear("STAT_LPC_SYNTH_CHUNKED")
    o1, s1 = run(vdev, "synth", d, inp=d["exc"][:, :cut])
    o2, s2 = run(vdev, "synth", d, inp=d["exc"][:, cut:], state=s1, offset=c["offset"] + cut)
    assert vdev.debug_get("STAT_LPC_SYNTH_CHUNKED") == 2
    y = np.concatenate([o1, o2], axis=1).astype(np.float64)
    assert np.all(np.abs(y - Y_m) <= chunk_bound(Y_m, D))
    assert np.all(np.abs(s2 - s_m) <= 8.0 * D * np.abs(Y_m).max(axis=-1, keepdims=True))


@pytest.mark.parametrize("chunk", (0, 64))
def test_one_nan_in_the_excitation(vdev, knob, chunk):
    """the outputs before the NaN are unchanged, every output from it on is the quiet NaN"""
    d = dict(fu.expected("chunk_vowel"))
    at = 1234
    exc = d["exc"].copy()
    exc[0, at] = np.float32(np.nan)
    if chunk:
        knob("LPC_SYNTH_CHUNK", chunk)
    clean, _ = run(vdev, "synth", d)
    y, st = run(vdev, "synth", d, inp=exc)
    fu.assert_bits(y[:, :at], clean[:, :at], "before the NaN")
    assert np.all(fu.bits(y[:, at:]) == 0x7FC00000)
    assert np.all(np.isnan(st))
    # the residual: the p + 1 outputs that read the NaN, and no other
    x = d["x"].copy()
    x[0, at] = np.float32(np.nan)
    e_clean, _ = run(vdev, "residual", d)
    e, _ = run(vdev, "residual", d, inp=x)
    hit = np.zeros(x.shape, bool)
    hit[0, at:at + d["case"]["order"] + 1] = True
    assert np.all(fu.bits(e[hit]) == 0x7FC00000)
    fu.assert_bits(e[~hit], e_clean[~hit], "away from the NaN")


def test_rows_do_not_depend_on_the_batch(vdev, amd_lib_path):
    """a row's bits are the same at nch 1 and 65, with packed and pitched rows, and through the
    host-row call"""
    d = fu.expected("vowel65")
    c = d["case"]
    api = fu.LpcFilterApi(amd_lib_path)
    for which, inp, want in (("residual", d["x"], d["res"]), ("synth", d["exc"], (d["syn"][0], d["syn"][2]))):
        full = {pad: run(vdev, which, d, pad=pad) for pad in (False, True)}
        for pad in (False, True):
            fu.assert_bits(full[pad][0], want[0], (which, pad))
            fu.assert_bits(full[pad][1], want[1], (which, pad, "state"))
        for ch in (0, 1, 63, 64):
            one = dict(d, x=d["x"][ch:ch + 1], exc=d["exc"][ch:ch + 1], a=d["a"][ch:ch + 1])
            for pad in (False, True):
                o, s = run(vdev, which, one, state=d["state"][ch:ch + 1], pad=pad)
                fu.assert_bits(o[0], want[0][ch], (which, ch, pad))
                fu.assert_bits(s[0], want[1][ch], (which, ch, pad, "state"))
            st, o, s = api.run(which, inp[ch], d["a"][ch], c["seg_len"], c["offset"], state=d["state"][ch])
            assert st == 0
            fu.assert_bits(o, want[0][ch], (which, ch, "host"))
            fu.assert_bits(s, want[1][ch], (which, ch, "host state"))
    # the host call with a gain plane and no state
    g = fu.expected("vowel")
    st, o, s = api.run("synth", g["exc"][0], g["a"][0], 160, 80, gain=g["gain"][0])
    assert st == 0 and s is None
    fu.assert_bits(o, g["syn"][0][0], "host synth with gain")
    st, o, _ = api.run("residual", g["x"][0], g["a"][0], 160, 80, gain=g["gain"][0])
    assert st == 0
    fu.assert_bits(o, g["res"][0][0], "host residual with gain")


@pytest.mark.parametrize("chunk", (0, 100))
def test_synthesis_in_place(vdev, knob, chunk):
    d = fu.expected("chunk_vowel3")
    if chunk:
        knob("LPC_SYNTH_CHUNK", chunk)
    out, s_out = run(vdev, "synth", d)
    inplace, s_in = run(vdev, "synth", d, out_is_in=True)
    fu.assert_bits(inplace, out, "in place")
    fu.assert_bits(s_in, s_out, "in place, state")


@pytest.mark.parametrize("center", (False, True))
@pytest.mark.parametrize("windowed", (False, True))
def test_residual_frames_equal_the_two_calls(vdev, knob, center, windowed):
    """lpc_residual_frames == lpc_frames followed by lpc_residual, bit for bit, with the rows
    returned and with the rows in scratch, in channel groups of 1 and of all channels"""
    x = np.stack([fu.channel_signal(c) for c in range(3)])
    dx = dev(x)
    win = dev(hamming(400).astype(np.float32)) if windowed else None
    order, frame, hop = 16, 400, 160
    a, err = vdev.lpc_frames(dx, frame, hop, order, window=win, center=center)
    assert a.shape[1] == (15 if center else 13)
    want = vdev.lpc_residual(dx, a, hop, hop // 2 - (0 if center else frame // 2)).cpu().numpy()
    for group in (1, 5):
        knob("LPC_FILTER_GROUP", group)
        vdev.debug_clear("STAT_LPC_RESIDUAL")
        got = vdev.lpc_residual_frames(dx, frame, hop, order, window=win, center=center, what=("e", "a", "err"))
        assert vdev.debug_get("STAT_LPC_RESIDUAL") == 1          # the caller's rows: one group
        fu.assert_bits(got["e"].cpu().numpy(), want, ("rows returned", group))
        fu.assert_bits(got["a"].cpu().numpy(), a.cpu().numpy(), "a")
        fu.assert_bits(got["err"].cpu().numpy(), err.cpu().numpy(), "err")
        vdev.debug_clear("STAT_LPC_RESIDUAL")
        only = vdev.lpc_residual_frames(dx, frame, hop, order, window=win, center=center)
        assert vdev.debug_get("STAT_LPC_RESIDUAL") == (3 if group == 1 else 1)
        assert sorted(only) == ["e"]
        fu.assert_bits(only["e"].cpu().numpy(), want, ("rows in scratch", group))
    one = vdev.lpc_residual_frames(dx[0], frame, hop, order, window=win, center=center)["e"]
    fu.assert_bits(one.cpu().numpy(), want[0], "one channel")


def test_nothing_to_do_writes_nothing(vdev):
    import torch
    d = fu.expected("vowel")
    a = dev(d["a"][0])
    out = torch.full((1, 8), float(POISON), dtype=torch.float32, device="cuda")
    st = torch.ones((1, 16), dtype=torch.float64, device="cuda")
    for fn in (vdev.lpc_residual, vdev.lpc_synth):
        y = fn(out[:, :0], a, 160, state=st, out=out[:, :0])
        assert y.shape == (1, 0)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == POISON) and np.all(st.cpu().numpy() == 1.0)
    assert vdev.lpc_residual_frames(dev(np.zeros((2, 300), np.float32)), 400, 160, 16)["e"].shape == (2, 300)


def test_pitch_shift_keeps_the_formants(vdev):
    """The whole chain on the fixture's first half, ratio 1.25: the median f0 (pitch_frames) is
    within 3 % of 1.25 x the input's, and the medians of F1 and F2 (formant_frames) move by less
    than a quarter of what they move under the plain stretch-and-resample shift (which moves a
    formant by 0.25 F).  Sizes: LPC 400 / 160 order 16, vocoder 512 / 64; with these the numpy
    model chain (pvoc_util, interp_util, lpc_filter_util) moved F1 / F2 by 0.024 / 0.059 of the
    plain shift's 184 / 315 Hz, under one eighth.  Measured on the MI355X: f0 126.4 -> 158.5 Hz
    (158.0 wanted); F1 / F2 moved 9.4 / 11.2 Hz against 184 / 308 Hz, 0.05 and 0.04 of it."""
    import torch
    x = dev(fu.fixture()["signal"][:1200])
    ratio, n = 1.25, 1200
    st = vdev.Stft(512, 64)
    plain = vdev.interpolate_uniform(st.time_stretch(x, 1.0 / ratio), 0.0, ratio, n, method="cubic")
    shifted = vdev.pitch_shift_lpc(x, ratio, 400, 160, 16, 512, 64, window=dev(hamming(400).astype(np.float32)))
    assert shifted.shape == (n,) and bool(torch.isfinite(shifted).all())
    pp = vdev.PitchParams(16000.0, 80.0, 400.0, 0.15)
    fp = vdev.formant_params(16000.0)
    win = dev(hamming(400).astype(np.float32))

    def measure(sig):
        f0 = vdev.pitch_frames(sig, 512, 80, pp, "f0")["f0"].cpu().numpy()
        fr = vdev.formant_frames(sig, 400, 80, 16, fp, what="freq", window=win, center=True)["freq"].cpu().numpy()
        return float(np.median(f0[f0 > 0])), np.nanmedian(fr[:, :2].astype(np.float64), axis=0)

    (f_in, F_in), (f_pl, F_pl), (f_sh, F_sh) = measure(x), measure(plain), measure(shifted)
    move_pl, move_sh = np.abs(F_pl - F_in), np.abs(F_sh - F_in)
    print(f"f0 in {f_in:.1f} plain {f_pl:.1f} lpc {f_sh:.1f} Hz; F1 F2 in {F_in} plain {F_pl} lpc {F_sh}; "
          f"moved plain {move_pl} lpc {move_sh} ratio {move_sh / move_pl}")
    assert abs(f_sh - ratio * f_in) <= 0.03 * ratio * f_in
    assert np.all(move_pl > 0.1 * F_in)          # the plain shift does move them
    assert np.all(move_sh < 0.25 * move_pl)
