"""GPU tests of the phase vocoder (include/vv_dsp/spectral/phase_vocoder.h) against the
f64 model of tests/pvoc_util.py, under its rule: every component within 2^-23 m_j of
the model's float, exact zeros where m_j == 0, NaN where the model is NaN.

On an MI355X (2026-10-20) the 95 comparisons of this file (the 38 cases x 2 channels
of the table and the 20 non-finite ones included) hold 2,553,944 components: 2,553,938
are the model's float
exactly, 6 are within one ulp of m_j (2 in the n_fft 400, rate 1.5 case, 4 in the
T = 1 case), none outside.  The identity at step 1 returns 105,152 of 105,152 floats
bit-equal to the input.  The stretched sines: amplitude 0.999999 to 1.000000, residual
rms 1.2e-6 to 2.6e-4 (8.37 bins: 6.3e-5, 2.6e-4, 2.1e-4 at rates 0.5, 1.25, 2; 20.5
bins: 1.2e-6, 1.4e-6, 4.2e-5)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pvoc_util as pu
from pvoc_util import CASES, CASE_IDS, S

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(vv, D, n_fft, p_or_pos=None, uniform=None, **kw):
    """D (T, n_fft) or (nch, T, n_fft) numpy -> numpy rows through the binding"""
    if uniform is not None:
        out = vv.phase_vocoder(dev(D), n_fft, uniform[0], uniform[1], m=uniform[2], **kw)
    else:
        out = vv.phase_vocoder(dev(D), n_fft, pos=dev(p_or_pos), **kw)
    return out.cpu().numpy()


def run_case(vv, case, D):
    n_fft, T, kind, arg, m = case
    pos, p = pu.case_positions(case)
    got = run(vv, D, n_fft, pos, uniform=(arg[0], arg[1], m) if kind == "u" else None)
    return got, p


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case_table_against_the_model(vdev, i):
    case = CASES[i]
    n_fft, T = case[0], case[1]
    D = pu.noise_rows(T, n_fft, 100 + i, nch=2)
    vdev.debug_clear("STAT_PVOC_ROWS")
    got, p = run_case(vdev, case, D)
    assert vdev.debug_get("STAT_PVOC_ROWS") == 1
    assert got.shape == (2, case[4], n_fft)
    for c in range(2):
        pu.check(got[c], pu.model(D[c], n_fft, p), n_fft, CASE_IDS[i])


@pytest.mark.parametrize("n_fft,T", [(64, 70), (400, 33), (1024, 34), (2, 40)])
def test_identity_at_step_one(vdev, n_fft, T):
    """start 0, step 1: every output row is the input row's lower half and its mirror"""
    K = n_fft // 2 + 1
    D = pu.noise_rows(T, n_fft, 7)
    got = run(vdev, D, n_fft, None, uniform=(0.0, 1.0, T))
    want = np.zeros_like(D)
    want[:, :K] = D[:, :K]
    for k in range(1, K):
        if 2 * k < n_fft:
            want[:, n_fft - k] = np.conj(D[:, k])
    mdl = pu.model(D, n_fft, pu.uniform_positions(0.0, 1.0, T))
    assert np.array_equal(mdl["out"], want)
    pu.check(got, mdl, n_fft, f"identity n_fft {n_fft}")
    equal = int(np.sum(got.view(np.float32) == want.view(np.float32)))
    print(f"identity n_fft {n_fft}: {equal} of {2 * got.size} floats bit-equal to the input")


def test_independent_of_channels_strides_alignment_form_and_entry(vdev):
    vv = vdev
    n_fft, T, m, start, step = 64, 45, 2 * S + 5, 0.5, 0.625          # exact in float, and so is every position
    D = pu.noise_rows(T, n_fft, 21, nch=3)
    base = run(vv, D, n_fft, None, uniform=(start, step, m))
    # one channel at a time
    for c in range(3):
        assert np.array_equal(run(vv, D[c], n_fft, None, uniform=(start, step, m)), base[c])
    # channel strides padded with NaN that is never read; the output's pad words stay
    pad_in, pad_out = 37, 11
    big = torch.full((3, T * n_fft + pad_in), float("nan"), dtype=torch.complex64, device="cuda")
    spec = big.as_strided((3, T, n_fft), (T * n_fft + pad_in, n_fft, 1))
    spec.copy_(dev(D))
    canary = complex(pu.CANARY)
    obig = torch.full((3, m * n_fft + pad_out), canary, dtype=torch.complex64, device="cuda")
    out = obig.as_strided((3, m, n_fft), (m * n_fft + pad_out, n_fft, 1))
    assert vv.phase_vocoder(spec, n_fft, start, step, m=m, out=out) is out
    assert np.array_equal(out.cpu().numpy(), base)
    assert torch.all(obig[:, m * n_fft:] == canary)
    # buffers 8 bytes past a 16 byte boundary
    fin = torch.zeros(3 * T * n_fft + 1, dtype=torch.complex64, device="cuda")
    fout = torch.zeros(3 * m * n_fft + 1, dtype=torch.complex64, device="cuda")
    sin, sout = fin[1:].view(3, T, n_fft), fout[1:].view(3, m, n_fft)
    assert sin.data_ptr() % 16 == 8 and sout.data_ptr() % 16 == 8
    sin.copy_(dev(D))
    vv.phase_vocoder(sin, n_fft, start, step, m=m, out=sout)
    assert np.array_equal(sout.cpu().numpy(), base)
    # the curve form at the same positions
    p = pu.uniform_positions(start, step, m)
    pos = p.astype(np.float32)
    assert np.array_equal(pos.astype(np.float64), p)
    assert np.array_equal(run(vv, D, n_fft, pos), base)
    # the host form
    api = pu.PvocApi(vv.LIB_PATH)
    for c in range(3):
        st, hout = api.run(D[c], n_fft, start, step, m)
        assert st == pu.OK and np.array_equal(hout, base[c])
    pu.check(base[1], pu.model(D[1], n_fft, p), n_fft, "independence base")


NON_FINITE = [("rate0.5", 0.5), ("rate0.8", 0.8), ("rate2", 2.0), ("backwards", None)]


@pytest.mark.parametrize("name,rate", NON_FINITE, ids=[n for n, _ in NON_FINITE])
def test_non_finite_input_poisons_its_column_only(vdev, name, rate):
    """a NaN or an infinite bin of row t: both components of its column (and of the mirror
    column) are NaN from the first output row that uses row t -- as row t0 + 1 with
    0 < a < 1 (rate 0.8), with a == 0 (0.5), as row t0 (2, where odd rows are only ever
    row t0 + 1 and even rows row t0; the backwards curve) -- and nothing else changes"""
    n_fft, T = 64, 40
    D = pu.noise_rows(T, n_fft, 22)
    if rate is None:
        m = 2 * S + 3
        pos = pu.curve("backwards", T, m)
        p = pu.curve_positions(pos, T)
        kw = {"p_or_pos": pos}
    else:
        m = min(2 * S + 3, pu.stretch_rows(T, rate))
        p = pu.uniform_positions(0.0, rate, m)
        kw = {"p_or_pos": None, "uniform": (0.0, rate, m)}
    clean = run(vdev, D, n_fft, **kw)
    t0 = np.floor(p).astype(int)
    seen = set()
    for bad, (t, k) in ((np.nan, (9, 3)), (np.inf, (20, 0)), (-np.inf, (17, 32)), (np.inf, (12, 5)), (np.inf, (13, 7))):
        E = D.copy()
        E[t, k] = np.complex64(complex(bad, 1.0)) if k != 7 else np.complex64(complex(0.5, bad))
        got = run(vdev, E, n_fft, **kw)
        used = (t0 == t) | (t0 + 1 == t)
        assert used.any()
        first = int(np.argmax(used))
        seen.add(("t0" if t0[first] == t else "t1", bool(p[first] > t0[first])))
        cols = sorted({k, (n_fft - k) % n_fft})
        keep = [q for q in range(n_fft) if q not in cols]
        assert np.all(np.isnan(got[first:, cols].real)) and np.all(np.isnan(got[first:, cols].imag))
        assert np.array_equal(got[:first], clean[:first])
        assert np.array_equal(got[:, keep], clean[:, keep])
        pu.check(got, pu.model(E, n_fft, p), n_fft, f"non-finite {bad} in row {t}, {name}")
    print(f"non-finite {name}: first uses seen as (row, a > 0): {sorted(seen)}")
    want = {"rate0.5": ("t1", False), "rate0.8": ("t1", True), "rate2": ("t0", False), "backwards": ("t0", True)}[name]
    assert want in seen


PLANE_CASES = [i for i, c in enumerate(CASES) if c[0] in (64, 2) or c[2] == "c" or c[3] == (3.0, 0.5)]


def test_phase_plane_knob_gives_the_same_bits(vdev, knob):
    """knob PVOC_PLANE = 1 (the phases stored in an f64 plane instead of a second atan2) gives
    every bit of the default path, NaN columns included"""
    assert len(PLANE_CASES) >= 16
    for i in PLANE_CASES:
        case = CASES[i]
        D = pu.noise_rows(case[1], case[0], 300 + i, nch=2)
        D[0, case[1] // 2, 1] = np.complex64(complex(np.inf, 0.0))
        D[1, 0, 0] = 0
        want, _ = run_case(vdev, case, D)
        knob("PVOC_PLANE", 1)
        got, _ = run_case(vdev, case, D)
        knob("PVOC_PLANE", None)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), CASE_IDS[i]


def test_silence_in_the_middle(vdev):
    n_fft, T, rate = 64, 60, 0.8
    D = pu.noise_rows(T, n_fft, 23)
    D[20:35] = 0
    m = pu.stretch_rows(T, rate)
    p = pu.uniform_positions(0.0, rate, m)
    got = run(vdev, D, n_fft, None, uniform=(0.0, rate, m))
    t0 = np.floor(p).astype(int)
    silent = (t0 >= 20) & (t0 + 1 < 35)
    assert silent.sum() > 10
    assert np.all(got[silent].view(np.float32) == 0)
    assert np.all(np.isfinite(got.view(np.float32)))
    after = t0 >= 35
    assert np.all(np.abs(got[after][:, :n_fft // 2 + 1]) > 0)
    pu.check(got, pu.model(D, n_fft, p), n_fft, "silence")


def by_steps(vv, st, sig, rate):
    """spectrum -> vocoder -> reconstruct -> divide, through the public calls"""
    sig2 = sig if sig.dim() == 2 else sig.unsqueeze(0)
    nch, n = sig2.shape
    m, ln = st.time_stretch_length(n, rate)
    spec = st.spectrogram(sig2, complex_out=True)
    assert m == pu.stretch_rows(spec.shape[1], rate) and ln == (m - 1) * st.hop + st.nfft
    rows = vv.phase_vocoder(spec, st.nfft, 0.0, rate, m=m)
    y = np.zeros((nch, ln), np.float32)
    for c in range(nch):
        out = torch.zeros(ln, dtype=torch.float32, device="cuda")
        norm = torch.zeros(ln, dtype=torch.float32, device="cuda")
        st.reconstruct(rows[c], out, norm)
        o, w = out.cpu().numpy(), norm.cpu().numpy()
        with np.errstate(all="ignore"):
            y[c] = np.where(w > pu.NORM_FLOOR, o / w, np.float32(0))
    return y


@pytest.mark.parametrize("nfft,hop", [(256, 64), (400, 160)])
@pytest.mark.parametrize("nch", [1, 3])
def test_time_stretch_is_the_public_calls_in_sequence(vdev, knob, nfft, hop, nch):
    vv = vdev
    st = vv.Stft(nfft, hop)
    rng = np.random.default_rng(31)
    sig = dev(rng.uniform(-1, 1, (nch, 5000 + 13 * nch)).astype(np.float32))
    for rate in (0.8, 1.5):
        want = by_steps(vv, st, sig, rate)
        for group in (None, 1, 2):
            knob("PVOC_GROUP", group)
            got = st.time_stretch(sig, rate)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (rate, group)
        knob("PVOC_GROUP", None)
    # one row of samples in, one row out
    one = st.time_stretch(sig[0], 1.5)
    assert one.dim() == 1 and np.array_equal(one.cpu().numpy(), by_steps(vv, st, sig, 1.5)[0])


@pytest.mark.parametrize("bins", [8.37, 20.5])
@pytest.mark.parametrize("rate", [0.5, 1.25, 2.0])
def test_time_stretch_of_a_sine(vdev, bins, rate):
    """the interior of a stretched unit sine is a unit sine of the same frequency:
    amplitude within 1e-3 of 1, residual rms <= 1e-3 (the f64 model with a plain
    ISTFT gives 1.00000 and <= 2.1e-4 on these inputs)"""
    nfft, hop, n = 256, 64, 10240
    w = 2.0 * np.pi * bins / nfft
    x = np.sin(w * np.arange(n)).astype(np.float32)
    st = vdev.Stft(nfft, hop)
    y = st.time_stretch(dev(x), rate).cpu().numpy().astype(np.float64)
    assert len(y) == st.time_stretch_length(n, rate)[1]
    i = np.arange(2 * nfft, len(y) - 3 * nfft)
    assert len(i) > 4 * nfft
    A = np.stack([np.sin(w * i), np.cos(w * i)], axis=1)
    coef, *_ = np.linalg.lstsq(A, y[i], rcond=None)
    amp = float(np.hypot(*coef))
    rms = float(np.sqrt(np.mean((y[i] - A @ coef) ** 2)))
    print(f"sine at {bins} bins, rate {rate}: amplitude {amp:.6f}, residual rms {rms:.2e}")
    assert abs(amp - 1.0) <= 1e-3
    assert rms <= 1e-3


def test_degenerate_calls(vdev):
    vv = vdev
    n_fft, T = 64, 5
    D = pu.noise_rows(T, n_fft, 24, nch=2)
    assert vv.phase_vocoder(dev(D), n_fft, m=0).shape == (2, 0, n_fft)
    assert vv.phase_vocoder(dev(D[:0]), n_fft, m=3).shape == (0, 3, n_fft)
    # the C entry points: OK and nothing written
    L = vv.lib()
    out = torch.full((2, 4, n_fft), complex(pu.CANARY), dtype=torch.complex64, device="cuda")
    d, pos = dev(D), dev(np.zeros(4, np.float32))
    vv.debug_clear("STAT_PVOC_ROWS")
    for nch, m in ((2, 0), (0, 4)):
        assert L.vv_dsp_phase_vocoder_uniform_device(d.data_ptr(), T, n_fft, nch, T * n_fft, 0.0, 1.0, m,
                                                     out.data_ptr(), 4 * n_fft, None) == pu.OK
        assert L.vv_dsp_phase_vocoder_device(d.data_ptr(), T, n_fft, nch, T * n_fft, pos.data_ptr(), m,
                                             out.data_ptr(), 4 * n_fft, None) == pu.OK
    torch.cuda.synchronize()
    assert vv.debug_get("STAT_PVOC_ROWS") == 0 and torch.all(out == complex(pu.CANARY))
    # T == 1: one analysis row, held and faded towards the zero row after it
    one = pu.noise_rows(1, n_fft, 25)
    p = pu.uniform_positions(0.0, 0.125, 9)
    got = run(vv, one, n_fft, None, uniform=(0.0, 0.125, 9))
    pu.check(got, pu.model(one, n_fft, p), n_fft, "T 1")
    assert np.all(got[8] == 0)
    # a signal shorter than a frame: one frame in, rows and samples by the rule
    st = vv.Stft(256, 64)
    y = st.time_stretch(dev(np.ones(100, np.float32)), 0.25)
    assert y.shape == (3 * 64 + 256,) and bool(torch.all(torch.isfinite(y)))
    # a bad rate is refused with the output untouched
    buf = torch.full((600,), -7.25, dtype=torch.float32, device="cuda")
    ln = C.c_size_t(77)
    for rate in (0.0, -1.0, float("nan"), float("inf")):
        assert L.vv_dsp_stft_time_stretch_device(st.h, buf.data_ptr(), 100, 1, 100, rate, buf.data_ptr(), 600, None,
                                                 C.byref(ln)) == pu.ERR_RANGE
    assert L.vv_dsp_stft_time_stretch_device(st.h, buf.data_ptr(), 100, 1, 100, 0.25, buf.data_ptr(), 447, None,
                                             C.byref(ln)) == pu.ERR_SIZE
    torch.cuda.synchronize()
    assert ln.value == 77 and bool(torch.all(buf == -7.25))
