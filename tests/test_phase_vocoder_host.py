"""CPU tests of the phase vocoder front-end (include/vv_dsp/spectral/phase_vocoder.h):
the exported symbols, the argument checks in the header's order with the outputs
untouched -- for the three device forms and the host form, all decided before any
device work --, UNSUPPORTED instead of a CPU computation with no GPU, the counter and
the knob, the binding's own checks, the time-stretch's row and sample counts, and the
f64 model of the definition (tests/pvoc_util.py): against the plain wrapped recurrence
(limit 1e-8 m_j; 6e-10 measured), the identity at step 1, zero bins and signed
zeros."""
import ctypes as C

import numpy as np
import pytest

import pvoc_util as pu
from pvoc_util import OK, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_UNSUPPORTED, PvocApi, untouched

INF, NAN = float("inf"), float("nan")
NAMES = ("vv_dsp_phase_vocoder", "vv_dsp_phase_vocoder_uniform_device", "vv_dsp_phase_vocoder_device",
         "vv_dsp_stft_time_stretch_device", "vv_dsp_stft_time_stretch_length")


@pytest.fixture(scope="module")
def api(amd_lib_path):
    return PvocApi(amd_lib_path)


def test_symbols_exported(amd_lib_path):
    lib = C.CDLL(amd_lib_path)
    for name in NAMES:
        assert hasattr(lib, name), name


# positions that check 3 refuses, for T = 8 and m = 5
BAD_UNIFORM = {"start_nan": (NAN, 1.0), "start_inf": (INF, 1.0), "step_nan": (0.0, NAN), "step_inf": (0.0, INF),
               "start_negative": (-0.5, 1.0), "step_negative": (4.0, -0.5), "past_T": (0.0, 2.0 + 2.0 ** -50),
               "start_past_T": (8.5, 0.0)}


def test_argument_rules_in_order_host_form(api):
    spec = pu.noise_rows(8, 64, 1)
    # 1. NULL rows or out, whatever else is wrong
    for kw in ({"null_in": True}, {"null_in": True, "T": 0}):
        st, out = api.run(spec, 64, 0.0, 1.0, 5, **kw)
        assert st == ERR_NULL and untouched(out)
    assert api.run(spec, 64, 0.0, 1.0, 5, null_out=True)[0] == ERR_NULL
    assert api.run(spec, 1, NAN, 1.0, 5, null_in=True)[0] == ERR_NULL
    # 2. n_fft < 2 comes before the positions
    for n_fft in (0, 1):
        for start, step in ((0.0, 1.0), (NAN, -1.0)):
            st, out = api.run(spec, n_fft, start, step, 5)
            assert st == ERR_SIZE and untouched(out)
    # 3. the positions come before the limit
    for name, (start, step) in BAD_UNIFORM.items():
        st, out = api.run(spec, 64, start, step, 5)
        assert st == ERR_RANGE and untouched(out), name
        q = spec.ctypes.data                                # never read: the limit would refuse n_fft
        assert api.lib.vv_dsp_phase_vocoder(q, 8, 2 * pu.MAX_FFT, start, step, 5, q) == ERR_RANGE, name
    # the last position may be exactly T
    assert api.run(spec, 64, 0.0, 2.0, 5)[0] in (OK, ERR_UNSUPPORTED)
    # 4. the kernel's limits (the pointers are never read)
    for n_fft, T, m in ((pu.MAX_FFT + 2, 8, 1), (64, 2 ** 31, 1)):
        assert api.lib.vv_dsp_phase_vocoder(spec.ctypes.data, T, n_fft, 0.0, 0.0, m, spec.ctypes.data) == ERR_UNSUPPORTED
        assert b"limits" in api.lib.vv_dsp_amd_last_error()
    # m == 0: OK, nothing written, no device asked for
    st, out = api.run(spec, 64, 0.0, 1.0, 0)
    assert st == OK


def test_device_forms_check_before_any_device_work():
    """every rule of the device forms is decided before a device is needed (the pointers
    are host dummies or NULL and never read)"""
    import vvdsp_amd as vv
    L = vv.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    uni, cur, ts = L.vv_dsp_phase_vocoder_uniform_device, L.vv_dsp_phase_vocoder_device, L.vv_dsp_stft_time_stretch_device
    vv.debug_clear("STAT_PVOC_ROWS")
    T, n_fft, m = 8, 64, 5
    good = (T * n_fft, m * n_fft)             # the channel strides
    # 1. NULL pointers first
    assert uni(None, T, 1, 2, 0, NAN, 1.0, m, p, 0, None) == ERR_NULL
    assert uni(p, T, 1, 2, 0, NAN, 1.0, m, None, 0, None) == ERR_NULL
    assert cur(None, T, 1, 2, 0, p, m, p, 0, None) == ERR_NULL
    assert cur(p, T, 1, 2, 0, None, m, p, 0, None) == ERR_NULL
    assert cur(p, T, 1, 2, 0, p, m, None, 0, None) == ERR_NULL
    # 2. n_fft < 2 or a short channel stride, before the positions and the limits
    for n in (0, 1):
        assert uni(p, T, n, 2, good[0], NAN, 1.0, m, p, good[1], None) == ERR_SIZE
        assert cur(p, T, n, 2, good[0], p, m, p, good[1], None) == ERR_SIZE
    for strides in ((good[0] - 1, good[1]), (good[0], good[1] - 1), (0, 0)):
        assert uni(p, T, n_fft, 2, strides[0], NAN, 1.0, m, p, strides[1], None) == ERR_SIZE
        assert uni(p, T, n_fft, 1, strides[0], 0.0, 1.0, m, p, strides[1], None) == ERR_SIZE   # one channel too
        assert cur(p, T, n_fft, 2, strides[0], p, m, p, strides[1], None) == ERR_SIZE
        assert cur(p, 2 ** 31, n_fft, 2, strides[0], p, m, p, strides[1], None) == ERR_SIZE    # before the limit
    # 3. the uniform form's positions, before the limits
    for name, (start, step) in BAD_UNIFORM.items():
        assert uni(p, T, n_fft, 2, good[0], start, step, m, p, good[1], None) == ERR_RANGE, name
        big = 2 * pu.MAX_FFT
        assert uni(p, T, big, 2, T * big, start, step, m, p, m * big, None) == ERR_RANGE, name
    # 4. the limits
    big = 2 * pu.MAX_FFT
    assert uni(p, T, big, 2, T * big, 0.0, 1.0, m, p, m * big, None) == ERR_UNSUPPORTED
    assert cur(p, T, big, 2, T * big, p, m, p, m * big, None) == ERR_UNSUPPORTED
    assert cur(p, 2 ** 31, n_fft, 1, 2 ** 31 * n_fft, p, m, p, m * n_fft, None) == ERR_UNSUPPORTED
    # m == 0 or no channel: OK, nothing launched, no device asked for
    assert uni(p, T, n_fft, 2, good[0], 0.0, 1.0, 0, p, 0, None) == OK
    assert uni(p, T, n_fft, 0, good[0], 0.0, 1.0, m, p, good[1], None) == OK
    assert cur(p, T, n_fft, 2, good[0], p, 0, p, 0, None) == OK
    assert cur(p, T, n_fft, 0, good[0], p, m, p, good[1], None) == OK
    # the time-stretch: its handle is a NULL here, which rule 1 answers
    ln = C.c_size_t(77)
    assert ts(None, p, 6400, 2, 6400, 1.25, p, 6400, None, C.byref(ln)) == ERR_NULL
    assert L.vv_dsp_stft_time_stretch_length(None, 6400, 1.25, None, C.byref(ln)) == ERR_NULL
    assert ln.value == 77
    assert np.all(buf == 0)
    assert vv.debug_get("STAT_PVOC_ROWS") == 0


def test_no_gpu_fails_loudly(api):
    L = api.lib
    if L.vvhip_available() > 0:
        pytest.skip("a GPU is visible")
    import vvdsp_amd as vv
    L.vvhip_set_error.argtypes = [C.c_char_p]
    L.vvhip_set_error(b"")
    st, out = api.run(pu.noise_rows(8, 64, 1), 64, 0.0, 1.0, 5)
    assert st == ERR_UNSUPPORTED and untouched(out)                # nothing computed on the CPU
    assert b"no HIP device" in L.vv_dsp_amd_last_error()
    # the device forms with every check passed (the pointers are never read: there is no device)
    buf = np.zeros(2 * 8 * 64, np.float32)
    p = buf.ctypes.data
    V = vv.lib()
    assert V.vv_dsp_phase_vocoder_uniform_device(p, 8, 64, 1, 512, 0.0, 1.0, 5, p, 320, None) == ERR_UNSUPPORTED
    assert V.vv_dsp_phase_vocoder_device(p, 8, 64, 1, 512, p, 5, p, 320, None) == ERR_UNSUPPORTED
    assert np.all(buf == 0)


def test_knob_and_counter_registered():
    import vvdsp_amd as vv
    try:
        vv.debug_set("PVOC_GROUP", 2)
        assert vv.debug_get("PVOC_GROUP") == 2 and vv.debug_get("VVHIP_PVOC_GROUP") == 2
        vv.debug_clear("PVOC_GROUP")
        assert vv.debug_get("PVOC_GROUP") == -1
        vv.debug_set("PVOC_PLANE", 1)
        assert vv.debug_get("PVOC_PLANE") == 1
        vv.debug_clear("PVOC_PLANE")
        assert vv.debug_get("PVOC_PLANE") == -1
        vv.debug_clear("STAT_PVOC_ROWS")
        assert vv.debug_get("STAT_PVOC_ROWS") == 0
    finally:
        vv.debug_clear(None)


def test_binding_checks_without_gpu():
    """the checks of vvdsp_amd.phase_vocoder / Stft.time_stretch that need no device"""
    import torch
    import vvdsp_amd as vv
    x = torch.zeros((2, 8, 64), dtype=torch.complex64)
    for call in (lambda: vv.phase_vocoder(x, 64),                               # not a device tensor
                 lambda: vv.phase_vocoder(x[0, 0], 64),                         # one dimension
                 lambda: vv.phase_vocoder(x.real, 64),                          # not complex64
                 lambda: vv.phase_vocoder(x, 1),                                # n_fft below 2
                 lambda: vv.Stft.time_stretch(None, x.real[0], 1.25),           # not a device signal
                 lambda: vv.Stft.time_stretch(None, x[0], 1.25)):               # not float32
        with pytest.raises(vv.VvError):
            call()


@pytest.mark.parametrize("n,nfft,hop", [(10240, 256, 64), (6400, 400, 160), (100, 256, 64), (4096, 1024, 256)])
def test_time_stretch_row_and_sample_counts(n, nfft, hop):
    """m is the number of j >= 0 with j rate < T, out_len = (m - 1) hop + n_fft, where
    T / rate is an integer and where it is not"""
    import vvdsp_amd as vv
    f = vv.lib().vvhip_stft_stretch_length
    T = 1 if n < nfft else 1 + (n - nfft + hop) // hop
    for rate in pu.RATES + (1.25, 4.0, 0.1, 7.0 / 3.0, float(T), T + 0.5, 0.25):
        m, ln = C.c_size_t(0), C.c_size_t(0)
        assert f(n, nfft, hop, rate, C.byref(m), C.byref(ln)) == OK
        want = pu.stretch_rows(T, rate)
        assert m.value == want and ln.value == (want - 1) * hop + nfft, (rate, T, m.value, want)
        assert (want - 1) * rate < T <= want * rate
        assert f(n, nfft, hop, rate, None, None) == OK
    whole = [r for r in (0.5, 1.0, 2.0, 0.25) if (T / r) == int(T / r)]
    assert whole and all(pu.stretch_rows(T, r) == int(T / r) for r in whole)
    assert pu.stretch_rows(9, 2.0) == 5 and pu.stretch_rows(8, 2.0) == 4 and pu.stretch_rows(10, 3.0) == 4
    m = C.c_size_t(5)
    for rate in (0.0, -1.0, INF, NAN):
        assert f(n, nfft, hop, rate, C.byref(m), None) == ERR_RANGE and m.value == 5
    assert f(n, 1, 1, 1.0, C.byref(m), None) == ERR_SIZE and f(n, nfft, 0, NAN, C.byref(m), None) == ERR_SIZE
    assert f(n, nfft, hop, 2.0 ** -40, C.byref(m), None) == ERR_UNSUPPORTED and m.value == 5


# ------------------------------------------------------------- the model
@pytest.mark.parametrize("rate", pu.RATES, ids=lambda r: "rate%.3g" % r)
def test_model_agrees_with_the_wrapped_recurrence(rate):
    n_fft, hop, T = 64, 16, 240
    D = pu.noise_rows(T, n_fft, 11)
    m = pu.stretch_rows(T, rate)
    assert m > 100
    p = pu.uniform_positions(0.0, rate, m)
    mdl = pu.model(D, n_fft, p)
    z = pu.recurrence(D, n_fft, hop, p)
    err = np.abs(mdl["z"] - z)
    assert np.all(mdl["mj"] > 0)
    worst = float(np.max(err / mdl["mj"]))
    print(f"model against the wrapped recurrence, rate {rate:.3g}, {m} rows: {worst:.2e} m_j")
    assert worst <= 1e-8


def test_model_order_is_the_headers():
    """the segment length is the header's, and the sum is formed segment by segment:
    the floats agree with the sequential order (the phase differs at the 1e-12 level)"""
    assert pu.S == 32
    D = pu.noise_rows(130, 64, 12)
    p = pu.uniform_positions(0.0, 0.5, 259)
    a, b = pu.model(D, 64, p), pu.model(D, 64, p, S=10 ** 9)
    assert np.max(np.abs(a["z"] - b["z"]) / a["mj"]) < 1e-11
    assert np.array_equal(a["z"][:pu.S + 1], b["z"][:pu.S + 1])      # one segment, and a zero base, are the same sum
    differing = int(np.sum(a["out"] != b["out"]))
    print("segments against the sequential order:", differing, "of", a["out"].size, "floats differ")
    assert differing <= a["out"].size // 1000


def test_model_identity_at_step_one():
    """start 0, step 1: the floats of the lower half come back, and the mirror bins are
    their conjugates"""
    for n_fft, T in ((64, 70), (400, 9), (2, 40)):
        K = n_fft // 2 + 1
        D = pu.noise_rows(T, n_fft, 13)
        out = pu.model(D, n_fft, pu.uniform_positions(0.0, 1.0, T))["out"]
        assert np.array_equal(out[:, :K], D[:, :K])
        for k in range(1, K):
            if 2 * k < n_fft:
                assert np.array_equal(out[:, n_fft - k], np.conj(D[:, k]))


def test_model_zero_bins_and_signed_zeros():
    D = pu.noise_rows(6, 8, 14)
    D[:, 1] = 0.0
    D[:, 2] = np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0]) + 1j * np.array([-0.0, 0.0, 0.0, -0.0, -0.0, 0.0])
    D[2, 3] = np.complex64(-0.0 + 0.0j)                   # atan2(+0, -0) would be pi
    mag, th = pu._planes(D, 8)
    assert np.all(th[:, 1] == 0) and np.all(th[:, 2] == 0) and th[2, 3] == 0 and np.all(mag[:, 2] == 0)
    out = pu.model(D, 8, pu.uniform_positions(0.0, 0.5, 11))["out"]
    for k in (1, 2, 8 - 1, 8 - 2):
        assert np.all(out[:, k] == 0)
    for k in (1, 2):                                       # (+0, +0); the mirror bin is its conjugate
        assert not np.any(np.signbit(out[:, k].real) | np.signbit(out[:, k].imag))
    assert np.all(np.isfinite(out.view(np.float32)))
    # a non-finite bin: both components of its column are NaN from the first row that uses it
    # onward, nothing else changes
    E = D.copy()
    E[3, 4] = np.complex64(INF + 0j)
    a, b = pu.model(D, 8, pu.uniform_positions(0.0, 0.5, 11))["out"], pu.model(E, 8, pu.uniform_positions(0.0, 0.5, 11))["out"]
    first = 4                                              # position 2.0 reads rows 2 and 3
    assert np.all(np.isnan(b[first:, 4].real)) and np.all(np.isnan(b[first:, 4].imag))
    assert np.array_equal(b[:first], a[:first])
    keep = [k for k in range(8) if k != 4]
    assert np.array_equal(b[:, keep], a[:, keep])


def test_model_infinite_bin_is_nan_from_its_first_use():
    """an infinity has neither an infinite magnitude nor a finite phase here: the column is
    NaN in both components from the first use on, whether that use is row t0 + 1 with
    0 < a < 1 (rate 0.8), row t0 (rate 2, an even row) or either on a backwards curve"""
    n_fft, T, k = 64, 40, 2
    D = pu.noise_rows(T, n_fft, 15)
    for val in (complex(INF, 1.0), complex(1.0, -INF), complex(-INF, INF)):
        for name, p, t in (("0.8", pu.uniform_positions(0.0, 0.8, 50), 20), ("2", pu.uniform_positions(0.0, 2.0, 20), 20),
                           ("2 odd", pu.uniform_positions(0.0, 2.0, 20), 21),
                           ("backwards", pu.curve_positions(pu.curve("backwards", T, 67), T), 20)):
            E = D.copy()
            E[t, k] = np.complex64(val)
            mag, th = pu._planes(E, n_fft)
            assert np.isnan(mag[t, k]) and np.isnan(th[t, k])
            t0 = np.floor(p).astype(int)
            first = int(np.argmax((t0 == t) | (t0 + 1 == t)))
            a, b = pu.model(D, n_fft, p)["out"], pu.model(E, n_fft, p)["out"]
            for col in (k, n_fft - k):
                assert np.all(np.isnan(b[first:, col].real)) and np.all(np.isnan(b[first:, col].imag)), (name, val)
                assert not np.any(np.isinf(b[:, col].real) | np.isinf(b[:, col].imag))
            assert np.array_equal(b[:first], a[:first]), name
            keep = [q for q in range(n_fft) if q not in (k, n_fft - k)]
            assert np.array_equal(b[:, keep], a[:, keep])
    # at rate 0.8 the first use of row 20 is row t0 + 1 = 20 at position 19.2: 0 < a < 1
    p = pu.uniform_positions(0.0, 0.8, 50)
    j = int(np.argmax(np.floor(p) + 1 == 20))
    assert 0 < p[j] - np.floor(p[j]) < 1


def test_case_table_covers_the_issue():
    S = pu.S
    assert {c[0] for c in pu.CASES} == {64, 400, 1024, 2}
    for n_fft in (64, 400, 1024, 2):
        rows = [c for c in pu.CASES if c[0] == n_fft and c[2] == "u" and c[3][0] == 0.0]
        assert {c[3][1] for c in rows} >= set(pu.RATES)
        assert {c[4] for c in rows} >= {S - 1, S, S + 1, 2 * S + 1}
    Ts = [c[1] for c in pu.CASES]
    assert min(Ts) == 1 and 120 <= max(Ts) <= 160
    assert any(c[2] == "u" and c[3][0] > 0 for c in pu.CASES)
    assert any(c[2] == "u" and pu.uniform_positions(c[3][0], c[3][1], c[4])[-1] == c[1] for c in pu.CASES)
    assert {c[3] for c in pu.CASES if c[2] == "c"} == {"clamped", "nan", "backwards"}
    for c in pu.CASES:
        pos, p = pu.case_positions(c)
        assert len(p) == c[4] and p.min() >= 0 and p.max() <= c[1]
    pos, p = pu.case_positions(next(c for c in pu.CASES if c[3] == "clamped"))
    assert pos[0] < 0 and pos[-1] > 50 and p[0] == 0 and p[-1] == 50
    assert np.isnan(pu.curve("nan", 30, S + 1)).sum() == 1 and np.all(np.diff(pu.curve("backwards", 40, 9)) < 0)
