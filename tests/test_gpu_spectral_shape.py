"""GPU tests of the spectral shape kernel (shape_kernels.hip) against the f64 model of
include/vv_dsp/features/spectral_shape.h (tests/shape_util.py, which states the
comparison rule): the case table, groups, the independence of a row's values from the
batch, the pitch, the outputs requested, the load path and the entry point, the STFT
route, edge rows inside a batch and the degenerate calls.

Observed on an MI355X over the case table (105 rows, 8 f64-class outputs each):
840 values equal to the model's float, 0 at 1 ulp; peak bin and roll-off equal on
every row."""
import ctypes as C

import numpy as np
import pytest
import torch

import shape_util as su
from shape_util import CASES, CASE_IDS, NAMES, params

pytestmark = pytest.mark.gpu


def vparams(vv, q):
    return vv.SpectralShapeParams(q.n_fft, q.sample_rate, q.magnitude, q.k_min, q.k_max, q.rolloff, q.floor)


def device_rows(rows, pitch, offset=0, fill=np.nan):
    """rows [r][K] on the device `pitch` floats apart, the first `offset` floats past a
    16-byte boundary; the pad floats hold `fill` (a NaN: reading one would show)"""
    r, K = rows.shape
    host = np.full(offset + r * pitch, fill, np.float32)
    view = host[offset:].reshape(r, pitch)
    view[:, :K] = rows
    dev = torch.from_numpy(host).cuda()
    return dev[offset:].view(r, pitch)


def run(vv, rows, q, pitch=None, offset=0, what=NAMES, rpg=0):
    K = rows.shape[1]
    d = device_rows(rows, pitch or K, offset)
    got = vv.spectral_shape(d, vparams(vv, q), what, rows_per_group=rpg)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def same_bits(a, b, names=NAMES):
    for n in names:
        x, y = np.asarray(a[n]), np.asarray(b[n])
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), (n, x, y)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case_against_model(vdev, i):
    case = CASES[i]
    rows, want = su.case_model(i)
    before = vdev.debug_get("STAT_SHAPE_WAVE")
    got = run(vdev, rows, su.case_params(case), su.case_pitch(case), case[3])
    assert vdev.debug_get("STAT_SHAPE_WAVE") == before + 1
    counts = su.compare(got, want)
    print(CASE_IDS[i], " ".join(f"{n}={e}/{u}" for n, (e, u) in counts.items()), "(exact/1 ulp)")


def test_groups(vdev):
    rows = su.case_rows(1024, 15, 31)
    q = params(1024)
    for rpg in (5, 0, 1, 4, 15, 40):           # 4: a short last group; 40: more than there are rows
        want = su.model_rows(rows, q, rpg if rpg <= 15 else 0)
        got = run(vdev, rows, q, 544, rpg=rpg)
        su.compare(got, want)
        starts = [r for r in range(15) if rpg and r % rpg == 0] or [0]
        assert np.all(got["flux"][starts] == 0)
        assert np.all(np.delete(got["flux"], starts) > 0)
    # a (ch, frames, pitch) tensor: one group per channel
    d = device_rows(rows, 544).view(3, 5, 544)
    got = vdev.spectral_shape(d, vparams(vdev, q), NAMES)
    want = su.model_rows(rows, q, 5)
    assert got["flux"].shape == (3, 5)
    su.compare({k: v.cpu().numpy().reshape(15) for k, v in got.items()}, want)


@pytest.mark.parametrize("n_fft", (130, 1024, 16384))
def test_values_depend_on_the_row_alone(vdev, n_fft):
    """one row (with its predecessor) alone, in a batch of 7 and at another pitch; every single
    output against all ten; 4-byte against 16-byte loads; the host call: all bit for bit"""
    K = n_fft // 2 + 1
    rows = su.case_rows(n_fft, 7, 41)
    q = params(n_fft, magnitude=1, band=(1, K - 2), rolloff=0.5)
    pitch16 = (K + 3) // 4 * 4 + 4                               # 16-byte loads
    full = run(vdev, rows, q, pitch16)
    su.compare(full, su.model_rows(rows, q))
    for r in (0, 3, 6):
        lo = max(r - 1, 0)
        alone = run(vdev, rows[lo:r + 1], q, K)                  # packed: 4-byte loads unless K % 4 == 0
        same_bits({n: alone[n][-1:] for n in NAMES}, {n: full[n][r:r + 1] for n in NAMES})
    for pitch, off in ((K, 0), (K + 1, 0), (pitch16, 1), (pitch16 + 28, 0)):
        same_bits(run(vdev, rows, q, pitch, off), full)
    for name in NAMES:
        same_bits(run(vdev, rows, q, pitch16, what=(name,)), full, (name,))
    same_bits(run(vdev, rows, q, pitch16, what=("centroid", "rolloff")), full, ("centroid", "rolloff"))
    # the two load paths, each seen taken: STAT_SHAPE_VEC16 counts the launches with 16-byte loads
    vec = vdev.debug_get("STAT_SHAPE_VEC16")
    same_bits(run(vdev, rows, q, pitch16), full)
    assert vdev.debug_get("STAT_SHAPE_VEC16") == vec + 1
    with vdev.knobs(SHAPE_DWORD=1):
        same_bits(run(vdev, rows, q, pitch16), full)
    assert vdev.debug_get("STAT_SHAPE_VEC16") == vec + 1
    for pitch, off in ((K + 1 if (K + 1) % 4 else K + 2, 0), (pitch16, 1)):      # a pitch or a base that bars them
        run(vdev, rows, q, pitch, off)
        assert vdev.debug_get("STAT_SHAPE_VEC16") == vec + 1
    # the host one-row call goes through the same kernel
    api = su.ShapeApi(vdev.LIB_PATH)
    for r in (0, 4):
        st, v = api.row(rows[r], q, prev=rows[r - 1] if r else None)
        assert st == su.OK
        host = {n: np.array([getattr(v, n)], np.uint32 if n == "peak_bin" else np.float32) for n in NAMES}
        same_bits(host, {n: full[n][r:r + 1] for n in NAMES})


@pytest.mark.parametrize("n_fft,hop", ((1024, 256), (400, 160)))
def test_stft_route(vdev, n_fft, hop):
    vv = vdev
    sig = torch.from_numpy(su_signals()).cuda()
    nch, n = sig.shape
    st = vv.Stft(n_fft, hop)
    K, fr = n_fft // 2 + 1, st.frames(n)
    q = vparams(vv, params(n_fft, magnitude=1))
    pitch = (K + 31) // 32 * 32
    power = st.power(sig, pitch=pitch)
    want = vv.spectral_shape(power, q, NAMES)
    got = st.spectral_shape(sig, q, NAMES)
    torch.cuda.synchronize()
    for name in NAMES:
        assert got[name].shape == (nch, fr)
        assert torch.equal(got[name].view(torch.int32), want[name].view(torch.int32)), name
    # one group per channel: flux 0 at each channel's first frame (later frames may repeat: silence)
    assert float(want["flux"][:, 0].abs().max()) == 0 and float(want["flux"][:, 1:].max()) > 0
    assert bool((want["flux"][:, 1:] > 0).any(dim=1).all())
    # a padded out_ch_stride through the C entry point, and out_frames
    stride = fr + 3
    planes = {n: torch.full((nch, stride), -7, dtype=torch.int32 if n == "peak_bin" else torch.float32, device="cuda")
              for n in NAMES}
    out = vv.SpectralShapeOut(*[planes[n].data_ptr() for n in NAMES])
    nf = C.c_size_t(0)
    f = vv.lib().vv_dsp_stft_spectral_shape_device
    assert f(st.h, C.byref(q), sig.data_ptr(), n, nch, sig.stride(0), C.byref(out), stride, None, C.byref(nf)) == 0
    torch.cuda.synchronize()
    assert nf.value == fr
    for name in NAMES:
        assert torch.equal(planes[name][:, :fr].view(torch.int32), want[name].view(torch.int32)), name
        assert torch.all(planes[name][:, fr:] == -7), name
    # params->n_fft must be the handle's
    other = vparams(vv, params(n_fft * 2))
    assert f(st.h, C.byref(other), sig.data_ptr(), n, nch, sig.stride(0), C.byref(out), stride, None, None) == su.ERR_SIZE
    assert f(st.h, C.byref(q), sig.data_ptr(), n, nch, sig.stride(0), C.byref(out), fr - 1, None, None) == su.ERR_SIZE
    assert f(st.h, C.byref(q), sig.data_ptr(), n, 1, sig.stride(0), C.byref(out), fr - 1, None, None) == su.ERR_SIZE
    # the header's order on a live handle: the n_fft mismatch (rule 2) before the band (3) before
    # sample_rate / floor / rolloff (4); nothing is launched and no plane is written
    before = vv.debug_get("STAT_SHAPE_WAVE")
    K2 = n_fft // 2

    def call(p):
        return f(st.h, C.byref(vparams(vv, p)), sig.data_ptr(), n, nch, sig.stride(0), C.byref(out), stride, None, None)
    assert call(params(n_fft * 2, band=(5, 4))) == su.ERR_SIZE
    assert call(params(n_fft + 2, rolloff=7.0)) == su.ERR_SIZE
    for band in ((5, 4), (0, K2 + 1)):
        assert call(params(n_fft, band=band)) == su.ERR_RANGE
        assert call(params(n_fft, band=band, rolloff=0.0, fs=-1.0)) == su.ERR_RANGE
    for kw in ({"rolloff": 0.0}, {"rolloff": 1.5}, {"floor": 0.0}, {"floor": float("nan")}, {"fs": 0.0},
               {"fs": float("inf")}):
        assert call(params(n_fft, **kw)) == su.ERR_RANGE, kw
    assert vv.debug_get("STAT_SHAPE_WAVE") == before
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(planes[name][:, :fr].view(torch.int32), want[name].view(torch.int32)), name


def test_stft_route_limit(vdev):
    """rule 5 on a live handle: 8194 bins are UNSUPPORTED, after the band and the parameters"""
    vv = vdev
    st = vv.Stft(16386, 4096)
    sig = torch.zeros((1, 16386), device="cuda")
    plane = torch.full((1, 4), -7.0, device="cuda")
    out = vv.SpectralShapeOut(energy=plane.data_ptr())
    f = vv.lib().vv_dsp_stft_spectral_shape_device

    def call(p):
        return f(st.h, C.byref(vparams(vv, p)), sig.data_ptr(), 16386, 1, 16386, C.byref(out), 4, None, None)
    assert call(params(16386)) == su.ERR_UNSUPPORTED
    assert call(params(16386, band=(9, 3))) == su.ERR_RANGE
    assert call(params(16386, rolloff=2.0)) == su.ERR_RANGE
    torch.cuda.synchronize()
    assert torch.all(plane == -7.0)


def su_signals():
    import pitch_util
    return pitch_util.signals()


@pytest.mark.parametrize("magnitude", (0, 1))
def test_edge_rows_inside_a_batch(vdev, magnitude):
    n_fft, K = 1024, 513
    q = params(n_fft, magnitude=magnitude)
    fs = 16000.0
    base = su.case_rows(n_fft, 11, 51)
    clean = run(vdev, base, q, 544)
    rows = base.copy()
    rows[1] = 0.0                                   # all zero
    rows[3] = 0.0
    rows[3, 200] = 2.25                             # one non-zero bin
    rows[5] = 1e-30                                 # zeros below the floor
    rows[7, 77] = np.nan                            # one NaN
    rows[9, 300] = -4.0                             # one negative bin
    got = run(vdev, rows, q, 544)
    f64 = ("energy", "centroid", "spread", "skewness", "kurtosis", "flatness", "crest")
    # all zero: the defined zeros, flatness 1, roll-off and peak at k_min
    for n in ("energy", "centroid", "spread", "skewness", "kurtosis", "crest", "rolloff"):
        assert got[n][1] == 0, n
    assert got["flatness"][1] == 1.0 and got["peak_bin"][1] == 0
    # one non-zero bin
    w = np.float32(1.5 if magnitude else 2.25)
    hz = np.float32(200 * fs / n_fft)
    assert got["energy"][3] == w and got["centroid"][3] == hz and got["rolloff"][3] == hz and got["peak_bin"][3] == 200
    assert got["spread"][3] == 0 and got["skewness"][3] == 0 and got["kurtosis"][3] == 0
    assert got["crest"][3] == np.float32(K)
    # below the floor everywhere: flatness 1 (every w' is the floor), the rest from the tiny weights
    assert got["flatness"][5] == 1.0 and got["crest"][5] == 1.0 and got["peak_bin"][5] == 0
    assert got["centroid"][5] == np.float32(256 * fs / n_fft)
    want = su.model_rows(rows, q)
    for r in (1, 3, 5):
        for n in f64 + ("flux",):
            assert su.f32_ulps(got[n][r], want[n][r]) <= 1, (n, r)
        assert got["rolloff"][r] == want["rolloff"][r] and got["peak_bin"][r] == want["peak_bin"][r]
    # a NaN (and, as a weight, a negative power) poisons the f64 class of its row and the next row's flux
    bad = (7, 9)
    for r in bad:
        for n in f64 + ("flux",):
            assert np.isnan(got[n][r]), (n, r)
        assert np.isnan(got["flux"][r + 1])
        assert got["peak_bin"][r] == want["peak_bin"][r] and got["rolloff"][r] == want["rolloff"][r]
    # every other row is what it was without the edge rows, but for the flux that reads one
    for r in (0, 2, 4, 6, 8, 10):
        same_bits({n: got[n][r:r + 1] for n in NAMES}, {n: clean[n][r:r + 1] for n in NAMES},
                  [n for n in NAMES if n != "flux" or r == 0])
        if r:
            assert su.f32_ulps(got["flux"][r], want["flux"][r]) <= 1 or r - 1 in bad


def test_degenerate_calls(vdev):
    vv = vdev
    q = vparams(vv, params(1024))
    d = device_rows(su.case_rows(1024, 3, 61), 544)
    before = vv.debug_get("STAT_SHAPE_WAVE")
    assert vv.spectral_shape(d, q, ()) == {}
    none = vv.SpectralShapeOut()
    f = vv.lib().vv_dsp_spectral_shape_device
    assert f(d.data_ptr(), 3, 544, 0, C.byref(q), C.byref(none), None) == 0
    assert vv.debug_get("STAT_SHAPE_WAVE") == before
    plane = torch.full((3,), -7.0, device="cuda")
    one = vv.SpectralShapeOut(energy=plane.data_ptr())
    assert f(d.data_ptr(), 0, 544, 0, C.byref(q), C.byref(one), None) == 0
    torch.cuda.synchronize()
    assert torch.all(plane == -7.0) and vv.debug_get("STAT_SHAPE_WAVE") == before
    got = vv.spectral_shape(d[:0], q, ("energy",))
    assert got["energy"].shape == (0,)
