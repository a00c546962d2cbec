"""GPU tests of the YIN pitch kernel (pitch_kernels.hip, shim_pitch.hip) against the
f64 model of the definition in tests/pitch_util.py (the reference library has no
pitch code; include/vv_dsp/features/pitch.h is the definition).

What is compared how (the conventions of tests/test_gpu_stats.py):
  * the curve d' (cmnd) at <= 1 float32 ulp from the model on every frame: another
    f64 summation order moves the f64 value by about W 2^-53 relative, far below
    half a float32 ulp, so the rounded value is the model's float or its neighbour;
  * lag equal, f0 and aperiodicity at <= 1 ulp on every decidable frame (decision
    margin >= 1e-9, pitch_util.py); at most 1 % of the frames may be undecidable
    (the model leaves none: tests/test_pitch_host.py) and at most 1 % of the
    values may differ at all; the count is printed;
  * the fused frames form, the rows form at any batch and stride, every subset of
    outputs, both LDS storages and the host call against each other bit for bit.
(tests/test_gpu_pitch.py is about the row pitch of power spectrograms, not this.)
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import pitch_util as pu
from frames_util import fetch_frames
from pitch_util import CASES, CASE_IDS, BATCH, SENTINEL, OK, f32_ulps

pytestmark = pytest.mark.gpu

NAMES = ("f0", "aperiodicity", "lag", "cmnd")
POISON = float("nan")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def vparams(vdev, case):
    return vdev.PitchParams(pu.FS, case[2], case[3], case[6])


def strided(x, pad):
    """device rows of x, (row length + pad) floats apart, the gaps poisoned"""
    import torch
    b, n = x.shape
    buf = torch.full((b, n + pad), POISON, dtype=torch.float32, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return buf[:, :n]


@pytest.fixture
def counter(vdev):
    vdev.debug_clear("STAT_PITCH_WAVE")
    return lambda: vdev.debug_get("STAT_PITCH_WAVE")


def check_against_model(got, m, what):
    """got / m: name -> arrays of equal shape; returns (values compared, values that differ)"""
    u = f32_ulps(got["cmnd"], m["cmnd"])
    assert u.max() <= 1, (what, "cmnd", int(u.max()))
    total, differ = u.size, int(np.sum(u != 0))
    ok = m["margin"] >= pu.MARGIN
    assert np.sum(~ok) <= 0.01 * ok.size, (what, int(np.sum(~ok)))
    assert np.array_equal(got["lag"][ok].astype(np.int64), m["lag"][ok]), what
    for k in ("f0", "aperiodicity"):
        u = f32_ulps(got[k][ok], m[k][ok])
        assert u.max() <= 1, (what, k, int(u.max()))
        total, differ = total + u.size, differ + int(np.sum(u != 0))
    print(f"{what}: {differ} of {total} values not bit-identical to the model, "
          f"{int(np.sum(~ok))} of {ok.size} frames undecidable")
    assert differ <= 0.01 * total, what
    return total, differ


# ---------------------------------------------------------------- 1. the fused form against the model
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_frames_against_model(vdev, counter, i):
    case, (tau_min, tau_max, W) = CASES[i]
    frame, hop, _, _, center, win, _ = case
    sig = dev(pu.signals())
    w = None if win is None else dev(pu.window_of(win, frame))
    assert vdev.pitch_lag_range(vparams(vdev, case), frame) == (tau_min, tau_max, W)
    got = host(vdev.pitch_frames(sig, frame, hop, vparams(vdev, case), NAMES, window=w, center=bool(center)))
    assert counter() == 1
    m = pu.case_model(i)
    fr = pu.num_frames(6400, frame, hop, center)
    assert got["f0"].shape == got["aperiodicity"].shape == got["lag"].shape == (2, fr)
    assert got["cmnd"].shape == (2, fr, tau_max + 1)
    check_against_model(got, m, CASE_IDS[i])
    assert np.all(got["cmnd"][..., 0] == 1.0)
    voiced = got["f0"] > 0
    assert np.all((got["lag"][voiced] >= tau_min) & (got["lag"][voiced] <= tau_max))


# ---------------------------------------------------------------- 2. bit for bit against each other
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_frames_is_the_pipeline(vdev, i):
    """pitch_frames_device == fetch_frames_device -> pitch_device, also with ch_stride > n"""
    import torch
    case = CASES[i][0]
    frame, hop, _, _, center, win, _ = case
    p = vparams(vdev, case)
    w = None if win is None else dev(pu.window_of(win, frame))
    sig = strided(pu.signals(), 5)
    assert sig.stride(0) == 6405
    got = vdev.pitch_frames(sig, frame, hop, p, NAMES, window=w, center=bool(center))
    packed = vdev.pitch_frames(dev(pu.signals()), frame, hop, p, NAMES, window=w, center=bool(center))
    for c in range(2):
        rows = fetch_frames(vdev, sig[c].contiguous(), frame, hop, center, w)
        want = vdev.pitch(rows, p, NAMES)
        for k in NAMES:
            assert torch.equal(got[k][c].view(torch.int32), want[k].view(torch.int32)), (c, k)
            assert torch.equal(got[k][c].view(torch.int32), packed[k][c].view(torch.int32)), (c, k)


@pytest.mark.parametrize("i", [1, 3, 5, 8], ids=[CASE_IDS[i] for i in (1, 3, 5, 8)])
def test_batch_stride_and_storage_change_nothing(vdev, knob, i):
    """batch 1 against batch 67 (rows cycled), contiguous against strided rows with a poisoned
    gap, f64 against f32 rows in LDS"""
    case = CASES[i][0]
    p = vparams(vdev, case)
    r = pu.case_rows(case)
    flat = r.reshape(-1, r.shape[2])
    pick = np.linspace(0, len(flat) - 1, 13).astype(int)       # 13 frames of both channels
    idx = pick[np.arange(BATCH) % 13]
    x = flat[idx]
    full = host(vdev.pitch(dev(x), p, NAMES))
    m = pu.case_model(i)
    check_against_model(full, {k: v.reshape((len(flat),) + v.shape[2:])[idx] for k, v in m.items()},
                        f"rows {CASE_IDS[i]}")
    for k in NAMES:                                              # the row's position changes nothing
        assert same(full[k][:BATCH - 13], full[k][13:]), k
    one = host(vdev.pitch(dev(x[:1]), p, NAMES))
    pad = host(vdev.pitch(strided(x, 3), p, NAMES))
    five = host(vdev.pitch(strided(x[:5], 1), p, NAMES))
    knob("PITCH_F32", 1)
    f32 = host(vdev.pitch(dev(x), p, NAMES))
    for k in NAMES:
        assert same(one[k], full[k][:1]), k
        assert same(pad[k], full[k]), k
        assert same(five[k], full[k][:5]), k
        assert same(f32[k], full[k]), k


def test_every_subset_of_outputs(vdev):
    case = CASES[5][0]
    p = vparams(vdev, case)
    x = dev(pu.case_rows(case)[1][:9])
    sig = dev(pu.signals())
    full = host(vdev.pitch(x, p, NAMES))
    full_fr = host(vdev.pitch_frames(sig, case[0], case[1], p, NAMES))
    for r in range(1, 5):
        for what in itertools.combinations(NAMES, r):
            got = host(vdev.pitch(x, p, what))
            got_fr = host(vdev.pitch_frames(sig, case[0], case[1], p, what))
            assert tuple(got) == what and tuple(got_fr) == what
            for k in what:
                assert same(got[k], full[k]), (what, k)
                assert same(got_fr[k], full_fr[k]), (what, k)
    assert vdev.pitch(x, p, ()) == {}


def test_nothing_wanted_launches_nothing(vdev, counter):
    case = CASES[5][0]
    assert vdev.pitch(dev(pu.case_rows(case)[0][:3]), vparams(vdev, case), ()) == {}
    L = vdev.lib()
    x = dev(pu.case_rows(case)[0][:3])
    none = vdev.PitchOut()
    p = vparams(vdev, case)
    assert L.vv_dsp_pitch_device(x.data_ptr(), 400, 3, 400, C.byref(p), C.byref(none), 0, None) == OK
    assert counter() == 0


def test_host_call_equals_the_batch_row(vdev, amd):
    api = pu.PitchApi(amd.lib)
    for i in (1, 3, 5, 8):
        case = CASES[i][0]
        rows = pu.case_rows(case)
        for x in (rows[0][0], rows[0][len(rows[0]) // 2], rows[1][len(rows[1]) // 2], rows[1][-1]):
            batch = host(vdev.pitch(dev(x[None, :]), vparams(vdev, case), ("f0", "aperiodicity")))
            st, f0, ap = api.yin(x, pu.params(case[2], case[3], case[6]))
            assert st == OK
            assert same(np.array([f0]), batch["f0"]) and same(np.array([ap]), batch["aperiodicity"]), CASE_IDS[i]
    # either output alone
    x = pu.case_rows(CASES[5][0])[0][0]
    p = pu.params(80.0, 400.0, 0.15)
    res = np.full(2, SENTINEL, np.float32)
    fp = C.POINTER(C.c_float)
    assert api.lib.vv_dsp_pitch_yin(x.ctypes.data_as(fp), 400, C.byref(p), res.ctypes.data_as(fp), None) == OK
    assert res[1] == SENTINEL and same(res[:1], host(vdev.pitch(dev(x[None, :]), vparams(vdev, CASES[5][0]), "f0"))["f0"])


# ---------------------------------------------------------------- 3. what lies beyond the outputs
def test_sentinels_survive(vdev):
    """planes wider than their frames, curve rows wider than their curves: the rest is untouched"""
    import torch
    L = vdev.lib()
    s = torch.cuda.current_stream().cuda_stream
    case = CASES[5][0]
    p = vparams(vdev, case)
    tau_max = CASES[5][1][1]
    curve = tau_max + 1
    sig = dev(pu.signals())
    fr = pu.num_frames(6400, 400, 160, 0)
    sent = float(SENTINEL)
    # frames: channels fr + 3 values apart, curves fr * curve + 5 floats apart
    planes = torch.full((3, 2, fr + 3), sent, dtype=torch.float32, device="cuda")
    cm = torch.full((2, fr * curve + 5), sent, dtype=torch.float32, device="cuda")
    out = vdev.PitchOut(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), cm.data_ptr())
    assert L.vv_dsp_pitch_frames_device(sig.data_ptr(), 6400, 2, 6400, 400, 160, 0, None, C.byref(p), C.byref(out),
                                        fr + 3, fr * curve + 5, s) == OK
    torch.cuda.synchronize()
    want = vdev.pitch_frames(sig, 400, 160, p, NAMES)
    assert torch.all(planes[:, :, fr:] == sent) and torch.all(cm[:, fr * curve:] == sent)
    assert torch.equal(planes[0, :, :fr], want["f0"]) and torch.equal(planes[1, :, :fr], want["aperiodicity"])
    assert torch.equal(planes[2, :, :fr].view(torch.int32), want["lag"])
    assert torch.equal(cm[:, :fr * curve].reshape(2, fr, curve), want["cmnd"])
    # rows: curve rows curve + 2 floats apart, planes one value longer than the batch
    rows = dev(pu.case_rows(case)[0][:7])
    planes = torch.full((3, 8), sent, dtype=torch.float32, device="cuda")
    cm = torch.full((7, curve + 2), sent, dtype=torch.float32, device="cuda")
    out = vdev.PitchOut(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), cm.data_ptr())
    assert L.vv_dsp_pitch_device(rows.data_ptr(), 400, 7, 400, C.byref(p), C.byref(out), curve + 2, s) == OK
    torch.cuda.synchronize()
    want = vdev.pitch(rows, p, NAMES)
    assert torch.all(planes[:, 7:] == sent) and torch.all(cm[:, curve:] == sent)
    assert torch.equal(cm[:, :curve], want["cmnd"]) and torch.equal(planes[0, :7], want["f0"])


def test_zero_frames_write_nothing(vdev, counter):
    import torch
    L = vdev.lib()
    s = torch.cuda.current_stream().cuda_stream
    case = CASES[5][0]
    p = vparams(vdev, case)
    sig = dev(pu.signals())
    planes = torch.full((4, 2, 300), float(SENTINEL), dtype=torch.float32, device="cuda")
    out = vdev.PitchOut(*(planes[k].data_ptr() for k in range(4)))
    # n < frame_len, not centred: no frame
    assert L.vv_dsp_pitch_frames_device(sig.data_ptr(), 399, 2, 6400, 400, 160, 0, None, C.byref(p), C.byref(out),
                                        1, 201, s) == OK
    assert L.vv_dsp_pitch_device(sig.data_ptr(), 400, 0, 400, C.byref(p), C.byref(out), 201, s) == OK
    torch.cuda.synchronize()
    assert counter() == 0 and torch.all(planes == float(SENTINEL))
    got = vdev.pitch_frames(sig[:, :399], 400, 160, p, NAMES)
    assert got["f0"].shape == (2, 0) and got["cmnd"].shape == (2, 0, 201)
    assert L.vv_dsp_pitch_frames_device(sig.data_ptr(), 6400, 2, 6400, 400, 0, 0, None, C.byref(p), C.byref(out),
                                        38, 38 * 201, s) == pu.ERR_SIZE


# ---------------------------------------------------------------- 4. edge rows at frame 400
def test_edge_rows_inside_a_batch(vdev):
    case = CASES[5][0]
    p = vparams(vdev, case)
    plain = pu.case_rows(case)[0][[3, 20]]
    base = pu.case_rows(case)[1][2].copy()
    edges = {"const": np.full(400, 0.1, np.float32), "zeros": np.zeros(400, np.float32)}
    e = base.copy()
    e[0] = np.nan
    edges["nan_first"] = e
    e = base.copy()
    e[399] = np.nan
    edges["nan_last"] = e
    e = base.copy()
    e[200] = np.inf
    edges["inf_mid"] = e
    edges["square"] = pu.square_wave(400, 50)
    x = []
    for row in edges.values():       # every edge row between two ordinary rows
        x += [plain[0], row, plain[1]]
    got = host(vdev.pitch(dev(np.stack(x)), p, NAMES))
    alone = host(vdev.pitch(dev(plain), p, NAMES))
    res = {}
    for j, name in enumerate(edges):
        res[name] = (got["f0"][3 * j + 1], got["aperiodicity"][3 * j + 1], int(got["lag"][3 * j + 1]))
        for k in NAMES:              # the neighbours are unaffected
            assert same(got[k][3 * j], alone[k][0]) and same(got[k][3 * j + 2], alone[k][1]), (name, k)
    for name in ("const", "zeros"):
        assert res[name] == (0.0, 1.0, 40), name
        assert np.all(got["cmnd"][3 * list(edges).index(name) + 1] == 1.0)
    for name in ("nan_first", "nan_last", "inf_mid"):
        f0, ap, lag = res[name]
        assert f0 == 0 and np.isnan(ap) and lag == 0, (name, res[name])
    # a NaN at index 399 enters d(200) alone: the curve before it is the clean one
    c = got["cmnd"][3 * list(edges).index("nan_last") + 1]
    assert np.isnan(c[200]) and np.all(np.isfinite(c[:200]))
    # the square wave: d(50) == 0 exactly; the model's f0 (the parabola on d' sits just left of 50)
    f0, ap, lag = res["square"]
    m = pu.model_rows(edges["square"][None], 80.0, 400.0, 0.15)
    assert lag == 50 and ap == 0.0 and bits(np.float32(ap)) == 0
    assert f32_ulps(np.float32(f0), m["f0"][0]) <= 1 and 320.0 < f0 < 320.1


# ---------------------------------------------------------------- 5. the other launch shapes
@pytest.mark.parametrize("n,fmin,rows", [(2048, 60.0, 5), (4096, 60.0, 4), (5000, 7.5, 3), (16384, 1.9535, 2)])
def test_long_frames(vdev, n, fmin, rows):
    """frames past the f64 rows (f32 rows in LDS), fewer than four rows per workgroup, and
    the longest frame with the longest lag range (one row's 128 KiB of LDS)"""
    sig = pu.signals()
    long = np.tile(sig[0], 3)
    x = np.stack([long[r * 371:r * 371 + n] for r in range(rows)])
    p = vdev.PitchParams(pu.FS, fmin, 400.0, 0.15)
    tau_min, tau_max, W = vdev.pitch_lag_range(p, n)
    assert (tau_min, tau_max, W) == pu.lag_range(pu.FS, fmin, 400.0, n)
    if n == 16384:
        assert tau_max == 8191
    got = host(vdev.pitch(dev(x), p, NAMES))
    m = pu.model_rows(x, fmin, 400.0, 0.15)
    u = f32_ulps(got["cmnd"], m["cmnd"])
    assert u.max() <= 1, int(u.max())
    ok = m["margin"] >= pu.MARGIN
    assert np.array_equal(got["lag"][ok].astype(np.int64), m["lag"][ok])
    for k in ("f0", "aperiodicity"):
        assert f32_ulps(got[k][ok], m[k][ok]).max() <= 1, k
    one = host(vdev.pitch(dev(x[-1:]), p, NAMES))
    for k in NAMES:
        assert same(one[k], got[k][-1:]), k


# ---------------------------------------------------------------- 6. binding checks
def test_binding_checks(vdev):
    import torch
    case = CASES[5][0]
    p = vparams(vdev, case)
    x = dev(pu.case_rows(case)[0][:4])
    bad = [lambda: vdev.pitch(x.double(), p, ("f0",)),
           lambda: vdev.pitch(x.cpu(), p, ("f0",)),
           lambda: vdev.pitch(x[:, ::2], p, ("f0",)),                          # sample stride 2
           lambda: vdev.pitch(x, p, ("f0", "pitch")),                          # unknown name
           lambda: vdev.pitch(x[:, :200], p, ("f0",)),                         # W < 1
           lambda: vdev.pitch(x, vdev.PitchParams(16000.0, 80.0, 400.0, 1.5), ("f0",)),
           lambda: vdev.pitch(x.reshape(2, 2, 400), p, ("f0",)),
           lambda: vdev.pitch_frames(x, 400, 160, p, ("f0",), window=dev(pu.hann(399))),
           lambda: vdev.pitch_frames(x, 400, 0, p, ("f0",)),
           lambda: vdev.pitch_frames(x, 0, 160, p, ("f0",)),
           lambda: vdev.pitch_frames(x.double(), 400, 160, p, ("f0",))]
    for i, call in enumerate(bad):
        with pytest.raises(vdev.VvError):
            call()
            pytest.fail(f"case {i} passed the checks")
    got = vdev.pitch(x, p, ("lag", "f0"))
    assert got["lag"].dtype == torch.int32 and got["f0"].dtype == torch.float32
    one = vdev.pitch(x[0], p, NAMES)
    assert one["f0"].dim() == 0 and one["cmnd"].shape == (201,) and one["f0"] == got["f0"][0]
