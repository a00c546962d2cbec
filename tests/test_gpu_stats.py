"""GPU tests of the statistics kernels (stats_kernels.hip, shim_stats.hip) against
the reference's outputs in tests/golden/stats_*.npz.

What is compared how:
  * the exact class (min, max, argmin, argmax, zero crossings) bit for bit and
    count for count against the reference;
  * the f64 class (sum, rms, var, skewness, kurtosis, the correlations) at
    <= 1 float32 ulp from the reference's value: another f64 summation order
    moves the f64 value by about n 2^-53 relative, far below half a float32 ulp,
    so the rounded result is the reference's float or its neighbour.  At most
    1 % of the values may differ at all (the f64 model differs on none); the
    count is printed;
  * mean and crest, derived in float32 from sum and rms / min / max, at <= 1 ulp
    of their inputs' effect: they are bit-identical whenever their inputs are,
    which is asserted row by row;
  * both routes, every output mask, the host calls and the frames form against
    each other bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import frames_util
from frames_util import fetch_frames, hamming
from stats_util import (StatsApi, STAT_NAMES, COUNT_NAMES, EXACT_NAMES, F64_NAMES, ENERGY_NAMES, MIN_LEN, ROW_N, BATCH,
                        SLICES, CHUNK, LONG_N, AUTO_CASES, CROSS_CASES, EDGE_N, SENTINEL, ERR_SIZE, OK, load,
                        signals, valid_names, batch_rows, long_row, edge_rows, f32_ulps)

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def golden_rows():
    return load("stats_rows")


@pytest.fixture(scope="module")
def golden_corr():
    return load("stats_corr")


@pytest.fixture
def counters(vdev):
    vdev.debug_clear("STAT_STATS_WAVE")
    vdev.debug_clear("STAT_STATS_LONG")
    return lambda: (vdev.debug_get("STAT_STATS_WAVE"), vdev.debug_get("STAT_STATS_LONG"))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(x, pad):
    """device rows of x, (row length + pad) floats apart"""
    import torch
    b, n = x.shape
    buf = torch.full((b, n + pad), 7.5, dtype=torch.float32, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return buf[:, :n]


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def check_against_reference(got, want, prefix, nrows, names):
    """got[name] [rows] against want[prefix + name] [SLICES] cycled; returns (values, differing) of the f64 class"""
    idx = np.arange(nrows) % len(want[prefix + names[0]])
    total = differ = 0
    for name in names:
        ref = want[prefix + name][idx]
        if name in COUNT_NAMES:
            assert np.array_equal(got[name].astype(np.int64), ref), name
        elif name in EXACT_NAMES:
            assert same(got[name], ref), name
        else:
            u = f32_ulps(got[name], ref)
            assert u.max() <= 1, (name, int(u.max()))
            if name in F64_NAMES:
                total += u.size
                differ += int(np.sum(u != 0))
    # derived values are bit-identical whenever their inputs are
    if "mean" in names:
        ok = bits(got["sum"]) == bits(want[prefix + "sum"][idx])
        assert np.array_equal(bits(got["mean"])[ok], bits(want[prefix + "mean"][idx])[ok])
    if "crest" in names:
        ok = bits(got["rms"]) == bits(want[prefix + "rms"][idx])
        assert np.array_equal(bits(got["crest"])[ok], bits(want[prefix + "crest"][idx])[ok])
    return total, differ


# ---------------------------------------------------------------- 1. rows
@pytest.mark.parametrize("long_route", [0, 1])
@pytest.mark.parametrize("n", ROW_N)
def test_rows_against_reference(vdev, golden_rows, knob, counters, n, long_route):
    if long_route:
        knob("STATS_LONG", 1)
    names = valid_names(n)
    x = batch_rows(n)
    total = differ = 0
    first = None
    for batch, pad in ((BATCH, 0), (BATCH, 4), (1, 0), (1, 4)):
        got = host(vdev.stats(strided(x[:batch], pad), names))
        assert all(got[k].shape == (batch,) for k in names)
        t, d = check_against_reference(got, golden_rows, f"n{n}_", batch, names)
        total, differ = total + t, differ + d
        if first is None:
            first = got
        for k in names:   # the batch, the row's position and the stride change nothing
            assert same(got[k], first[k][:batch]), (k, batch, pad)
            assert same(first[k][:BATCH - SLICES], first[k][SLICES:]), k
    assert counters() == ((0, 4) if long_route else (4, 0))
    print(f"n={n} long={long_route}: {differ} of {total} f64-class values not bit-identical to the reference")
    assert differ <= 0.01 * total


def test_long_row(vdev, golden_rows, knob, counters):
    """3 chunks + 17 samples: below the wave kernel's limit, so the knob picks the route"""
    x = long_row()[None, :]
    assert x.shape[1] == LONG_N == 3 * CHUNK + 17
    wave = host(vdev.stats(dev(x), STAT_NAMES))
    knob("STATS_LONG", 1)
    long = host(vdev.stats(dev(x), STAT_NAMES))
    assert counters() == (1, 1)
    total, differ = check_against_reference(long, golden_rows, "long_", 1, STAT_NAMES)
    print(f"long row: {differ} of {total} f64-class values not bit-identical to the reference")
    assert differ <= 0.01 * total
    for k in STAT_NAMES:
        assert same(wave[k], long[k]), k


def test_row_beyond_the_wave_limit_takes_the_long_route(vdev, counters):
    """16385 samples take the long route without the knob; checked against the f64 model"""
    from stats_util import model
    x = np.tile(signals()[0], 2)[:16385]
    got = host(vdev.stats(dev(x[None, :]), STAT_NAMES))
    assert counters() == (0, 1)
    m = model(x)
    for k in STAT_NAMES:
        if k in COUNT_NAMES:
            assert int(got[k][0]) == m[k], k
        elif k in EXACT_NAMES:
            assert same(got[k], np.array([m[k]], np.float32)), k
        else:
            assert f32_ulps(got[k], np.array([m[k]], np.float32)).max() <= 1, k


# ---------------------------------------------------------------- 2. edge rows inside a batch
@pytest.mark.parametrize("long_route", [0, 1])
@pytest.mark.parametrize("n", EDGE_N)
def test_edge_rows_inside_a_batch(vdev, golden_rows, knob, n, long_route):
    if long_route:
        knob("STATS_LONG", 1)
    edges = edge_rows(n)
    plain = batch_rows(n, 2)
    x = []
    for row in edges.values():       # every edge row between two ordinary rows
        x += [plain[0], row, plain[1]]
    got = host(vdev.stats(dev(np.stack(x)), STAT_NAMES))
    alone = host(vdev.stats(dev(plain), STAT_NAMES))
    for j, name in enumerate(edges):
        pre = f"edge{n}_{name}_"
        for k in STAT_NAMES:
            ref = golden_rows[pre + k]
            g = got[k][3 * j + 1:3 * j + 2]
            if k in COUNT_NAMES:
                assert int(g[0]) == int(ref[0]), (name, k, int(g[0]), int(ref[0]))
            elif k in EXACT_NAMES:
                assert same(g, ref), (name, k, g, ref)
            elif k not in ("skewness", "kurtosis") or abs(ref[0]) >= 1e-3 or ref[0] == 0:
                # (a third or fourth moment that all but cancels has no digits to compare:
                # the fixtures' own criterion, tests/golden/make_golden_stats.py)
                assert f32_ulps(g, ref).max() <= 1, (name, k, g, ref)
            # the neighbours are unaffected
            assert same(got[k][3 * j:3 * j + 1], alone[k][0:1]) and same(got[k][3 * j + 2:3 * j + 3], alone[k][1:2])
    c = 3 * list(edges).index("const") + 1
    assert got["var"][c] == 0 and got["skewness"][c] == 0 and got["kurtosis"][c] == 0
    z = 3 * list(edges).index("zeros") + 1
    assert np.isposinf(got["crest"][z]) and got["rms"][z] == 0
    f = 3 * list(edges).index("nan_first") + 1
    assert np.isnan(got["min"][f]) and np.isnan(got["max"][f]) and got["argmin"][f] == 0 and got["argmax"][f] == 0
    t = 3 * list(edges).index("ties") + 1
    assert (got["argmax"][t], got["argmin"][t]) == (64, 63)
    for name, sign in (("zeros_pm", 0), ("zeros_mp", 1)):
        i = 3 * list(edges).index(name) + 1
        assert got["argmin"][i] == 0 and got["argmax"][i] == 0
        assert np.signbit(got["min"][i]) == bool(sign) and np.signbit(got["max"][i]) == bool(sign)
    i = 3 * list(edges).index("zero_min") + 1
    assert got["argmin"][i] == 63 and np.signbit(got["min"][i])
    i = 3 * list(edges).index("zero_max") + 1
    assert got["argmax"][i] == 63 and not np.signbit(got["max"][i]) and got["max"][i] == 0


# ---------------------------------------------------------------- 3. masks, host calls
@pytest.mark.parametrize("long_route", [0, 1])
def test_mask_independence(vdev, knob, long_route):
    if long_route:
        knob("STATS_LONG", 1)
    for n in (5, 400, 4097):
        x = dev(batch_rows(n, 9))
        full = host(vdev.stats(x, STAT_NAMES))
        for name in STAT_NAMES:
            one = host(vdev.stats(x, (name,)))
            assert list(one) == [name] and same(one[name], full[name]), (n, name)
        energy = host(vdev.stats(x, ENERGY_NAMES))
        for name in ENERGY_NAMES:
            assert same(energy[name], full[name]), (n, name)


def test_no_output_launches_nothing(vdev, counters):
    assert vdev.stats(dev(batch_rows(64, 3)), ()) == {}
    assert counters() == (0, 0)


def test_host_calls_equal_the_batch_row(vdev, amd):
    api = StatsApi(amd.lib)
    for n in (1, 4, 65, 400, 4097, LONG_N):
        x = long_row()[:n] if n == LONG_N else batch_rows(n, SLICES)[4]
        names = valid_names(n)
        batch = host(vdev.stats(dev(x[None, :]), names))
        for name in names:
            st, v = api.stat(name, x)
            assert st == OK, (n, name, st)
            if name in COUNT_NAMES:
                assert v == int(batch[name][0]), (n, name)
            else:
                assert same(np.array([v], np.float32), batch[name]), (n, name)
        st, mn, mx = api.peak(x)
        assert st == OK and same(np.array([mn, mx]), np.array([batch["min"][0], batch["max"][0]]))
        st, mn, mx = api.peak(x, False, True)
        assert st == OK and mn == SENTINEL and same(np.array([mx]), batch["max"])
    for name, least in MIN_LEN.items():
        st, v = api.stat(name, long_row()[:least - 1])
        assert st == ERR_SIZE and v == 0


# ---------------------------------------------------------------- 4. frames
@pytest.fixture(scope="module")
def three_channels():
    return frames_util.three_channels(*signals())


@pytest.mark.parametrize("windowed", [0, 1])
@pytest.mark.parametrize("center", [0, 1])
@pytest.mark.parametrize("frame,hop", [(400, 160), (33, 7), (64, 64), (600, 200), (4100, 1000), (1, 1)])
def test_stats_frames_is_the_pipeline(vdev, three_channels, counters, frame, hop, center, windowed):
    import torch
    sig = three_channels
    assert sig.stride(0) == 16004
    names = valid_names(frame)        # (1, 1): the mask that n = 1 allows
    win = dev(hamming(frame)) if windowed else None
    got = vdev.stats_frames(sig, frame, hop, names, window=win, center=bool(center))
    assert counters() == (1, 0)
    fr = vdev.num_frames(16000, frame, hop, center)
    assert fr > 3 and all(got[k].shape == (3, fr) for k in names)
    for c in range(3):
        rows = fetch_frames(vdev, sig[c].contiguous(), frame, hop, center, win)
        want = vdev.stats(rows, names)
        for k in names:
            assert torch.equal(got[k][c].view(torch.int32), want[k].view(torch.int32)), (c, k)


def test_stats_frames_long_route(vdev, three_channels, knob, counters):
    import torch
    knob("STATS_LONG", 1)
    got = vdev.stats_frames(three_channels, 4100, 1000, STAT_NAMES, center=True)
    assert counters() == (0, 1)
    knob("STATS_LONG", None)
    want = vdev.stats_frames(three_channels, 4100, 1000, STAT_NAMES, center=True)
    for k in STAT_NAMES:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k


def test_stats_frames_zero_frames_and_sizes(vdev, three_channels):
    import torch
    L = vdev.lib()
    sig = three_channels
    planes = torch.full((12, 3, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    full = vdev.StatsOut()
    for i, name in enumerate(STAT_NAMES):
        setattr(full, name, planes[i].data_ptr())

    def call(n, frame, hop, center, out=full):
        return L.vv_dsp_stats_frames_device(sig.data_ptr(), n, 3, 16004, frame, hop, center, None, C.byref(out), 4, s)

    assert call(100, 400, 160, 0) == OK                 # zero frames: nothing written
    assert call(16000, 400, 0, 0) == ERR_SIZE
    assert call(16000, 0, 160, 0) == ERR_SIZE
    assert call(16000, 3, 4000, 0) == ERR_SIZE          # kurtosis needs 4 samples: nothing written at all
    assert call(16000, 1, 4000, 0) == ERR_SIZE
    assert call(16000, 400, 4000, 0, vdev.StatsOut()) == OK   # nothing wanted
    torch.cuda.synchronize()
    assert torch.all(planes == float(SENTINEL))
    assert L.vv_dsp_stats_device(sig.data_ptr(), 3, 3, 16004, C.byref(full), s) == ERR_SIZE
    torch.cuda.synchronize()
    assert torch.all(planes == float(SENTINEL))
    assert call(16000, 400, 4000, 0) == OK              # 4 frames per channel fill the planes
    torch.cuda.synchronize()
    assert not torch.any(planes == float(SENTINEL))


# ---------------------------------------------------------------- 5. correlations
@pytest.mark.parametrize("biased", [0, 1])
@pytest.mark.parametrize("n,r_len", AUTO_CASES)
def test_autocorrelation(vdev, amd, golden_corr, n, r_len, biased):
    white = signals()[0]
    ref = golden_corr[f"auto_{n}_{r_len}_{biased}"]
    x = np.stack([white[:n], white[40:40 + n], white[:n]])
    r = vdev.autocorrelation(dev(x), r_len, biased=bool(biased)).cpu().numpy()
    assert r.shape == (3, r_len)
    u = f32_ulps(r[0], ref)
    print(f"autocorrelation {n} {r_len} {biased}: {int(np.sum(u != 0))} of {u.size} not bit-identical")
    assert u.max() <= 1
    assert same(r[0], r[2])
    assert np.all(bits(r[:, n:]) == 0)                  # no overlap: exactly +0
    st, rh = StatsApi(amd.lib).autocorrelation(white[:n], r_len, biased)
    assert st == OK and same(rh, r[0])


@pytest.mark.parametrize("nx,ny,r_len", CROSS_CASES)
def test_cross_correlation(vdev, amd, golden_corr, nx, ny, r_len):
    white, resonant = signals()
    ref = golden_corr[f"cross_{nx}_{ny}_{r_len}"]
    x = np.stack([white[:nx], white[7:7 + nx]])
    y = np.stack([resonant[:ny], resonant[7:7 + ny]])
    r = vdev.cross_correlation(dev(x), dev(y), r_len).cpu().numpy()
    u = f32_ulps(r[0], ref)
    print(f"cross_correlation {nx} {ny} {r_len}: {int(np.sum(u != 0))} of {u.size} not bit-identical")
    assert u.max() <= 1
    assert np.all(bits(r[:, ny:]) == 0)
    st, rh = StatsApi(amd.lib).cross_correlation(white[:nx], resonant[:ny], r_len)
    assert st == OK and same(rh, r[0])


# ---------------------------------------------------------------- 6. binding checks
def test_binding_checks(vdev):
    import torch
    x = dev(batch_rows(64, 4))
    bad = [lambda: vdev.stats(x.double(), ("rms",)),
           lambda: vdev.stats(x.cpu(), ("rms",)),
           lambda: vdev.stats(x[:, ::2], ("rms",)),                       # sample stride 2
           lambda: vdev.stats(x, ("rms", "median")),                       # unknown name
           lambda: vdev.stats(x[:, :3], ("kurtosis",)),                    # size rule
           lambda: vdev.stats(x[:, :2], ("skewness",)),
           lambda: vdev.stats(x[:, :1], ("var",)),
           lambda: vdev.stats(x.reshape(2, 2, 64), ("rms",)),
           lambda: vdev.stats_frames(x, 16, 8, ("rms",), window=dev(hamming(15))),
           lambda: vdev.stats_frames(x, 16, 0, ("rms",)),
           lambda: vdev.stats_frames(x, 0, 8, ("rms",)),
           lambda: vdev.stats_frames(x, 3, 1, ("kurtosis",)),
           lambda: vdev.stats_frames(x.double(), 16, 8, ("rms",)),
           lambda: vdev.stats_frames(x[:, ::2], 16, 8, ("rms",)),
           lambda: vdev.autocorrelation(x, 0),
           lambda: vdev.autocorrelation(x.double(), 4),
           lambda: vdev.cross_correlation(x, x[:2], 4),
           lambda: vdev.cross_correlation(x, x.double(), 4),
           lambda: vdev.cross_correlation(x, x, 0)]
    for i, call in enumerate(bad):
        with pytest.raises(vdev.VvError):
            call()
            pytest.fail(f"case {i} passed the checks")
    got = vdev.stats(x, ("zero_crossings", "argmin", "rms"))
    assert got["zero_crossings"].dtype == torch.int32 and got["argmin"].dtype == torch.int32
    assert got["rms"].dtype == torch.float32
    one = vdev.stats(x[0], "rms")
    assert one["rms"].dim() == 0 and one["rms"] == got["rms"][0]
