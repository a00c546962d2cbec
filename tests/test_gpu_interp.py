"""GPU tests of the interpolation kernel (interp_kernels.hip, shim_interp.hip)
against the reference's outputs in tests/golden/interp_ref.npz and the float32
model of tests/interp_util.py (which equals the reference bit for bit on every
recorded value, tests/test_interp_host.py).

Everything is compared bit for bit: the kernel does the reference's float32
operations in the reference's order with every product and sum rounded on its
own, so there is no tolerance.  Where a row holds a NaN sample, any NaN equals
any NaN.
"""
import ctypes as C

import numpy as np
import pytest

from interp_util import (InterpApi, load, model, same, row, special_row, positions, warp_positions, uniform_positions,
                         signals, METHODS, ROW_N, SPECIAL_N, LINEAR, CUBIC, OK)

pytestmark = pytest.mark.gpu

SENT = 7.5


@pytest.fixture(scope="module")
def golden():
    return load("interp_ref")


@pytest.fixture(scope="module")
def cases():
    """(key, row, positions) of every recorded case"""
    c = [(f"n{n}", row(n), positions(n)) for n in ROW_N]
    return c + [(kind, special_row(kind), positions(SPECIAL_N)) for kind in ("inf", "nan")]


@pytest.fixture(scope="module")
def long_signal():
    """[5][1031] float32 rows of the fixtures' signals"""
    white, resonant = signals()
    return np.stack([(white, resonant)[r % 2][700 * r:700 * r + 1031] for r in range(5)]).astype(np.float32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def padded(rows, width, pad):
    """(buffer, view): `rows` rows of `width` floats, width + pad floats apart, starting one
    float into a buffer filled with SENT"""
    import torch
    buf = torch.full((1 + rows * (width + pad),), SENT, dtype=torch.float32, device="cuda")
    return buf, buf[1:].as_strided((rows, width), (width + pad, 1))


def only_view_written(buf, rows, width, pad):
    b = host(buf)
    grid = b[1:].reshape(rows, width + pad)
    return b[0] == SENT and bool(np.all(grid[:, width:] == SENT))


# ---------------------------------------------------------------- 1. the reference's values
@pytest.mark.parametrize("method", METHODS)
def test_golden_through_device_tensors(vdev, golden, cases, method):
    for key, x, pos in cases:
        y = host(vdev.interpolate(dev(x), dev(pos), method))
        want = golden[f"{key}_{method}"]
        finite = np.isfinite(want)
        assert same(y[finite], want[finite]), (key, method)
        assert same(y, want, nan_equal=True), (key, method)


@pytest.mark.parametrize("method", METHODS)
def test_golden_through_host_batch(vdev, golden, cases, method):
    fn = vdev.lib().vv_dsp_interpolate_real_batch
    for key, x, pos in cases:
        y = np.full(len(pos), SENT, np.float32)
        assert fn(x.ctypes.data, len(x), pos.ctypes.data, len(pos), METHODS.index(method), y.ctypes.data) == OK
        assert same(y, golden[f"{key}_{method}"], nan_equal=True), (key, method)


def test_golden_through_scalar_functions(amd, golden):
    api = InterpApi(amd.lib)
    count = 0
    for n in (1, 2, 5, 257):
        x, pos = row(n), positions(n)
        for method in METHODS:
            want = golden[f"n{n}_{method}"]
            for k in range(3, len(pos), len(pos) // 6):
                st, v = api.one(method, x, pos[k])
                assert st == OK and same([v], [want[k]]), (n, method, float(pos[k]))
                count += 1
    assert count >= 36
    got = api.argument_cases(device=True)
    want = dict(zip((str(s) for s in golden["arg_names"]), (int(s) for s in golden["arg_status"])))
    assert got == want


# ---------------------------------------------------------------- 2. batches, strides, offsets
@pytest.mark.parametrize("method", METHODS)
def test_strided_batches(vdev, long_signal, method):
    import torch
    b, n = long_signal.shape
    m = vdev.interp_run_length() + 1
    xbuf, x = padded(b, n, 3)
    x.copy_(dev(long_signal))
    per_row = np.stack([warp_positions(n, m, ("warp", "reverse", "random", "warp", "random")[r], seed=r)
                        for r in range(b)])
    pbuf = torch.full((1 + b * m,), SENT, dtype=torch.float32, device="cuda")
    pos = pbuf[1:].view(b, m)
    pos.copy_(dev(per_row))

    # one row of positions shared by every signal row
    obuf, out = padded(b, m, 5)
    vdev.interpolate(x, pos[0], method, out=out)
    shared = host(out)
    for r in range(b):
        assert same(shared[r], model(long_signal[r], per_row[0], method)), r
        assert same(host(vdev.interpolate(x[r], pos[0], method)), shared[r]), r         # the batch = 1 call
    assert only_view_written(obuf, b, m, 5)

    # one row of positions per signal row
    obuf, out = padded(b, m, 5)
    vdev.interpolate(x, pos, method, out=out)
    rows = host(out)
    for r in range(b):
        assert same(rows[r], model(long_signal[r], per_row[r], method)), r
        assert same(host(vdev.interpolate(x, pos[r], method))[r], rows[r]), r           # the shared call
    assert only_view_written(obuf, b, m, 5)
    assert np.all(host(xbuf)[1:].reshape(b, n + 3)[:, n:] == SENT) and same(host(x), long_signal)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["warp", "reverse", "const", "random"])
def test_run_boundaries(vdev, knob, long_signal, method, kind):
    R = vdev.interp_run_length()
    x = long_signal[:2, :777]
    dx = dev(x)
    for m in (1, R - 1, R, R + 1, 2 * R + 3):
        pos = warp_positions(777, m, kind, seed=m)
        want = np.stack([model(x[r], pos, method) for r in range(2)])
        for one_row in (None, 1):                 # both routes of a shared position array
            knob("INTERP_ROWS", one_row)
            y = host(vdev.interpolate(dx, dev(pos), method))
            assert y.shape == (2, m) and same(y, want), (m, one_row)


# ---------------------------------------------------------------- 3. uniform positions
@pytest.mark.parametrize("method", METHODS)
def test_uniform_equals_explicit(vdev, long_signal, method):
    b, n = 3, long_signal.shape[1]
    x = long_signal[:b]
    dx = dev(x)
    m = 2 * vdev.interp_run_length() + 3
    for start, step in ((0.0, 1.0), (0.0, 1.0 / 3.0), (-1.5, 0.918), (float(n - 1), -1.0), (2.25, 0.0)):
        pos = uniform_positions(start, step, m)
        got = host(vdev.interpolate_uniform(dx, start, step, m, method))
        assert same(got, host(vdev.interpolate(dx, dev(pos), method))), (start, step)
        for r in range(b):
            assert same(got[r], model(x[r], pos, method)), (start, step, r)


# ---------------------------------------------------------------- 4. a row longer than 2^24
def test_row_beyond_2_to_24(vdev):
    """floats above 2^24 are 2 apart: the index and the fraction must come out as the
    reference's float32 arithmetic gives them"""
    n = (1 << 24) + 5
    rng = np.random.default_rng(24)
    x = np.zeros(n, np.float32)
    x[-4096:] = rng.uniform(-0.5, 0.5, 4096).astype(np.float32)
    pos = rng.uniform(n - 64.0, n + 1.0, 3000).astype(np.float32)
    pos = np.concatenate([pos, np.arange(n - 64, n + 2).astype(np.float32),
                          np.float32(1 << 24) + np.arange(-6, 7, dtype=np.float32) * np.float32(0.5)])
    dx, dp = dev(x), dev(pos)
    for method in METHODS:
        assert same(host(vdev.interpolate(dx, dp, method)), model(x, pos, method)), method
    m = 200
    start, step = float(n - 150), 0.75
    up = uniform_positions(start, step, m)
    assert same(host(vdev.interpolate_uniform(dx, start, step, m, "cubic")), model(x, up, "cubic"))


# ---------------------------------------------------------------- 5. NaN positions
@pytest.mark.parametrize("method", METHODS)
def test_nan_position_gives_nan_and_nothing_else(vdev, long_signal, method):
    x = long_signal[:2]
    pos = warp_positions(x.shape[1], 700, "warp")
    clean = host(vdev.interpolate(dev(x), dev(pos), method))
    at = [0, 63, 64, 300, 699]
    bad = pos.copy()
    bad[at] = np.nan
    y = host(vdev.interpolate(dev(x), dev(bad), method))
    keep = np.ones(700, bool)
    keep[at] = False
    assert np.all(np.isnan(y[:, at])) and same(y[:, keep], clean[:, keep])
    assert same(y[0], model(x[0], bad, method), nan_equal=True)
    # the cubic's n < 2 rule comes before the position, as in the reference
    one = host(vdev.interpolate(dev(x[0, :1]), dev(bad[:70]), method))
    assert same(one, model(x[0, :1], bad[:70], method), nan_equal=True)


# ---------------------------------------------------------------- 6. the rows route
@pytest.mark.parametrize("method", METHODS)
def test_rows_routes_agree(vdev, knob, long_signal, method):
    """One position array for every row: a workgroup takes its run through 8 signal rows,
    or through one with knob INTERP_ROWS = 1 -- the same bits, the batch (5 and 13) not
    a multiple of 8.  Every other call takes one row per workgroup."""
    x = long_signal
    dx = dev(x)
    m = vdev.interp_run_length() + 37
    pos = warp_positions(x.shape[1], m, "random", seed=5)
    pos[[1, 70]] = np.nan
    dp = dev(pos)
    per_row = dev(np.stack([pos] * x.shape[0]))

    def count():
        got = vdev.debug_get("STAT_INTERP_ONE"), vdev.debug_get("STAT_INTERP_ROWS")
        vdev.debug_clear("STAT_INTERP_ONE")
        vdev.debug_clear("STAT_INTERP_ROWS")
        return got

    count()
    knob("INTERP_ROWS", 1)
    want = host(vdev.interpolate(dx, dp, method))
    assert count() == (1, 0)
    for r in range(x.shape[0]):
        assert same(want[r], model(x[r], pos, method), nan_equal=True), r
    knob("INTERP_ROWS", None)
    assert same(host(vdev.interpolate(dx, dp, method)), want, nan_equal=True)
    assert count() == (0, 1)
    x13 = dev(np.concatenate([x, x[::-1], x[:3]]))
    got = host(vdev.interpolate(x13, dp, method))
    assert count() == (0, 1)
    assert same(got, np.concatenate([want, want[::-1], want[:3]]), nan_equal=True)
    # per-row positions, single rows and uniform positions always take one row per workgroup
    assert same(host(vdev.interpolate(dx, per_row, method)), want, nan_equal=True)
    assert same(host(vdev.interpolate(dx[0], dp, method)), want[0], nan_equal=True)
    vdev.interpolate_uniform(dx, -3.0, 0.77, m, method)
    assert count() == (3, 0)


# ---------------------------------------------------------------- 7. every entry point, one value
def test_entry_points_agree(vdev, long_signal):
    x = long_signal[0]
    m = 300
    pos = uniform_positions(-1.0, 3.5, m)
    for method in METHODS:
        a = host(vdev.interpolate(dev(x), dev(pos), method))
        b = host(vdev.interpolate_uniform(dev(x), -1.0, 3.5, m, method))
        c = np.full(m, SENT, np.float32)
        assert vdev.lib().vv_dsp_interpolate_real_batch(x.ctypes.data, len(x), pos.ctypes.data, m,
                                                        METHODS.index(method), c.ctypes.data) == OK
        d = host(vdev.interpolate(dev(np.stack([x, x])), dev(np.stack([pos, pos])), method))
        assert same(a, b) and same(a, c) and same(a, d[0]) and same(a, d[1]) and same(a, model(x, pos, method))
