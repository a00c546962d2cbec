"""GPU tests of the running median (include/vv_dsp/filter/median.h) against the numpy
model of tests/median_util.py.  Selection returns one of its inputs, so every comparison
is of uint32 bit patterns and exact: ties, signed zeros, infinities, denormals and NaNs
of both signs with payloads included.  Batches are three rows with strides above n: the
input pads hold a value that would change a median if it were read (+inf next to rows of
small numbers), the output pads a sentinel that must survive."""
import numpy as np
import pytest
import torch

import median_util as mu

pytestmark = pytest.mark.gpu

PAD_IN, PAD_OUT = np.float32(np.inf), np.float32(-12345.0)
MODES = (mu.REFLECT, mu.NEAREST, mu.ZERO)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_padded(vv, x, Lw, mode, pad_in=5, pad_out=3):
    """x (batch, n) through views of wider buffers; returns (rows, output pads)"""
    b, n = x.shape
    xin = np.full((b, n + pad_in), PAD_IN, np.float32)
    xin[:, :n] = x
    dx = dev(xin)
    dy = torch.full((b, n + pad_out), float(PAD_OUT), dtype=torch.float32, device="cuda")
    vv.medfilt(dx[:, :n], Lw, mode, out=dy[:, :n])
    y = dy.cpu().numpy()
    assert np.array_equal(mu.bits(dx.cpu().numpy()), mu.bits(xin)), "the input changed"
    return y[:, :n], y[:, n:]


@pytest.mark.parametrize("n", mu.MEDFILT_N)
def test_rows_equal_the_model(vdev, n):
    x = mu.medfilt_rows(n, n)
    for Lw in mu.MEDFILT_L:
        for mode in MODES:
            want = mu.median_sort(x, Lw, mode)
            got, pads = run_padded(vdev, x, Lw, mode)
            assert np.array_equal(mu.bits(got), mu.bits(want)), (n, Lw, mode)
            assert np.all(pads == PAD_OUT), (n, Lw, mode)
            # a row filtered alone, packed, equals the same row inside the batch
            alone = vdev.medfilt(dev(x[1]), Lw, mode).cpu().numpy()
            assert np.array_equal(mu.bits(alone), mu.bits(want[1])), (n, Lw, mode)


@pytest.mark.parametrize("Lw", (5, 31, 33, 127))
def test_both_selects_give_the_same_bits(vdev, Lw):
    x = mu.medfilt_rows(1000, 77)
    want = mu.median_sort(x, Lw, mu.REFLECT)
    for select in (1, 2):
        with vdev.knobs(MEDIAN_SELECT=select):
            got = vdev.medfilt(dev(x), Lw).cpu().numpy()
        assert np.array_equal(mu.bits(got), mu.bits(want)), (Lw, select)


def test_host_entry_equals_device_entry(vdev):
    L = vdev.lib()
    for n, Lw, mode in ((5, 31, mu.REFLECT), (1000, 5, mu.ZERO), (4099, 127, mu.NEAREST), (65, 33, mu.REFLECT)):
        x = mu.medfilt_rows(n, 3 * n, batch=1)[0]
        y = np.full(n, PAD_OUT, np.float32)
        assert L.vv_dsp_medfilt(x.ctypes.data, n, Lw, mode, y.ctypes.data) == 0
        d = vdev.medfilt(dev(x), Lw, mode).cpu().numpy()
        assert np.array_equal(mu.bits(y), mu.bits(d)), (n, Lw, mode)
        assert np.array_equal(mu.bits(y), mu.bits(mu.median_sort(x, Lw, mode))), (n, Lw, mode)


def test_despikes_an_f0_plane(vdev):
    """what the filter is for: single-frame octave errors in a pitch plane are removed and
    every other frame is returned as it was"""
    f0 = np.full((2, 400), 220.0, np.float32)
    f0[1] = np.linspace(180, 260, 400, dtype=np.float32)
    clean = f0.copy()
    f0[:, 50::37] *= 2.0
    got = vdev.medfilt(dev(f0), 3, mu.NEAREST).cpu().numpy()
    assert np.array_equal(got[0], clean[0])
    far = np.ones(400, bool)
    for d in (-1, 0, 1):
        far[np.clip(np.arange(50, 400, 37) + d, 0, 399)] = False
    assert np.array_equal(got[1][far], clean[1][far]) and np.all(got[1] < 270)


def test_binding_refuses_bad_arguments(vdev):
    x = torch.zeros((2, 16), dtype=torch.float32, device="cuda")
    for Lw, mode in ((4, 0), (0, 0), (3, 5), (129, 0)):
        with pytest.raises(vdev.VvError):
            vdev.medfilt(x, Lw, mode)
    with pytest.raises(vdev.VvError):
        vdev.medfilt(x, 3, out=torch.zeros((2, 15), dtype=torch.float32, device="cuda"))
    with pytest.raises(vdev.VvError):
        vdev.medfilt(x.double(), 3)
