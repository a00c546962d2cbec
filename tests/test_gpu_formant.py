"""Formants of LPC rows on the GPU (include/vv_dsp/features/formant.h,
csrc/hip/formant_kernels.hip) against the numpy model of the definition
(tests/formant_util.py; the CPU suite holds its two forms equal on the same case
table).  The roots plane, flags and counts are compared bit for bit: the
iteration has no library call and no sum whose order is free.  freq and bw are
compared as equal or adjacent floats, because the device's atan2 / log and
numpy's may differ in the last f64 bit; the NaN fills bit for bit.  No case is
left out of a comparison."""
import ctypes as C

import numpy as np
import pytest

import formant_util as fu
import lpc_util
import lsf_util as lu
from frames_util import hamming

pytestmark = pytest.mark.gpu

POISON = np.float32(-7.0e7)
NAMES = ("freq", "bw", "count", "flags", "roots")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(planes):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


def vv_params(vv, p):
    return vv.FormantParams(*(getattr(p, f) for f, _ in p._fields_))


@pytest.fixture(scope="module")
def table(amd_lib_path):
    api = fu.FormantApi(amd_lib_path)
    prm = fu.default_params()
    out = {}
    for p in lu.ORDERS:
        cs = lu.cases(p)
        names = list(cs)
        A = np.stack([cs[n] for n in names])
        out[p] = dict(names=names, A=A, model=fu.formants_vec(A, api.start(p), prm))
    return out


TALLY = {"freq": [0, 0], "bw": [0, 0]}


def compare(got, want, what):
    lu.assert_bits(got["roots"], want["roots"], (what, "roots"))
    lu.assert_bits(got["flags"], want["flags"], (what, "flags"))
    lu.assert_bits(got["count"], want["count"], (what, "count"))
    tally = {}
    for k in ("freq", "bw"):
        tally[k] = lu.assert_adjacent(got[k], want[k], (what, k))
    return tally


@pytest.mark.parametrize("p", lu.ORDERS)
def test_cases_equal_the_model(vdev, table, p):
    """Every row of the case table at order p, default parameters, and with n_formants 1 and 16
    and a narrowed band.  Observed on the MI355X over the eight orders (default parameters):
    all 127 kept freq values and all 127 bw values exact, none one ulp off."""
    t = table[p]
    vdev.debug_clear("STAT_FORMANT")
    prm = fu.default_params()
    got = host(vdev.formants(dev(t["A"]), vv_params(vdev, prm), NAMES))
    assert vdev.debug_get("STAT_FORMANT") == 1
    tally = compare(got, t["model"], p)
    for k in TALLY:
        TALLY[k][0] += tally[k][0]
        TALLY[k][1] += tally[k][1]
    print(f"order {p}: running tally (exact, 1 ulp) {TALLY}")
    start = np.asarray(vdev.formant_start_points(p).numpy())
    for kw in (dict(n_formants=1), dict(n_formants=16), dict(f_min=900.0, f_max=3000.0, bw_max=250.0, n_formants=3)):
        q = fu.default_params(**kw)
        compare(host(vdev.formants(dev(t["A"]), vv_params(vdev, q), NAMES)), fu.formants_vec(t["A"], start, q),
                (p, tuple(kw)))


def batch_rows(t, n):
    """n rows: the slowest converging row next to the fastest and next to one that does not
    converge, a NaN row between two ordinary rows, then the table in turn"""
    names, it, fl = t["names"], t["model"]["iters"], t["model"]["flags"]
    conv = [i for i in range(len(names)) if fl[i] and it[i] > 0]
    slow, fast = max(conv, key=lambda i: it[i]), min(conv, key=lambda i: it[i])
    stuck = names.index("double")
    front = [slow, fast, slow, stuck, slow, names.index("nan"), names.index("white0")]
    order = front + [i for i in range(len(names))]
    return [order[i % len(order)] for i in range(n)]


@pytest.mark.parametrize("p", lu.ORDERS)
def test_rows_are_independent(vdev, amd_lib_path, table, p):
    """bit for bit, freq and bw included: a row alone, inside batches of 1, 7 and 65 rows (more
    than a workgroup holds at any order), at another pitch, each output alone, and through the
    host call"""
    t = table[p]
    A = t["A"]
    prm = vv_params(vdev, fu.default_params())
    alone = [host(vdev.formants(dev(A[r:r + 1]), prm, NAMES)) for r in range(len(A))]
    if p >= 8:
        assert t["model"]["flags"][t["names"].index("double")] == 0      # the row that does not converge
    for n in (1, 7, 65):
        idx = batch_rows(t, n)
        got = host(vdev.formants(dev(A[idx]), prm, NAMES))
        wide = np.full((n, p + 6), POISON, np.float32)
        wide[:, :p + 1] = A[idx]
        dw = dev(wide)
        pitched = host(vdev.formants(dw[:, :p + 1], prm, NAMES))
        assert np.array_equal(dw.cpu().numpy().view(np.uint32), wide.view(np.uint32))
        singles = {k: host(vdev.formants(dev(A[idx]), prm, k))[k] for k in NAMES}
        for j, r in enumerate(idx):
            for k in NAMES:
                lu.assert_bits(got[k][j], alone[r][k][0], (k, n, j))
                lu.assert_bits(pitched[k][j], alone[r][k][0], (k, "pitch", n, j))
                lu.assert_bits(singles[k][j], alone[r][k][0], (k, "alone", n, j))
    api = fu.FormantApi(amd_lib_path)
    for r in range(len(A)):
        st, res = api.formants(A[r], fu.default_params())
        assert st == 0
        for k in NAMES:
            lu.assert_bits(res[k].reshape(alone[r][k][0].shape), alone[r][k][0], ("host", k, r))
        st, res = api.formants(A[r], fu.default_params(), want=("count",))
        assert st == 0 and res["count"][0] == alone[r]["count"][0]
        assert np.all(res["freq"] == -123.0) and np.all(res["roots"] == -123.0) and res["flags"][0] == -77


@pytest.mark.parametrize("nch", (1, 3))
@pytest.mark.parametrize("center", (False, True))
@pytest.mark.parametrize("windowed", (False, True))
def test_frames_equal_the_two_calls(vdev, knob, nch, center, windowed):
    """formant_frames == lpc_frames followed by formants, bit for bit, with channel groups of 1
    and of more than nch, and each output alone; the fixture's frames give its four formants"""
    fx = fu.load_fixture()["signal"]
    sig = lpc_util.load("lpc_signals")
    x = np.stack([fx[:2000], sig["resonant"][:2000], fx[2000:]])[:nch]
    dx = dev(x)
    win = dev(hamming(400).astype(np.float32)) if windowed else None
    order = 12
    prm = vv_params(vdev, fu.default_params(n_formants=4))
    a, _ = vdev.lpc_frames(dx, 400, 160, order, window=win, center=center)
    fr = a.shape[1]
    want = host(vdev.formants(a.reshape(nch * fr, order + 1), prm, NAMES))
    want = {k: v.reshape((nch, fr) + v.shape[1:]) for k, v in want.items()}
    for group in (1, 5):
        knob("LSF_GROUP", group)
        vdev.debug_clear("STAT_FORMANT")
        got = host(vdev.formant_frames(dx, 400, 160, order, prm, NAMES, window=win, center=center))
        assert vdev.debug_get("STAT_FORMANT") == (nch if group == 1 else 1)
        for k in NAMES:
            lu.assert_bits(got[k], want[k], (k, group))
        for k in NAMES:
            lu.assert_bits(host(vdev.formant_frames(dx, 400, 160, order, prm, k, window=win, center=center))[k],
                           want[k], (k, "alone", group))
    if windowed and not center:
        # whole Hamming frames of the fixture: the design's formants (bound: test_formant_host.py)
        assert np.all(want["count"][0] == 4) and np.all(want["flags"][0] == fu.CONVERGED)
        design = np.array([f for f, _ in fu.FIXTURE_FORMANTS])
        assert np.abs(want["freq"][0].astype(np.float64) - design).max() < 72.5


def test_zero_frames_write_nothing(vdev):
    import torch
    x = dev(np.zeros((2, 300), np.float32))
    bufs = [torch.full((64,), float(POISON), dtype=torch.float32, device="cuda") for _ in range(5)]
    out = vdev.FormantOut(*(b.data_ptr() for b in bufs))
    prm = vv_params(vdev, fu.default_params())
    st = vdev.lib().vv_dsp_formants_frames_device(C.c_void_p(x.data_ptr()), 300, 2, 300, 400, 160, 0, None, 12,
                                                  C.byref(prm), C.byref(out), None)
    torch.cuda.synchronize()
    assert st == 0
    for b in bufs:
        assert np.all(b.cpu().numpy() == POISON)
    planes = vdev.formant_frames(x, 400, 160, 12, prm, NAMES)
    assert planes["freq"].shape == (2, 0, 5) and planes["roots"].shape == (2, 0, 12, 2)


def test_counter_counts_launches(vdev, table):
    t = table[16]
    prm = vv_params(vdev, fu.default_params())
    vdev.debug_clear("STAT_FORMANT")
    for i in range(1, 4):
        vdev.formants(dev(t["A"]), prm, "count")
        assert vdev.debug_get("STAT_FORMANT") == i
    assert vdev.formants(dev(np.zeros((0, 17), np.float32)), prm, "count")["count"].shape == (0,)
    assert vdev.debug_get("STAT_FORMANT") == 3
