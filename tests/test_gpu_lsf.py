"""LPC <-> LSF and reflection coefficients on the GPU (include/vv_dsp/envelope/lsf.h,
csrc/hip/lsf_kernels.hip) against the numpy model of the definition
(tests/lsf_util.py; the CPU suite holds its two forms equal on the same case
table).  rc, flags, the NaN fills and the a of lsf_to_lpc (whose cosine the header
defines by arithmetic alone) are compared bit for bit; lsf as equal or adjacent
floats, because the device's acos and numpy's may differ in the last f64 bit.
No case is left out of a comparison."""
import ctypes as C

import numpy as np
import pytest

import lpc_util
import lsf_util as lu
from frames_util import hamming

pytestmark = pytest.mark.gpu

POISON = np.float32(-7.0e7)
POISON_I = 0x5A5A5A5A


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(planes):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


@pytest.fixture(scope="module")
def table():
    x = lu.grid()
    out = {}
    for p in lu.ORDERS:
        cs = lu.cases(p)
        names = list(cs)
        A = np.stack([cs[n] for n in names])
        lsf, rc, flags = lu.lpc_to_lsf_vec(A, x)
        # the way back: the model's own lsf rows (NaN rows among them), plus a row of +inf
        back_in = np.concatenate([lsf, np.full((1, p), np.inf, np.float32)])
        out[p] = dict(names=names, A=A, lsf=lsf, rc=rc, flags=flags, back_in=back_in, back=lu.lsf_to_lpc_vec(back_in))
    return out


TALLY = {"lsf": [0, 0]}


@pytest.mark.parametrize("p", lu.ORDERS)
def test_cases_equal_the_model(vdev, table, p):
    """Every row of the case table at order p.  Observed on the MI355X over the eight orders:
    all 1042 finite lsf values exact, none one ulp off; every a of lsf_to_lpc bit-equal."""
    t = table[p]
    vdev.debug_clear("STAT_LSF")
    got = host(vdev.lpc_to_lsf(dev(t["A"])))
    assert vdev.debug_get("STAT_LSF") == 1
    lu.assert_bits(got["rc"], t["rc"], "rc")
    lu.assert_bits(got["flags"], t["flags"], "flags")
    e, u = lu.assert_adjacent(got["lsf"], t["lsf"], "lsf")
    TALLY["lsf"][0] += e
    TALLY["lsf"][1] += u
    back = host(vdev.lsf_to_lpc(dev(t["back_in"])))["a"]
    assert vdev.debug_get("STAT_LSF") == 2
    assert np.all(back[:, 0] == 1.0)
    lu.assert_bits(back, t["back"], "a")
    print(f"order {p}: running tally (exact, 1 ulp) {TALLY}")


def batch_rows(t, n):
    """n rows cycling through the table with a NaN row between two ordinary rows at the front"""
    names = t["names"]
    first = [names.index("resonant0"), names.index("nan"), names.index("white0")]
    order = first + [i for i in range(len(names)) if i not in first]
    return [order[i % len(order)] for i in range(n)]


@pytest.mark.parametrize("p", lu.ORDERS)
def test_rows_are_independent(vdev, amd_lib_path, table, p):
    """bit for bit: a row alone, inside batches of 1, 7 and 65 rows (more than a workgroup
    holds), at another pitch, each output alone, and through the host call"""
    import torch
    t = table[p]
    A = t["A"]
    alone = [host(vdev.lpc_to_lsf(dev(A[r:r + 1]))) for r in range(len(A))]
    alone_back = [host(vdev.lsf_to_lpc(dev(t["back_in"][r:r + 1])))["a"][0] for r in range(len(t["back_in"]))]
    for n in (1, 7, 65):
        idx = batch_rows(t, n)
        got = host(vdev.lpc_to_lsf(dev(A[idx])))
        # another pitch: rows p + 4 floats apart in a poisoned buffer
        wide = np.full((n, p + 4), POISON, np.float32)
        wide[:, :p + 1] = A[idx]
        dw = dev(wide)
        pitched = host(vdev.lpc_to_lsf(dw[:, :p + 1]))
        assert np.array_equal(dw.cpu().numpy().view(np.uint32), wide.view(np.uint32))
        singles = {k: host(vdev.lpc_to_lsf(dev(A[idx]), what=k))[k] for k in lu_names()}
        for j, r in enumerate(idx):
            for k in lu_names():
                lu.assert_bits(got[k][j], alone[r][k][0], (k, n, j))
                lu.assert_bits(pitched[k][j], alone[r][k][0], (k, "pitch", n, j))
                lu.assert_bits(singles[k][j], alone[r][k][0], (k, "alone", n, j))
        # the way back, into rows p + 4 apart
        bidx = [i % len(t["back_in"]) for i in range(n)]
        outw = torch.full((n, p + 4), float(POISON), dtype=torch.float32, device="cuda")
        back = host(vdev.lsf_to_lpc(dev(t["back_in"][bidx]), out=outw))["a"]
        packed = host(vdev.lsf_to_lpc(dev(t["back_in"][bidx])))["a"]
        assert np.all(outw.cpu().numpy()[:, p + 1:] == POISON)
        for j, r in enumerate(bidx):
            lu.assert_bits(back[j], alone_back[r], ("a", "pitch", n, j))
            lu.assert_bits(packed[j], alone_back[r], ("a", n, j))
    # the host calls
    api = lu.LsfApi(amd_lib_path)
    for r in range(len(A)):
        st, lsf, rc, flags = api.lpc_to_lsf(A[r])
        assert st == 0
        lu.assert_bits(lsf, alone[r]["lsf"][0], ("host lsf", r))
        lu.assert_bits(rc, alone[r]["rc"][0], ("host rc", r))
        assert flags[0] == alone[r]["flags"][0]
        st, lsf, rc, flags = api.lpc_to_lsf(A[r], want=("rc",))
        assert st == 0 and np.all(lsf == lu.SENT) and flags[0] == -77
        lu.assert_bits(rc, alone[r]["rc"][0], ("host rc alone", r))
    for r in range(len(t["back_in"])):
        st, a = api.lsf_to_lpc(t["back_in"][r])
        assert st == 0
        lu.assert_bits(a, alone_back[r], ("host a", r))


def lu_names():
    return ("lsf", "rc", "flags")


@pytest.mark.parametrize("nch", (1, 3))
@pytest.mark.parametrize("center", (False, True))
@pytest.mark.parametrize("windowed", (False, True))
def test_frames_equal_the_two_calls(vdev, knob, nch, center, windowed):
    """lsf_frames == lpc_frames followed by lpc_to_lsf, bit for bit, with channel groups of 1 and
    of more than nch, and each output alone"""
    sig = lpc_util.load("lpc_signals")
    x = np.stack([sig["resonant"][:2000], sig["white"][100:2100], sig["resonant"][3000:5000]])[:nch]
    dx = dev(x)
    win = dev(hamming(400).astype(np.float32)) if windowed else None
    order = 16
    a, err = vdev.lpc_frames(dx, 400, 160, order, window=win, center=center)
    fr = a.shape[1]
    assert fr == (13 if center else 11)
    want = host(vdev.lpc_to_lsf(a.reshape(nch * fr, order + 1)))
    want = {k: v.reshape((nch, fr) + v.shape[1:]) for k, v in want.items()}
    want["err"] = err.cpu().numpy()
    for group in (1, 5):
        knob("LSF_GROUP", group)
        vdev.debug_clear("STAT_LSF")
        got = host(vdev.lsf_frames(dx, 400, 160, order, window=win, center=center))
        assert vdev.debug_get("STAT_LSF") == (nch if group == 1 else 1)
        for k in ("lsf", "rc", "flags", "err"):
            lu.assert_bits(got[k], want[k], (k, group))
        for k in ("lsf", "rc", "flags", "err"):
            lu.assert_bits(host(vdev.lsf_frames(dx, 400, 160, order, what=k, window=win, center=center))[k], want[k],
                           (k, "alone", group))
    assert np.all(want["flags"] == lu.STABLE | lu.COMPLETE)   # autocorrelation LPC is minimum phase


def test_zero_frames_write_nothing(vdev):
    import torch
    x = dev(np.zeros((2, 300), np.float32))
    bufs = [torch.full((64,), float(POISON), dtype=torch.float32, device="cuda") for _ in range(4)]
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = vdev.lib().vv_dsp_lsf_frames_device(vp(x), 300, 2, 300, 400, 160, 0, None, 16, vp(bufs[0]), vp(bufs[1]),
                                             vp(bufs[2]), vp(bufs[3]), None)
    torch.cuda.synchronize()
    assert st == 0
    for b in bufs:
        assert np.all(b.cpu().numpy() == POISON)
    out = vdev.lsf_frames(x, 400, 160, 16)
    assert out["lsf"].shape == (2, 0, 16) and out["flags"].shape == (2, 0)


def test_counter_counts_launches(vdev, table):
    t = table[8]
    vdev.debug_clear("STAT_LSF")
    for i in range(1, 4):
        vdev.lpc_to_lsf(dev(t["A"]), what="rc")
        assert vdev.debug_get("STAT_LSF") == 2 * i - 1
        vdev.lsf_to_lpc(dev(t["lsf"]))
        assert vdev.debug_get("STAT_LSF") == 2 * i
    # zero rows launch nothing
    assert vdev.lpc_to_lsf(dev(np.zeros((0, 9), np.float32)))["lsf"].shape == (0, 8)
    assert vdev.debug_get("STAT_LSF") == 6
