"""The mel / MFCC kernel (k_mel_grp, mel_kernels.hip) and its host schedule
(shim_mel.hip) against a float64 reference, at the plan shapes and edges where
they can go wrong: empty filters, odd and boundary M, C = 1 and C = M, every
frames-per-wave-step variant, pitched and misaligned rows, caller filterbanks
with gaps, single bins, no weights at all and mixed signs, and dynamic LDS
above 64 KB.  The reference and the derived bounds are in tests/mel_util.py;
every assertion message carries max(error / bound).

Measured max(error / bound) on an MI355X (first run of this module):
    A  probe, device plans P1-P11 0.609; caller banks 0.631
    B  log-mel 0.569; MFCC from the device's log-mel rows 0.324; MFCC from
       power 0.161.  Against the plain MFCC bound, without the lifter-factor
       term of mel_util.mfcc_bound, 1.070 (P5, eps 1e-10: C = 60, lifter 22)
    C  finite log-mel 0.381
    D  log-mel 0.552 (every pitched or offset call bit-identical to packed)
    E  MFCC 0.312; plain bound 0.977 (M = C = 65, lifter 22)
    F  log-mel 0.355
    G  the 82 KB bank and the 64 KB DCT table (94832 and 68096 bytes of
       dynamic LDS) launch as they are, status OK, values inside the bounds above

The tests without the gpu mark check the reference itself: the float64
formulas against the oracle (the C restatement of the reference's f32 code) at
the same bounds, and the host filterbank setup bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mel_util as mu
from vvapi import OK, ERR_SIZE, ERR_RANGE, VvDsp

gpu = pytest.mark.gpu
ALL = list(mu.PLANS)
ROWS = (1, 3, 4, 5, 9)


@functools.lru_cache(maxsize=None)
def _bank(orc, name):
    """The oracle's filterbank of plan `name`, read-only, after asserting on it
    what the plan is in the grid for."""
    nfft, M, sr, fmin, fmax, ncoef, lifter, _ = mu.PLANS[name]
    st, fb = orc.mel_filterbank(nfft, M, sr, fmin, fmax)
    assert st == OK and fb.shape == (M, nfft // 2 + 1)
    assert not (fb < 0).any()
    lo, ln = mu.fb_ranges(fb)
    empty = int(np.sum(ln == 0))
    used = np.flatnonzero(fb.any(axis=0))
    lc, nc = mu.chunk_count(fb)
    per_wave4 = 4 * ((4 * fb.shape[1] + 255) // 256 * 256 + ((4 * nc + 3) & ~3) + 4 * M)   # launch_mel_grp, MFCC
    per_wave2 = 4 * ((2 * fb.shape[1] + 255) // 256 * 256 + ((2 * nc + 3) & ~3) + 2 * M)
    fr = 4 if per_wave4 <= 16384 else 2 if per_wave2 <= 16384 else 1
    want = {
        "P1": M == 1 and 60 <= nc <= 68,
        "P3": M % 2 == 1 and ncoef == M,
        "P4": M % 2 == 1,
        "P5": empty >= 1 and 2 * M == 120 and ncoef == M,
        "P6": M % 2 == 1 and 2 * ncoef > 64,
        "P7": empty >= 1 and 64 < M <= 128 and nc <= 256,
        "P8": M == 128 and nc > 256,
        "P9": M > 128 and empty >= 2,
        "P10": ln.min() >= 1 and ln.max() <= 6,
        "P11": used[0] > 200 and used[-1] == fb.shape[1] - 1,
        "P12": fb.shape[1] == 9 and empty >= 1,
        "P13": fb.shape[1] == 3,
        "P14": fr == 2 and (2 * fb.shape[1]) % 4 != 0,
        "P15": fr == 1,
        "P16": fr == 1 and fb.shape[1] == 4097,
    }.get(name, True)
    assert want, (name, mu.PLANS[name][-1], dict(empty=empty, nc=nc, lc=lc, fr=fr, first=int(used[0]),
                                                 last=int(used[-1]), minlen=int(ln.min()), maxlen=int(ln.max())))
    fb.setflags(write=False)
    return fb


# ---------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("name", ALL)
def test_reference_within_bounds_of_oracle(orc, name):
    """The float64 reference against the oracle's f32 restatement of mel.c:
    log-mel at the kernel's bound (one running sum is K_m = 1), MFCC at the
    kernel's bound plus the oracle's own error (mel_util.oracle_mfcc_bound)."""
    nfft, M, sr, fmin, fmax, ncoef, lifter, _ = mu.PLANS[name]
    fb = _bank(orc, name)
    for eps in (1e-10, 1.0):
        p = mu.plan_power(fb.shape[1], 9, M)
        ref = mu.log_mel64(p, fb, eps)
        bound, _ = mu.log_mel_bound(p, fb, eps, ref)
        lm = orc.log_mel(p, fb, eps)
        r = mu.ratio(lm, ref, bound)
        assert r <= 1.0, ("log-mel", name, eps, r)
        mf = orc.mfcc(lm, ncoef, lifter)
        r = mu.ratio(mf, mu.mfcc64(lm, ncoef, lifter), mu.oracle_mfcc_bound(lm, ncoef, lifter))
        assert r <= 1.0, ("mfcc", name, eps, r)


def test_lifter_factor_gap():
    """The f32 lifter factor (mel.c:300-302, what the kernels multiply by) against
    the float64 formula: inside mel_util.lifter_gap, and for lifter 22 far
    outside a few ulp of the factor -- why mfcc_bound has its second term."""
    f = np.float32
    worst = 0.0
    for lifter, ncoef in ((22.0, 60), (22.0, 128), (0.5, 33), (1.0, 13)):
        i = np.arange(ncoef).astype(f)
        lf = f(1) + (f(lifter) / f(2)) * np.sin(f(np.pi) * i / f(lifter)).astype(f)
        lf[0] = 1
        err = np.abs(lf.astype(np.float64) - mu.lifter64(ncoef, lifter))
        assert np.all(err <= mu.lifter_gap(ncoef, lifter) + mu.U * np.abs(lf)), (lifter, ncoef)
        worst = max(worst, float(np.max(err / np.abs(lf))) / mu.U)
    assert worst > 16, worst


@pytest.fixture(scope="module")
def host_lib(amd_lib_path):
    """The product library's host entry points; they need no device."""
    return VvDsp(amd_lib_path)


@pytest.mark.parametrize("name", ALL)
def test_host_filterbank_equals_oracle(host_lib, orc, name):
    nfft, M, sr, fmin, fmax = mu.PLANS[name][:5]
    st, fb = host_lib.mel_filterbank(nfft, M, sr, fmin, fmax)
    assert st == OK and fb.dtype == np.float32
    assert np.array_equal(fb, _bank(orc, name)), name


def test_host_filterbank_status_codes(host_lib, orc):
    """n_mels >= nbins is a size error, fmax > sr / 2 a range error (mel.c:78-98)"""
    for args, code in (((1024, 513, 48000.0, 0.0, 24000.0), ERR_SIZE), ((16, 9, 8000.0, 0.0, 4000.0), ERR_SIZE),
                       ((4, 3, 8000.0, 0.0, 4000.0), ERR_SIZE), ((1024, 40, 48000.0, 0.0, 24000.5), ERR_RANGE),
                       ((1024, 600, 48000.0, 0.0, 30000.0), ERR_RANGE)):
        assert host_lib.mel_filterbank(*args)[0] == code == orc.mel_filterbank(*args)[0], args


def test_host_filterbank_equals_reference(host_lib, ref):
    for name in ALL:
        nfft, M, sr, fmin, fmax = mu.PLANS[name][:5]
        st, fb = host_lib.mel_filterbank(nfft, M, sr, fmin, fmax)
        st_r, fb_r = ref.mel_filterbank(nfft, M, sr, fmin, fmax)
        assert st == st_r == OK and np.array_equal(fb, fb_r), name
    for args in ((1024, 513, 48000.0, 0.0, 24000.0), (1024, 40, 48000.0, 0.0, 24000.5)):
        assert host_lib.mel_filterbank(*args)[0] == ref.mel_filterbank(*args)[0] != OK, args


# ---------------------------------------------------------------- device helpers
GUARD = 64


def _plan(vdev, name, eps):
    nfft, M, sr, fmin, fmax, ncoef, lifter, _ = mu.PLANS[name]
    return vdev.Mfcc(nfft, M, ncoef, sr, fmin, fmax, lifter=lifter, eps=eps)


def _run_rows(vdev, mf, power, kind, pitch=0, in_off=0):
    """Power rows (NumPy [rows][nbins]) through the plan's kernel by the C entry
    points, the input at `pitch` floats per row (0: packed; the pad is NaN, it
    must never reach a sum) and `in_off` floats into its buffer, the output
    between guard floats that must stay untouched.  kind 0: log-mel, 1: MFCC."""
    import torch
    rows, nb = power.shape
    width = mf.n_mels if kind == 0 else mf.n_coeffs
    step = pitch if pitch else nb
    src = torch.full((in_off + rows * step,), float("nan"), device="cuda")
    src[in_off:].view(rows, step)[:, :nb] = torch.from_numpy(power).cuda()
    buf = torch.full((GUARD + rows * width + GUARD,), -7.0, device="cuda")
    L = vdev.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pin = C.c_void_p(src.data_ptr() + 4 * in_off)
    pout = C.c_void_p(buf.data_ptr() + 4 * GUARD)
    if pitch:
        f = L.vv_dsp_log_mel_pitched_device if kind == 0 else L.vv_dsp_mfcc_process_pitched_device
        st = f(mf.h, pin, rows, pitch, pout, s)
    else:
        f = L.vv_dsp_log_mel_device if kind == 0 else L.vv_dsp_mfcc_process_device
        st = f(mf.h, pin, rows, pout, s)
    assert st == OK, (st, L.vvhip_last_error())
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:GUARD] == -7.0) and np.all(b[GUARD + rows * width:] == -7.0), "stores outside the rows"
    return b[GUARD:GUARD + rows * width].reshape(rows, width).copy()


def _check_log_mel(got, power, fb, eps, what):
    ref = mu.log_mel64(power, fb, eps)
    bound, amp = mu.log_mel_bound(power, fb, eps, ref)
    assert np.all(np.isfinite(got)), what
    r = mu.ratio(got, ref, bound)
    assert r <= 1.0, (what, "log-mel error / bound", r)
    return r


def _check_mfcc(got, lm, ncoef, lifter, what):
    """MFCC rows against the f64 DCT of the log-mel rows they were computed from"""
    ref = mu.mfcc64(lm, ncoef, lifter)
    r = mu.ratio(got, ref, mu.mfcc_bound(lm, ncoef, lifter))
    plain = mu.ratio(got, ref, mu.mfcc_bound(lm, ncoef, lifter, plain=True))
    assert r <= 1.0, (what, "mfcc error / bound", r, "without the lifter term", plain)
    return r, plain


def _check_probe(out, fb, eps, what):
    """out: log-mel rows of mel_util.probe_power.  A filter that does not weigh
    bin k answers row k exactly as it answers the all-zero row; one that does
    is within the log-mel bound of a one-bin sum."""
    nb = fb.shape[1]
    p = mu.probe_power(nb)
    zero_row = out[nb]
    same = out[:nb] == zero_row[None, :]
    off = (fb.T == 0)
    assert np.all(same[off]), (what, "a filter reads a bin it has no weight on", np.argwhere(off & ~same)[:4])
    ref = mu.log_mel64(p, fb, eps)
    bound, _ = mu.log_mel_bound(p, fb, eps, ref, unit=True)
    on = ~off
    err = np.abs(out[:nb].astype(np.float64) - ref[:nb])
    r = float(np.max(err[on] / bound[:nb][on])) if on.any() else 0.0
    assert r <= 1.0, (what, "probe error / bound", r, np.argwhere(on & (err > bound[:nb]))[:4])
    r0 = mu.ratio(zero_row[None, :], ref[nb:], bound[nb:])
    assert r0 <= 1.0, (what, "all-zero row", r0)
    return max(r, r0)


# ---------------------------------------------------------------- A: weight placement
@gpu
@pytest.mark.parametrize("name", mu.NFFT1024)
def test_probe_device_plan(vdev, orc, name):
    import torch
    fb = _bank(orc, name)
    eps = 2.0 ** -20
    mf = _plan(vdev, name, eps)
    out = mf.log_mel(torch.from_numpy(mu.probe_power(fb.shape[1])).cuda()).cpu().numpy()
    print("A %s: probe %.3f" % (name, _check_probe(out, fb, eps, name)))


@gpu
@pytest.mark.parametrize("nbins", [513, 257])
@pytest.mark.parametrize("bank", ["gaps", "ends", "zero", "mixed", "dense"])
def test_probe_caller_bank(amd, nbins, bank):
    fb = mu.caller_banks(nbins)[bank]
    # a one-bin row under a negative weight has a negative sum (>= -2^9): there
    # eps = 2^10 keeps the log's argument positive; 2^-20 everywhere else
    eps = 2.0 ** 10 if bank == "mixed" else 2.0 ** -20
    assert bank != "mixed" or fb.min() >= -0.5
    out = amd.log_mel(mu.probe_power(nbins), fb, eps)
    print("A %s nbins %d: probe %.3f" % (bank, nbins, _check_probe(out, fb, eps, (bank, nbins))))


# ---------------------------------------------------------------- B: plan grid
@gpu
@pytest.mark.parametrize("eps", [1e-10, 1.0])
@pytest.mark.parametrize("name", ALL)
def test_plan_grid(vdev, orc, name, eps):
    ncoef, lifter = mu.PLANS[name][5:7]
    fb = _bank(orc, name)
    mf = _plan(vdev, name, eps)
    worst = [0.0, 0.0, 0.0, 0.0]
    for rows in ROWS:
        p = mu.plan_power(fb.shape[1], rows, rows)
        assert not p[-1].any()
        lm = _run_rows(vdev, mf, p, 0)
        r_lm = _check_log_mel(lm, p, fb, eps, (name, eps, rows))
        mfc = _run_rows(vdev, mf, p, 1)
        # the DCT and lifter alone: from the device's own log-mel rows
        r_mf, plain = _check_mfcc(mfc, lm, ncoef, lifter, (name, eps, rows))
        # end to end from power
        ref = mu.log_mel64(p, fb, eps)
        lmb, _ = mu.log_mel_bound(p, fb, eps, ref)
        r_e2e = mu.ratio(mfc, mu.mfcc64(ref, ncoef, lifter), mu.mfcc_bound_from_power(ref, lmb, ncoef, lifter))
        assert r_e2e <= 1.0, (name, eps, rows, "mfcc from power error / bound", r_e2e)
        worst = [max(a, b) for a, b in zip(worst, (r_lm, r_mf, plain, r_e2e))]
    print("B %s eps %g: log-mel %.3f mfcc %.3f (plain bound %.3f) from power %.3f" % (name, eps, *worst))


# ---------------------------------------------------------------- C: empty filters, eps = 0
@gpu
@pytest.mark.parametrize("name", ["P5", "P7"])
def test_empty_filters_eps_zero(vdev, orc, name):
    ncoef, lifter = mu.PLANS[name][5:7]
    fb = _bank(orc, name)
    _, ln = mu.fb_ranges(fb)
    assert (ln == 0).any()
    mf = _plan(vdev, name, 0.0)
    rng = np.random.default_rng(5)
    p = (rng.random((5, fb.shape[1])) * 10 + 0.5).astype(np.float32)
    lm_o = orc.log_mel(p, fb, 0.0)
    assert np.array_equal(np.isneginf(lm_o), np.broadcast_to(ln == 0, lm_o.shape))
    lm = _run_rows(vdev, mf, p, 0)
    assert np.array_equal(np.isneginf(lm), np.isneginf(lm_o))
    assert np.array_equal(np.isfinite(lm), np.isfinite(lm_o))
    ref = mu.log_mel64(p, fb, 0.0)
    bound, _ = mu.log_mel_bound(p, fb, 0.0, ref)
    r = mu.ratio(lm, ref, bound)
    assert r <= 1.0, (name, "finite log-mel error / bound", r)
    mfc = _run_rows(vdev, mf, p, 1)
    mf_o = orc.mfcc(lm_o, ncoef, lifter)
    assert not np.isfinite(mf_o).all()
    assert np.array_equal(np.isfinite(mfc), np.isfinite(mf_o))
    print("C %s: log-mel %.3f" % (name, r))


# ---------------------------------------------------------------- D: row geometry
@gpu
@pytest.mark.parametrize("name,pitch,in_off,rows", [
    ("P14", 1026, 0, 5), ("P14", 1028, 0, 5),   # fr = 2, LDS-DMA on, a last group of one row
    ("P14", 1026, 0, 4), ("P14", 1028, 0, 4),   # a full last group whose valid & 3 != 0
    ("P15", 2052, 0, 3),                        # fr = 1
    ("P2", 0, 1, 9),                            # fr = 4, base 4 B past a 16 B boundary: no LDS-DMA
])
def test_row_geometry(vdev, orc, name, pitch, in_off, rows):
    ncoef, lifter = mu.PLANS[name][5:7]
    fb = _bank(orc, name)
    eps = 1e-10
    mf = _plan(vdev, name, eps)
    p = mu.plan_power(fb.shape[1], rows, 100 + rows)
    packed = _run_rows(vdev, mf, p, 0)
    r = _check_log_mel(packed, p, fb, eps, (name, "packed"))
    assert np.array_equal(_run_rows(vdev, mf, p, 0, pitch, in_off), packed)
    packed_c = _run_rows(vdev, mf, p, 1)
    _check_mfcc(packed_c, packed, ncoef, lifter, (name, "packed"))
    assert np.array_equal(_run_rows(vdev, mf, p, 1, pitch, in_off), packed_c)
    print("D %s pitch %d off %d: log-mel %.3f" % (name, pitch, in_off, r))


# ---------------------------------------------------------------- E: vv_dsp_mfcc from log-mel rows
@gpu
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("lifter", [0.0, 22.0])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 26, 64, 65, 128])
def test_mfcc_from_log_mel(amd, M, lifter, rows):
    """C = 1 and C = M; M = C = 128 is a 64 KB table (dynamic LDS above 64 KB)"""
    rng = np.random.default_rng(M + rows)
    lm = rng.uniform(-20.0, 5.0, (rows, M)).astype(np.float32)
    for ncoef in sorted({1, M}):
        got = amd.mfcc(lm, ncoef, lifter)
        assert got.shape == (rows, ncoef)
        r, plain = _check_mfcc(got, lm, ncoef, lifter, (M, ncoef, lifter, rows))
        print("E M %d C %d lifter %g rows %d: mfcc %.3f (plain bound %.3f)" % (M, ncoef, lifter, rows, r, plain))


# ---------------------------------------------------------------- F: caller filterbanks
@gpu
@pytest.mark.parametrize("nbins", [513, 257])
@pytest.mark.parametrize("bank", ["gaps", "ends", "zero", "mixed", "dense"])
def test_caller_bank(amd, nbins, bank):
    """dense at 513 bins: 82 KB of weights (dynamic LDS above 64 KB)"""
    fb = mu.caller_banks(nbins)[bank]
    rng = np.random.default_rng(nbins + len(bank))
    eps = 1e-3
    if bank == "mixed":
        assert (fb < 0).any() and (fb > 0).any()
        p = (1.0 + rng.random((5, nbins))).astype(np.float32)
        ref = mu.log_mel64(p, fb, eps)
        _, amp = mu.log_mel_bound(p, fb, eps, ref)
        assert np.all(np.isfinite(ref)) and amp.max() <= 10.0, amp.max()   # e + eps >= 0.1 sum|w p|
    else:
        p = mu.plan_power(nbins, 5, nbins)
    got = amd.log_mel(p, fb, eps)
    r = _check_log_mel(got, p, fb, eps, (bank, nbins))
    if bank == "zero":
        assert np.all(got == got[0, 0])   # logf(eps), and _check_log_mel held it to 2 u + 4 u |log eps|
    print("F %s nbins %d: log-mel %.3f" % (bank, nbins, r))


# ---------------------------------------------------------------- G: the table that cannot fit
@gpu
def test_mfcc_table_too_large(amd):
    """M = C = 256 is a 256 KB DCT table, more LDS than a CU has: a status, the
    output untouched, and the next ordinary call unharmed."""
    L = amd._mel_setup()
    lm = np.random.default_rng(0).uniform(-20.0, 5.0, (3, 256)).astype(np.float32)
    out = np.full((3, 256), -7.0, np.float32)
    st = L.vv_dsp_mfcc(lm.ctypes.data_as(C.POINTER(C.c_float)), 3, 256, 256, 2, 0.0,
                       out.ctypes.data_as(C.POINTER(C.c_float)))
    assert st != OK
    assert np.all(out == -7.0)
    small = lm[:, :26].copy()
    _check_mfcc(amd.mfcc(small, 13, 22.0), small, 13, 22.0, "after the refused call")
