"""Batched DCT and Hilbert rows (vv_dsp_dct_execute_device,
vv_dsp_hilbert_analytic_device) against plain f64 (scipy.fft.dct,
scipy.signal.hilbert, the DCT formulas of test_dct_types_vs_formula) on every
route of dct_run / vvhip_hilbert_device and on every trip of the persistent
pair kernels, with the error measured per row pair (analytic_util.py) at the
project's bound 2e-6 * max(1, log2 n), and NaN guard rows behind every output.

Routes (shim_analytic.hip, dct2_fused.hpp, hilbert_fused.hpp):
  DCT   II forward: k_dct2_small 16..128 (16 B aligned rows), k_dct2_pair pow2
        2..8192 (256, 4096, 8192 read their mirror bins through LDS), above and
        for even 7-smooth n k_dct2_pre + R2C + k_dct2_post;
        II / III backward: k_dct3_pre + C2R + k_dct3_post (pow2 4..16384, even
        7-smooth n); everything else (III forward, IV, odd or non-smooth n,
        n < 4 backward) k_dct_naive.
  Hilbert  k_hilbert_small 16..128, k_hilbert_pair pow2 2..8192, otherwise
        R2C + k_hilbert_mask + C2C in place on the output.

The pair clause these tests pin: in the fused kernels rows
2j and 2j + 1 share one complex FFT, so a row's error is bounded relative to
the larger row of its pair, and a non-finite value makes its own row
non-finite and may make its partner non-finite, and no other row.

Worst err / bound per n, measured on an MI355X (every test of this module, all
batches, types, routes and knobs; the bound is 2e-6 * max(1, log2 n); `-s`
prints the figure of every check):

      n     DCT    Hilbert  |      n     DCT    Hilbert
      1    0.029    0.000   |    400    0.014    0.015
      2    0.049    0.040   |    441      -      0.013
      3      -      0.036   |   1000    0.015    0.014
      4    0.056      -     |   1024    0.013    0.016
      7    0.011    0.026   |   1025      -      0.028
     16    0.025      -     |   2048    0.009    0.017
     64    0.019    0.026   |   4096    0.010    0.018
    202    0.004      -     |   8192    0.008    0.015
    255      -      0.007   |  16384    0.008    0.008
    256    0.015    0.021   |  32768      -      0.011
    257    0.004    0.003   |

so the kernels sit 18 to 300 times below the bound: the f32 two-for-one
emulation on the CPU (analytic_util.py) sits 80 to 100 times below it.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import vvdsp_amd as vv

import analytic_util as au

pytestmark = pytest.mark.gpu


def _rows(full, batch):
    return full[:batch].cpu().numpy()


# ---------------------------------------------------------------- B: batched DCT, every type, direction, route
DCT_N = [1, 2, 4, 7, 16, 64, 202, 256, 257, 400, 1000, 1024, 4096, 16384]   # 202 = 2 * 101: even, not smooth


def _dct_cases():
    for t, inv in ((2, False), (2, True), (3, False), (3, True), (4, False), (4, True)):
        for n in DCT_N:
            # III forward and IV are k_dct_naive at every n, O(n^2) per row: n <= 4096 in a
            # batch (n = 16384 at batch 1 is test_dct_types_vs_formula's)
            if ((t == 3 and not inv) or t == 4) and n > 4096:
                continue
            yield pytest.param(t, inv, n, id=f"type{t}-{'bwd' if inv else 'fwd'}-{n}")


@pytest.mark.parametrize("dct_type,inverse,n", _dct_cases())
def test_dct_batched_types_routes(dct_type, inverse, n):
    """Every (type, direction) over a batch: rows other than row 0 (f * n,
    f * nh in the pre / post / naive kernels), odd batches (the pair without a
    partner), 65 and 1029 rows (more than one wave block and workgroup)."""
    for batch in ((1, 2, 3, 65, 1029) if n <= 1024 else (3, 37)):
        x = au.rows_input(batch, n, 7000 * dct_type + 100 * n + 10 * inverse + batch)
        ref = au.dct_ref(x.cpu().numpy().astype(np.float64), dct_type, inverse)
        knob_sets = [{}]
        if dct_type == 2 and not inverse and 16 <= n <= 128:
            knob_sets.append({"DCT_SMALL": 0})   # the pair kernel at the staged sizes
        for kn in knob_sets:
            with vv.knobs(**kn):
                st, full = au.run_dct(vv, x, dct_type, inverse)
            assert st == au.ST_OK, (batch, kn, st)
            assert au.guards_intact(full, batch), (batch, kn, "rows behind the batch were written")
            au.assert_pairs(_rows(full, batch), ref, n,
                            what=f"dct type {dct_type} inverse {inverse} batch {batch} {kn}")


# ---------------------------------------------------------------- C: batched Hilbert off the fused sizes
@pytest.mark.parametrize("n,batches", [(n, (1, 2, 5, 64)) for n in (1, 3, 7, 255, 400, 441, 1000, 1025)]
                         + [(16384, (3,)), (32768, (3,))])
def test_hilbert_batched_chain(n, batches):
    """R2C + k_hilbert_mask + inverse C2C in place over a batch: odd, mixed-radix,
    Bluestein and four-step lengths (half_dist and the odd-n branch of the mask
    at rows other than row 0).  The chain has no pairs; the pair is the grouping."""
    for batch in batches:
        x = au.rows_input(batch, n, 31 * n + batch)
        ref = au.hilbert_ref(x.cpu().numpy().astype(np.float64))
        st, full = au.run_hilbert(vv, x)
        assert st == au.ST_OK, (batch, st)
        assert au.guards_intact(full, batch), (batch, "rows behind the batch were written")
        au.assert_pairs(au.as_complex(_rows(full, batch)), ref, n, what=f"hilbert chain batch {batch}")


# ---------------------------------------------------------------- D: past one resident sweep
# Geo<N>::T, threads per transform (fft_core.hpp: P = min(N, 16) points per thread, T = N / P)
GEO_T = {2: 1, 64: 4, 256: 16, 1024: 64, 2048: 128, 4096: 256, 8192: 512}


def sweep_rows(n, cus):
    """A CU holds at most 32 waves = 2048 threads, so a resident grid holds at
    most cus * 2048 / T pairs: more than two such sweeps, and odd.
    -> (rows, pairs per sweep)"""
    sweep = cus * 2048 // GEO_T[n]
    return 2 * (2 * sweep) + 3, sweep


@pytest.mark.parametrize("n", [2, 64, 256, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("kind", ["hilbert", "dct"])
def test_pair_kernels_past_one_sweep(kind, n):
    """k_hilbert_pair<N> / k_dct2_pair<N, 0> on a batch no resident grid can hold
    in two trips (so the loop wraps at least twice: the per-trip index math and
    the xsync before the next pair's loads), against the non-persistent grid
    (knob ANA_TPW = 1, one pair per slot) bit for bit over all rows, and 32
    sampled pairs against f64: the first, the last (unpaired) row, the pairs on
    either side of each sweep seam, the rest random.  N = 64 under *_SMALL = 0
    (by default the staged kernel, which is not persistent, takes it).  The
    grids seen under a kernel trace (3 to 9 trips per slot) are in DESIGN.md
    section 4."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, sweep = sweep_rows(n, cus)
    x = au.rows_input(rows, n, 900 + n)
    base = {("HIL_SMALL" if kind == "hilbert" else "DCT_SMALL"): 0} if n == 64 else {}
    run = (lambda: au.run_hilbert(vv, x)) if kind == "hilbert" else (lambda: au.run_dct(vv, x))
    with vv.knobs(**base):
        st, got = run()
    assert st == au.ST_OK
    with vv.knobs(ANA_TPW=1, **base):
        st, one = run()
    assert st == au.ST_OK
    assert au.guards_intact(got, rows) and au.guards_intact(one, rows), "rows behind the batch were written"
    assert torch.equal(got[:rows].view(torch.int32), one[:rows].view(torch.int32)), "persistent != one pair per slot"
    del one
    pairs = {0, (rows - 1) // 2}
    for k in (1, 2):
        seam = k * sweep * 2          # first row of sweep k
        assert 0 < seam < rows
        pairs |= {seam // 2 - 1, seam // 2}
    rng = np.random.default_rng(n)
    while len(pairs) < 32:
        pairs.add(int(rng.integers(0, (rows + 1) // 2)))
    pick = np.array(sorted(r for p in pairs for r in (2 * p, 2 * p + 1) if r < rows))
    idx = torch.from_numpy(pick).cuda()
    y = got.index_select(0, idx).cpu().numpy()
    x64 = x.index_select(0, idx).cpu().numpy().astype(np.float64)
    if kind == "hilbert":
        au.assert_pairs(au.as_complex(y), au.hilbert_ref(x64), n, rows=pick, what=f"hilbert sweep rows {rows}")
    else:
        au.assert_pairs(y, au.dct_ref(x64, 2, False), n, rows=pick, what=f"dct sweep rows {rows}")


# ---------------------------------------------------------------- E: rows of different scale
SCALES = (1.0, 1e-4, 1e4, 1.0, 1e-4, 1e-4)   # pairs (1, 1e-4), (1e4, 1), (1e-4, 1e-4)


@pytest.mark.parametrize("n", [64, 1024, 4096])
@pytest.mark.parametrize("kind", ["hilbert", "dct"])
def test_pair_scales(kind, n):
    """Rows of different scale in one pair: each pair meets the bound relative to
    its larger row; the (1e-4, 1e-4) pairs relative to their own scale (an
    absolute tolerance hiding in a kernel would fail them)."""
    batch = 66
    x = au.rows_input(batch, n, 4000 + n, scale=SCALES)
    x64 = x.cpu().numpy().astype(np.float64)
    amax = np.abs(x64).max(axis=1)
    assert amax[0] > 1e3 * amax[1] and amax[2] > 1e3 * amax[3] and amax[4] < 1e-2 and amax[5] < 1e-2
    if kind == "hilbert":
        st, full = au.run_hilbert(vv, x)
        y, ref = au.as_complex(_rows(full, batch)), au.hilbert_ref(x64)
    else:
        st, full = au.run_dct(vv, x)
        y, ref = _rows(full, batch), au.dct_ref(x64, 2, False)
    assert st == au.ST_OK and au.guards_intact(full, batch)
    au.assert_pairs(y, ref, n, what=f"{kind} scales")
    small = np.array([r for r in range(batch) if r % 6 >= 4])
    au.assert_pairs(y[small], ref[small], n, rows=small, what=f"{kind} scales small-pairs")


# ---------------------------------------------------------------- E: non-finite rows, the NaN policies over a batch
BAD_N = [64, 1024, 257]   # staged, pair, naive (DCT) / staged, pair, chain (Hilbert)


def _bad_rows(n, seed):
    """9 rows: a NaN in row 4, +Inf in row 7, -Inf in the last row 8.
    Pairs (0,1) (2,3) (4,5) (6,7) (8)."""
    x = au.rows_input(9, n, seed)
    x[4, 3] = float("nan")
    x[7, n // 2 - 12] = float("inf")
    x[8, n - 1] = float("-inf")
    return x


def _set_policy(p):
    L = vv.lib()
    L.vv_dsp_set_nan_policy.argtypes = [C.c_int]
    L.vv_dsp_set_nan_policy.restype = None
    L.vv_dsp_set_nan_policy(p)


@pytest.mark.parametrize("n", BAD_N)
@pytest.mark.parametrize("policy", [1, 3])
def test_dct_batched_policy_ignore_clamp(policy, n):
    """IGNORE (1) and CLAMP (3) over a batch (k_dct2_small<N, POL>,
    k_dct2_pair<N, POL>, k_nan_policy + k_dct_naive): the output is the f64 DCT
    of the input with the policy applied on read.  Under IGNORE that holds for
    all nine rows, pair by pair.  Under CLAMP rows 0...5 pair by pair (a NaN
    reads as 0); row 6, whose partner reads as FLT_MAX, relative to the larger
    row of its pair (the pair clause) and, on the naive route, which has no
    pairs, relative to itself; rows 7 and 8 (the transform of +-FLT_MAX
    overflows in f32 where the f64 sum does not, as
    test_dct_nan_policy_matches_reference notes) only hold no NaN."""
    x = _bad_rows(n, 5000 + n)
    ref = au.dct_ref(au.policy_on_read(x.cpu().numpy().astype(np.float64), policy), 2, False)
    _set_policy(policy)
    try:
        st, full = au.run_dct(vv, x)
    finally:
        _set_policy(0)
    assert st == au.ST_OK and au.guards_intact(full, 9)
    y = _rows(full, 9)
    what = f"dct policy {policy}"
    if policy == 1:
        au.assert_pairs(y, ref, n, what=what)
        return
    au.assert_pairs(y[:6], ref[:6], n, what=what)
    au.assert_pairs(y[6:8], ref[6:8], n, rows=np.array([6, 7]), only={6}, what=what + " row 6 in its pair")
    if n == 257:
        au.assert_pairs(y[6:7], ref[6:7], n, rows=np.array([6]), what=what + " row 6 alone")
    assert not np.isnan(y[7:]).any()


@pytest.mark.parametrize("n", BAD_N)
def test_dct_batched_policy_error(n):
    """ERROR (2) over a batch: a non-finite input in any row gives status NAN
    with nothing written; finite rows run the multi-pass route at status OK."""
    x = _bad_rows(n, 5100 + n)
    clean = au.rows_input(9, n, 5200 + n)
    _set_policy(2)
    try:
        st, full = au.run_dct(vv, x, fill=-7.0)
        st_ok, got = au.run_dct(vv, clean)
    finally:
        _set_policy(0)
    assert st == au.ST_NAN, st
    assert bool((full == -7.0).all()), "the output was written"
    assert st_ok == au.ST_OK and au.guards_intact(got, 9)
    au.assert_pairs(_rows(got, 9), au.dct_ref(clean.cpu().numpy().astype(np.float64), 2, False), n,
                    what="dct policy 2 finite")


def _check_propagated(y, ref, n, paired, what):
    assert not np.isfinite(y[[4, 7, 8]]).any(), "a bad row has a finite element"
    au.assert_pairs(y[:4], ref[:4], n, what=what)
    if not paired:
        for r in (5, 6):
            au.assert_pairs(y[r:r + 1], ref[r:r + 1], n, rows=np.array([r]), what=what + f" row {r} alone")
    # fused routes: rows 5 and 6 share their FFT with rows 4 and 7, so they may come out non-finite: not asserted


@pytest.mark.parametrize("n", BAD_N)
def test_dct_batched_propagate(n):
    """PROPAGATE (0): the bad rows are non-finite in every element, the rows of
    other pairs meet the bound, and on the naive route (no pairs) so do the bad
    rows' neighbours 5 and 6."""
    x = _bad_rows(n, 5300 + n)
    x64 = x.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        ref = au.dct_ref(x64, 2, False)
    st, full = au.run_dct(vv, x)
    assert st == au.ST_OK and au.guards_intact(full, 9)
    _check_propagated(_rows(full, 9), ref, n, paired=n != 257, what="dct propagate")


@pytest.mark.parametrize("n", BAD_N)
def test_hilbert_batched_nonfinite(n):
    """Hilbert has no policy: its rows behave as the DCT's under PROPAGATE
    (257: the chain, which has no pairs)."""
    x = _bad_rows(n, 5400 + n)
    x64 = x.cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        ref = au.hilbert_ref(x64)
    st, full = au.run_hilbert(vv, x)
    assert st == au.ST_OK and au.guards_intact(full, 9)
    _check_propagated(au.as_complex(_rows(full, 9)), ref, n, paired=n != 257, what="hilbert non-finite")


# ---------------------------------------------------------------- F: the row limit of the instantaneous phase
def test_inst_phase_row_limit(amd):
    """vvhip_inst_phase_device takes at most 65535 rows: 65535 rows of n = 2
    succeed and equal the host entry; 65536 return OUT_OF_RANGE and write nothing."""
    L = vv.lib()
    n = 2
    g = torch.Generator(device="cuda").manual_seed(65535)
    z = torch.complex(torch.randn(65536, n, device="cuda", generator=g),
                      torch.randn(65536, n, device="cuda", generator=g))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.full((65536 + au.GUARD, n), -7.0, device="cuda")
    zp, op = C.c_void_p(z.data_ptr()), C.c_void_p(out.data_ptr())
    assert L.vv_dsp_instantaneous_phase_device(zp, n, 65535, op, s) == au.ST_OK
    torch.cuda.synchronize()
    assert bool((out[65535:] == -7.0).all()), "rows behind the batch were written"
    p, zh = out.cpu().numpy(), z.cpu().numpy()
    for r in (0, 1, 255, 256, 32767, 65534):
        assert np.array_equal(p[r], amd.inst_phase(zh[r])), r
    out.fill_(-7.0)
    assert L.vv_dsp_instantaneous_phase_device(zp, n, 65536, op, s) == au.ST_RANGE
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote rows"
