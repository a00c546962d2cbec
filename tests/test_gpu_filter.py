"""GPU tests of the filter module: biquad cascades (iir_kernels.hip) and
Savitzky-Golay (savgol_kernels.hip) against the outputs recorded from the
reference (tests/golden/iir_*.npz, savgol_*.npz; layout in tests/filter_util.py).

Exact route (rows of n <= 8192, or knob IIR_CHUNK = 0): outputs and final states
bit-identical to the reference.  Batched rows are compared against the float32
model of filter_util, which tests/test_filter_host.py pins to the recorded
reference outputs bit for bit.

Chunked route (knob IIR_CHUNK = k, or n > 8192): the error against the f64 model
on the scale max|y_f64| is at most 2 x the reference's own (err_ref in the
fixture).  Basis: a CPU model of this scheme -- float walks, f64 transition
matrix and scan, L = 64 and 256, these four cascades -- measured 0.5 to 1.25 x
err_ref; 2 x leaves room for another L and scan grouping and nothing more.
After a NaN input the reference keeps finite states in the stages ahead of the
poisoned one and the chunked scan does not (every state is NaN from the next
chunk boundary on); the outputs are NaN either way and only they are compared.

Savitzky-Golay: bit-identical to the reference for every case, mode and length.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from filter_util import (FilterApi, load, cascade_model, savgol_model, savgol_lengths, mix_run, IIR_N, IIR_NAN_AT,
                         IIR_CUTS, IIR_CASCADES, SAVGOL_CASES, SAVGOL_MODES, SAVGOL_POLICY_CASE, OK, ERR_NAN)

pytestmark = pytest.mark.gpu

CAP, TILE = 8, 32     # IIR_MAX_STAGES, IIR_TILE of vvhip_internal.hpp
BOUND = 2.0           # x err_ref, see above


@pytest.fixture(scope="module")
def sig():
    return load("iir_signal")["x"]


@pytest.fixture(scope="module")
def ref():
    return load("iir_ref")


@pytest.fixture(scope="module")
def f64():
    return load("iir_f64")


@pytest.fixture(scope="module")
def api(amd_lib_path, vdev):
    return FilterApi(amd_lib_path)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_iir(vv, sos, rows, state=None, pad=0, inplace=False):
    """rows (b, n) numpy -> (y, final state) numpy; pad > 0: rows pad floats
    further apart than n on both sides (non-contiguous strides)"""
    rows = np.atleast_2d(rows)
    b, n = rows.shape
    S = len(sos)
    xb = torch.full((b, n + pad), -7.0, dtype=torch.float32, device="cuda")
    xb[:, :n] = dev(rows)
    x = xb[:, :n]
    st = dev(np.zeros((b, S, 2), np.float32) if state is None else np.asarray(state, np.float32).reshape(b, S, 2))
    if inplace:
        y = vv.iir(x, dev(sos), state=st, out=x)
    else:
        yb = torch.full((b, n + 2 * pad), -9.0, dtype=torch.float32, device="cuda")
        y = vv.iir(x, dev(sos), state=st, out=yb[:, :n])
        if pad:
            assert torch.all(yb[:, n:] == -9.0) and torch.all(xb[:, n:] == -7.0)   # nothing written between rows
    torch.cuda.synchronize()
    return y.cpu().numpy(), st.cpu().numpy()


def offset_rows(sig, b, n, step=4):
    return np.stack([sig[r * step:r * step + n] for r in range(b)])


def rel_err(y, y64, scale=None):
    return float(np.abs(y.astype(np.float64) - y64).max() / (np.abs(y64).max() if scale is None else scale))


# ------------------------------------------------------------------ exact route
@pytest.mark.parametrize("chunk", [0, None])
def test_iir_exact_matches_reference(vdev, knob, sig, ref, chunk):
    knob("IIR_CHUNK", chunk)
    vdev.debug_clear("STAT_IIR_EXACT")
    vdev.debug_clear("STAT_IIR_CHUNKED")
    for name in IIR_CASCADES:
        y, z = run_iir(vdev, ref[name + "_sos"], sig[:IIR_N])
        assert np.array_equal(y[0], ref[name + "_y"]), name
        assert np.array_equal(z[0], ref[name + "_z"]), name
    assert vdev.debug_get("STAT_IIR_EXACT") == 4 and vdev.debug_get("STAT_IIR_CHUNKED") == 0


@pytest.mark.parametrize("batch", [1, 3, 64, 65, 130])
def test_iir_exact_batches_and_strides(vdev, sig, ref, batch):
    rows = offset_rows(sig, batch, 1000)
    for name in "ad":
        sos = ref[name + "_sos"]
        want_y, want_z = cascade_model(sos, rows)
        for pad in (0, 5):
            y, z = run_iir(vdev, sos, rows, pad=pad)
            assert np.array_equal(y, want_y) and np.array_equal(z, want_z), (name, pad)


def test_iir_exact_in_place_and_incoming_state(vdev, sig, ref):
    rows = offset_rows(sig, 5, 777)
    sos = ref["a_sos"]
    _, z0 = cascade_model(sos, offset_rows(sig, 5, 300, step=11))   # some non-zero states
    want_y, want_z = cascade_model(sos, rows, state=z0)
    y, z = run_iir(vdev, sos, rows, state=z0, inplace=True)
    assert np.array_equal(y, want_y) and np.array_equal(z, want_z)


@pytest.mark.parametrize("cut", IIR_CUTS)
def test_iir_stream_of_calls_equals_one_shot(vdev, sig, ref, cut):
    """the state tensor carries the stream; one-sample calls over the first 500
    samples only (a launch each), the rest of the row in calls of 1000"""
    for name in IIR_CASCADES:
        sos = dev(ref[name + "_sos"])
        x = dev(sig[:IIR_N])
        y = torch.empty_like(x)
        st = torch.zeros((1, len(ref[name + "_sos"]), 2), dtype=torch.float32, device="cuda")
        i = 0
        while i < IIR_N:
            step = cut if (cut > 1 or i < 500) else 1000
            step = min(step, IIR_N - i)
            vdev.iir(x[i:i + step], sos, state=st, out=y[i:i + step])
            i += step
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy(), ref[name + "_y"]), name
        assert np.array_equal(st.cpu().numpy()[0], ref[f"{name}_z_cut{cut}"]), name


@pytest.mark.parametrize("stages", [0, 1, 2, 5, CAP, CAP + 3])
def test_iir_stage_counts(vdev, sig, ref, stages):
    """cascades built by repeating fixture stages; above the cap the kernel runs
    groups of stages through the output rows"""
    pool = np.concatenate([ref["a_sos"], ref["d_sos"], ref["c_sos"]])
    sos = np.stack([pool[s % len(pool)] for s in range(stages)]) if stages else np.zeros((0, 5), np.float32)
    rows = offset_rows(sig, 3, 1000)
    want_y, want_z = cascade_model(sos, rows)
    y, z = run_iir(vdev, sos, rows)
    assert np.array_equal(y, want_y) and np.array_equal(z, want_z)
    if stages:
        y, z = run_iir(vdev, sos, rows, inplace=True)
        assert np.array_equal(y, want_y) and np.array_equal(z, want_z)


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_iir_lengths_around_the_tile(vdev, sig, ref, n):
    rows = offset_rows(sig, 3, n)
    want_y, want_z = cascade_model(ref["a_sos"], rows)
    y, z = run_iir(vdev, ref["a_sos"], rows, pad=3)
    assert np.array_equal(y, want_y) and np.array_equal(z, want_z)


def test_iir_host_entry_writes_states_back(api, sig, ref):
    for name in IIR_CASCADES:
        sos = ref[name + "_sos"]
        st, y, z = api.iir(sos, sig[:IIR_N])
        assert st == OK and np.array_equal(y, ref[name + "_y"]) and np.array_equal(z, ref[name + "_z"]), name
        st, y, z = api.iir(sos, sig[:IIR_N], inplace=True)
        assert st == OK and np.array_equal(y, ref[name + "_y"]) and np.array_equal(z, ref[name + "_z"]), name
    # a following call continues the stream from the structs
    bq = api.biquads(ref["a_sos"])
    parts = [api.apply_structs(bq, 4, sig[a:b]) for a, b in ((0, 2500), (2500, IIR_N))]
    assert all(p[0] == OK for p in parts) and np.array_equal(np.concatenate([p[1] for p in parts]), ref["a_y"])
    st, y, _ = api.iir(ref["a_sos"][:0], sig[:100])                # no stages: a copy
    assert st == OK and np.array_equal(y, sig[:100])


def test_biquad_process_interleaved_with_apply(api, sig, ref):
    y, z = mix_run(api, ref["b_sos"], sig[:IIR_N])
    assert np.array_equal(y, ref["mix_y"]) and np.array_equal(z, ref["mix_z"])


# ---------------------------------------------------------------- chunked route
@pytest.fixture(scope="module")
def f64_long(sig, ref):
    """the f64 model over the fixture row and the 500 samples after it"""
    return {name: cascade_model(ref[name + "_sos"], sig[:IIR_N + 500], dtype=np.float64)[0] for name in IIR_CASCADES}


@pytest.mark.parametrize("chunk", [32, 64, 256, 33])
def test_iir_chunked_within_twice_the_reference_error(vdev, knob, sig, ref, f64, f64_long, chunk):
    vdev.debug_clear("STAT_IIR_EXACT")
    vdev.debug_clear("STAT_IIR_CHUNKED")
    for name in IIR_CASCADES:
        sos, y64, err_ref = ref[name + "_sos"], f64[name + "_y"], float(ref[name + "_err_ref"])
        knob("IIR_CHUNK", chunk)
        y, z = run_iir(vdev, sos, sig[:IIR_N])
        err = rel_err(y[0], y64)
        # the chunked call's final state continues the stream on the exact route
        knob("IIR_CHUNK", 0)
        y2, _ = run_iir(vdev, sos, sig[IIR_N:IIR_N + 500], state=z)
        err2 = rel_err(y2[0], f64_long[name][IIR_N:], scale=np.abs(y64).max())
        print(f"iir chunk {chunk} cascade {name}: err/err_ref {err / err_ref:.3f}, continued {err2 / err_ref:.3f} "
              f"(err_ref {err_ref:.3g})")
        assert err <= BOUND * err_ref, (name, chunk, err, err_ref)
        assert err2 <= BOUND * err_ref, (name, chunk, err2, err_ref)
    assert vdev.debug_get("STAT_IIR_CHUNKED") == 4 and vdev.debug_get("STAT_IIR_EXACT") == 4


def test_iir_route_rule_row_alone_equals_row_in_batch(vdev, knob, sig, ref):
    """forced chunks, and the default rule on rows beyond the exact route's
    length (chunks of 1024 with a short tail): a row's output does not depend on
    the batch it is computed in, nor on the strides"""
    long_rows = np.stack([np.resize(np.roll(sig, 17 * r), 20000) for r in range(7)]).astype(np.float32)
    for chunk, rows in ((64, offset_rows(sig, 7, IIR_N, step=9)), (None, long_rows)):
        knob("IIR_CHUNK", chunk)
        vdev.debug_clear("STAT_IIR_CHUNKED")
        y, z = run_iir(vdev, ref["a_sos"], rows)
        for r in (0, 3, 6):
            y1, z1 = run_iir(vdev, ref["a_sos"], rows[r], pad=7)
            assert np.array_equal(y1[0], y[r]) and np.array_equal(z1[0], z[r]), (chunk, r)
        assert vdev.debug_get("STAT_IIR_CHUNKED") == 4


def test_iir_default_route_on_long_rows_within_bound(vdev, sig, ref):
    """n = 20000 > 8192 takes the chunked route by default; err_ref here is the
    float32 model's (= the reference's) own error on this row"""
    row = np.resize(sig, 20000).astype(np.float32)
    for name in "ab":
        sos = ref[name + "_sos"]
        y64 = cascade_model(sos, row, dtype=np.float64)[0]
        err_ref = rel_err(cascade_model(sos, row)[0], y64)
        vdev.debug_clear("STAT_IIR_CHUNKED")
        y, _ = run_iir(vdev, sos, row)
        assert vdev.debug_get("STAT_IIR_CHUNKED") == 1
        err = rel_err(y[0], y64)
        print(f"iir default route n 20000 cascade {name}: err/err_ref {err / err_ref:.3f} (err_ref {err_ref:.3g})")
        assert err <= BOUND * err_ref, (name, err, err_ref)


@pytest.mark.parametrize("chunk", [IIR_N, IIR_N + 1000])
def test_iir_chunk_not_below_n_is_the_exact_route(vdev, knob, sig, ref, chunk):
    knob("IIR_CHUNK", chunk)
    vdev.debug_clear("STAT_IIR_EXACT")
    vdev.debug_clear("STAT_IIR_CHUNKED")
    for name in IIR_CASCADES:
        y, z = run_iir(vdev, ref[name + "_sos"], sig[:IIR_N])
        assert np.array_equal(y[0], ref[name + "_y"]) and np.array_equal(z[0], ref[name + "_z"]), name
    assert vdev.debug_get("STAT_IIR_EXACT") == 4 and vdev.debug_get("STAT_IIR_CHUNKED") == 0


@pytest.mark.parametrize("chunk", [0, 64])
def test_iir_nan_row(vdev, knob, sig, ref, f64, chunk):
    knob("IIR_CHUNK", chunk)
    row = sig[:IIR_N].copy()
    row[IIR_NAN_AT] = np.nan
    for name in IIR_CASCADES:
        y, _ = run_iir(vdev, ref[name + "_sos"], row)
        assert np.all(np.isnan(y[0][IIR_NAN_AT:])), name
        head = y[0][:IIR_NAN_AT]
        if chunk == 0:
            assert np.array_equal(head, ref[name + "_y_nan"][:IIR_NAN_AT]), name
        else:
            y64 = f64[name + "_y"]
            assert rel_err(head, y64[:IIR_NAN_AT], scale=np.abs(y64).max()) <= BOUND * float(ref[name + "_err_ref"])


# ------------------------------------------------------------- Savitzky-Golay
@pytest.fixture(scope="module")
def sg():
    d = load("savgol_signal")
    d.update(load("savgol_coeffs"))
    return d


@pytest.mark.parametrize("mode", SAVGOL_MODES)
def test_savgol_matches_reference(vdev, sg, mode):
    rec = load(f"savgol_mode{mode}")
    for i, (m, p, deriv, delta) in enumerate(SAVGOL_CASES):
        for n in savgol_lengths(m):
            y = vdev.savgol(dev(sg["x"][:n]), m, p, deriv, delta, mode).cpu().numpy()
            assert np.array_equal(y, rec[f"c{i}_n{n}"]), (mode, m, p, deriv, n)


@pytest.mark.parametrize("batch", [1, 5, 67])
def test_savgol_batches_and_strides(vdev, sg, batch):
    n = 1500                                      # two spans per row, the second short
    rows = np.stack([sg["x"][3 * r:3 * r + n] for r in range(batch)])
    for i, mode in ((4, 0), (5, 3), (6, 1)):
        m, p, deriv, delta = SAVGOL_CASES[i]
        want = savgol_model(rows, sg[f"h{i}"], mode)
        xb = torch.full((batch, n + 5), -7.0, dtype=torch.float32, device="cuda")
        xb[:, :n] = dev(rows)
        yb = torch.full((batch, n + 3), -9.0, dtype=torch.float32, device="cuda")
        vdev.savgol(xb[:, :n], m, p, deriv, delta, mode, out=yb[:, :n])
        assert np.array_equal(yb[:, :n].cpu().numpy(), want), (i, mode)
        assert torch.all(yb[:, n:] == -9.0)
        vdev.savgol(xb[:, :n], m, p, deriv, delta, mode, out=xb[:, :n])   # in place: the rows are staged
        assert np.array_equal(xb[:, :n].cpu().numpy(), want), (i, mode)


def test_savgol_nan_policies(vdev, sg):
    rec = load("savgol_misc")
    m, p, deriv, delta, mode = SAVGOL_POLICY_CASE
    L = vdev.lib()
    L.vv_dsp_set_nan_policy.argtypes = [C.c_int]
    L.vv_dsp_set_nan_policy.restype = None
    try:
        for policy in range(4):
            L.vv_dsp_set_nan_policy(policy)
            want_st = int(rec[f"policy{policy}_status"])
            if want_st != OK:
                assert want_st == ERR_NAN
                with pytest.raises(vdev.VvError, match="status 5"):
                    vdev.savgol(dev(sg["bad"]), m, p, deriv, delta, mode)
                continue
            y = vdev.savgol(dev(sg["bad"]), m, p, deriv, delta, mode).cpu().numpy()
            assert np.array_equal(y, rec[f"policy{policy}_y"], equal_nan=True), policy
    finally:
        L.vv_dsp_set_nan_policy(0)


def test_savgol_host_entry_equals_device_entry(api, vdev, sg):
    rec, misc = load("savgol_mode0"), load("savgol_misc")
    for i in (2, 4, 6):
        m, p, deriv, delta = SAVGOL_CASES[i]
        st, y = api.savgol(sg["x"][:300], m, p, deriv, delta, 0)
        assert st == OK and np.array_equal(y, rec[f"c{i}_n300"])
        assert np.array_equal(y, vdev.savgol(dev(sg["x"][:300]), m, p, deriv, delta, 0).cpu().numpy())
    m, p, deriv, delta, mode = SAVGOL_POLICY_CASE
    try:
        for policy in range(4):
            api.set_nan_policy(policy)
            st, y = api.savgol(sg["bad"], m, p, deriv, delta, mode)
            assert st == int(misc[f"policy{policy}_status"]), policy
            assert np.array_equal(y, misc[f"policy{policy}_y"], equal_nan=True), policy   # untouched under ERROR
    finally:
        api.set_nan_policy(0)
    want = dict(zip((str(s) for s in misc["arg_names"]), (int(s) for s in misc["arg_status"])))
    for name, st in api.savgol_argument_cases().items():
        assert st == want[name], (name, st, want[name])
    iir = load("iir_ref")
    want = dict(zip((str(s) for s in iir["arg_names"]), (int(s) for s in iir["arg_status"])))
    for name, st in api.iir_argument_cases().items():
        assert st == want[name], (name, st, want[name])
