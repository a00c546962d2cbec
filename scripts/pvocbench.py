#!/usr/bin/env python3
"""The phase vocoder on one MI355X: 32 channels x 10 minutes at 16 kHz, n_fft 1024 /
hop 256 (37,498 analysis rows of 513 bins per channel).

  rows_rate_<r>     vv_dsp_phase_vocoder_uniform_device on resident complex rows at
              rates 0.5, 1.25 and 2 (start 0, step r, every position below T);
  signal_rate_1.25  signal -> signal (vv_dsp_stft_time_stretch_device);
  rows_rate_<r>_plane  the same jobs with knob PVOC_PLANE = 1: the analysis rows' phases
              stored once in an f64 plane that both walks read, instead of a second
              atan2 (same bits; the default is whichever this run showed faster);
  torch_rate_1.25   the same definition as a torch expression (angle, cumsum, polar
              in float64) on the same rows.
Beside each rows job, from the same run:
  ceiling     a streaming kernel that moves the job's bytes once (membench k_rwmix:
              the lower halves of the analysis rows read, the output rows written);
  f64_floor   the job's f64 vector instructions at the 78.65 Tflop/s f64 vector
              peak, each counted as one fused multiply-add slot: F64_PER_ROW per
              analysis row a walk loads (both passes; the loads are counted by
              replaying the walks' two-row reuse on the job's positions) and
              F64_PER_OUT per output value, the counts of this build's gfx950
              listing of k_pvoc_rows.
Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.  A
seeded sample of rows and bins of two channels of every job is checked in the run
against the f64 model of tests/pvoc_util.py by its rule (<= 2^-23 m_j); the torch
expression, whose cumsum has another order, at 1e-5 m_j; the signal job's two
sampled channels must equal spectrum -> vocoder -> reconstruct -> divide bit for
bit.  Prints one JSON line.

    python scripts/pvocbench.py [--reps 5] [--seconds 600] [--channels 32] [--json FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vv-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vvdsp_amd as vv  # noqa: E402
import pvoc_util as pu  # noqa: E402

NFFT, HOP, K = 1024, 256, 513
RATES = (0.5, 1.25, 2.0)
PEAK_F64 = 78.65e12
# f64 vector instructions in the gfx950 listing of k_pvoc_rows<OUT, PLANE = false>:
# <false> holds 105 with the row load inlined twice; <true> holds 264 with the row load
# (now with the magnitude's sqrt) inlined twice.  They hold for the compiler named in
# F64_COUNTED_ON; `python scripts/pvocbench.py --count-f64` (needs hipcc, no GPU) prints
# the counts of the present sources and compiler, to be copied here when they move.
F64_PER_ROW, F64_PER_ROW_MAG, F64_PER_OUT = 52, 60, 144
F64_COUNTED_ON = "AMD clang 22.0.0git roc-7.2.0 (HIP 7.2.26015), -O3 --offload-arch=gfx950: <false> 105, <true> 264"
SAMPLE_BINS, SAMPLE_ROWS = 16, 64


def count_f64():
    """f64 vector instructions of each kernel of pvoc_kernels.hip in a fresh gfx950 listing"""
    import re
    import subprocess
    import tempfile
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[:2]
    with tempfile.TemporaryDirectory() as tmp:
        lst = os.path.join(tmp, "pvoc.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "vv-dsp_amd", "csrc", "host"), "--cuda-device-only", "-S",
                        os.path.join(ROOT, "vv-dsp_amd", "csrc", "hip", "pvoc_kernels.hip"), "-o", lst],
                       check=True, stderr=subprocess.DEVNULL)
        lines = open(lst).read().splitlines()
    counts, name = {}, None
    for ln in lines:
        if re.match(r"_ZN3vvh\S*k_pvoc\w*:", ln):
            name = subprocess.run(["c++filt", ln.split(":")[0]], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
            counts[name] = [0, 0]
        elif name and ln.strip() == "s_endpgm":
            name = None
        elif name and ln.startswith("\t") and not ln.strip().startswith((".", ";")):
            counts[name][0] += 1
            counts[name][1] += "f64" in ln.split()[0]
    print(json.dumps({"compiler": ver, "instructions_total_and_f64": counts,
                      "in_use": [F64_PER_ROW, F64_PER_ROW_MAG, F64_PER_OUT], "in_use_counted_on": F64_COUNTED_ON}))


def timed(fn, reps, burst):
    for _ in range(2):
        fn()
    s = torch.cuda.current_stream()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(s)
        fn()
        b.record(s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(burst):
        fn()
    e1.record(s)
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return float(np.median(t)), float(np.min(t)), e0.elapsed_time(e1) / burst


def signal(nch, n, rate, seed):
    """a gliding three-harmonic tone per channel, gated, over noise: float32 on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / rate
    x = torch.empty(nch, n, device="cuda", dtype=torch.float32)
    for c in range(nch):
        f = 180.0 + 35.0 * c + 60.0 * torch.sin(2 * np.pi * 0.21 * t + c)
        ph = 2 * np.pi * torch.cumsum(f, 0) / rate
        tone = torch.sin(ph) + 0.5 * torch.sin(2 * ph + 0.4) + 0.25 * torch.sin(3 * ph + 1.1)
        gate = (torch.sin(2 * np.pi * 0.9 * t + 0.5 * c) > -0.3).to(torch.float64)
        noise = torch.randn(n, device="cuda", generator=g, dtype=torch.float32)
        x[c] = (0.3 * gate * tone).to(torch.float32) + 0.02 * noise
    return x


def ceiling(src, dst, bytes_read, bytes_written, reps, burst):
    path = os.path.join(ROOT, "scripts", "libmembench.so")
    if not os.path.exists(path):
        raise SystemExit("scripts/libmembench.so missing: run `make -C vv-dsp_amd membench`")
    mb = C.CDLL(path)
    mb.membench_rwmix.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
    n_in4, n_out4 = bytes_read // 16, bytes_written // 16
    assert n_in4 * 16 <= src.numel() * 8 and n_out4 * 16 <= dst.numel() * 8
    s = torch.cuda.current_stream().cuda_stream
    best = None
    for blocks in (2048, 4096, 8192):
        def fn(blocks=blocks):
            assert mb.membench_rwmix(src.data_ptr(), dst.data_ptr(), n_in4, n_out4, blocks, s) == 0
        t = timed(fn, reps, burst)
        if best is None or t[0] < best[1][0]:
            best = (blocks, t)
    return {"what": "streaming kernel moving the job's bytes once (membench k_rwmix, float4 per lane, best of 3 "
                    "grid sizes)", "bytes_read": n_in4 * 16, "bytes_written": n_out4 * 16, "blocks": best[0],
            "ms": round(best[1][0], 4), "ms_min": round(best[1][1], 4),
            "GBps": round((n_in4 + n_out4) * 16 / best[1][0] / 1e6, 1)}


def row_loads(p, T):
    """analysis rows one pass of the walks loads for positions p: each segment starts
    with nothing held and keeps the two rows it used last; rows >= T cost nothing"""
    loads = 0
    t0s = np.floor(p).astype(np.int64)
    for j0 in range(0, len(p), pu.S):
        held = (-1, -1)
        for t0 in t0s[j0:j0 + pu.S]:
            for t in (t0, t0 + 1):
                if t not in held and t < T:
                    loads += 1
            held = (t0, t0 + 1)
    return loads


def f64_floor(p, T, nch):
    loads = row_loads(p, T)
    m = len(p)
    first_pass = row_loads(p[:(m - 1) // pu.S * pu.S], T)     # the last segment's total is never formed
    instr = (first_pass * F64_PER_ROW + loads * F64_PER_ROW_MAG + m * F64_PER_OUT) * nch * K
    return {"what": "f64 vector instructions of the two walks, each as one FMA slot at 78.65 Tflop/s",
            "row_loads_per_channel": [int(first_pass), int(loads)], "output_rows": m, "f64_instructions": int(instr),
            "atan2_calls": int((first_pass + loads) * nch * K), "sincos_calls": int(m * nch * K),
            "ms": round(2.0 * instr / PEAK_F64 * 1e3, 4)}


def sample(m, seed):
    rng = np.random.default_rng(seed)
    rows = sorted({0, 1, pu.S - 1, pu.S, m - 1} | {int(r) for r in rng.integers(0, m, SAMPLE_ROWS)})
    bins = sorted({0, 1, K - 1} | {int(b) for b in rng.integers(0, K, SAMPLE_BINS - 3)})
    return rows, bins


def model_of(spec, c, bins, p):
    """the model on bins `bins` of channel c: they stand as bins 0.. of rows of
    n_fft 2 len(bins) - 2, which changes no value of theirs"""
    nb = len(bins)
    D = np.zeros((spec.shape[1], 2 * nb - 2), np.complex64)
    D[:, :nb] = spec[c][:, bins].cpu().numpy()
    return pu.model(D, 2 * nb - 2, p)


def check_rows(out, spec, p, seed, limit=2.0 ** -23):
    """out [nch][m][NFFT] on the device against the model on a seeded sample"""
    nch, m = out.shape[0], out.shape[1]
    rows, bins = sample(m, seed)
    worst, exact, total, mirrored = 0.0, 0, 0, True
    for c in sorted({0, nch - 1}):
        mdl = model_of(spec, c, bins, p)
        got = out[c][rows][:, bins].cpu().numpy()
        want, mj = mdl["out"][rows][:, :len(bins)], mdl["mj"][rows]
        inner = [i for i, b in enumerate(bins) if 0 < b < NFFT // 2]
        mirror = out[c][rows][:, [NFFT - bins[i] for i in inner]].cpu().numpy()
        mirrored &= bool(np.array_equal(mirror, np.conj(got[:, inner])))
        for g, w in ((got.real, want.real), (got.imag, want.imag)):
            err = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.maximum(mj, 1e-300)
            worst = max(worst, float(err.max()))
            exact += int(np.sum(g == w))
            total += g.size
    return {"ok": bool(worst <= limit and mirrored), "max_err_over_m": float(f"{worst:.3g}"), "limit": limit, "values": total,
            "bit_equal": exact, "what": f"{len(rows)} seeded rows x {len(bins)} bins of the first and last channel "
            "vs the f64 model; mirror bins are the conjugates"}


def torch_pvoc(spec, p):
    """the definition as a user would write it in torch: float64 angle, cumsum, polar"""
    nch, T = spec.shape[0], spec.shape[1]
    half = spec[..., :K]
    pad = torch.zeros((nch, 2, K), dtype=torch.float64, device=spec.device)
    mag = torch.cat([half.abs().to(torch.float64), pad], 1)
    th = torch.cat([torch.angle(half.to(torch.complex128)), pad], 1)
    t0 = torch.floor(p).to(torch.int64)
    a = (p - torch.floor(p))[None, :, None]
    mj = (1.0 - a) * mag[:, t0] + a * mag[:, t0 + 1]
    d = th[:, t0 + 1] - th[:, t0]
    phi = th[:, t0[:1]] + (torch.cumsum(d, 1) - d)
    low = torch.polar(mj, phi).to(torch.complex64)
    out = torch.empty((nch, p.numel(), NFFT), dtype=torch.complex64, device=spec.device)
    out[..., :K] = low
    out[..., K:] = torch.conj(low[..., 1:K - 1]).flip(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "pvoc_bench.json"))
    ap.add_argument("--count-f64", action="store_true", help="print the kernels' f64 instruction counts and exit")
    o = ap.parse_args()
    if o.count_f64:
        return count_f64()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("pvocbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    nch, fs = o.channels, 16000
    n = o.seconds * fs
    x = signal(nch, n, fs, 20261020)
    st = vv.Stft(NFFT, HOP)
    spec = st.spectrogram(x, complex_out=True)
    T = spec.shape[1]
    workload = f"{nch} ch x {o.seconds} s at {fs} Hz, n_fft {NFFT} hop {HOP}: {T} analysis rows of {K} bins per channel"
    jobs, res = [], {}

    def report(name, what, t, check, **extra):
        med, mn, b2b = t
        job = {"job": name, "workload": workload + what, "ms": round(med, 4), "ms_min": round(mn, 4),
               "ms_back_to_back": round(b2b, 4), "check": check}
        job.update(extra)
        jobs.append(job)
        return job

    rows_125 = None
    for rate in RATES:
        m = pu.stretch_rows(T, rate)
        p = pu.uniform_positions(0.0, rate, m)
        out = torch.empty((nch, m, NFFT), dtype=torch.complex64, device="cuda")

        def rows_job(rate=rate, m=m, out=out):
            vv.phase_vocoder(spec, NFFT, 0.0, rate, m=m, out=out)
        vv.debug_clear("STAT_PVOC_ROWS")
        t = timed(rows_job, o.reps, o.burst)
        calls = vv.debug_get("STAT_PVOC_ROWS")
        check = check_rows(out, spec, p, 7)
        # the alternative: the rows' phases stored in an f64 plane instead of a second atan2
        out2 = torch.empty_like(out)

        def plane_job(rate=rate, m=m, out2=out2):
            vv.phase_vocoder(spec, NFFT, 0.0, rate, m=m, out=out2)
        with vv.knobs(PVOC_PLANE=1):
            tp = timed(plane_job, o.reps, o.burst)
        same = torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(out2).view(torch.int32))
        del out2
        report(f"rows_rate_{rate:g}_plane", f", the same job with knob PVOC_PLANE = 1 (phases through an f64 plane)", tp,
               {"ok": bool(same), "what": f"every bit equal to rows_rate_{rate:g}"}, plane_bytes=8 * nch * T * K,
               times_default=round(tp[0] / t[0], 3))
        touched = min(T, int(np.floor(p[-1])) + 2)
        b_in, b_out = nch * touched * K * 8 // 16 * 16, nch * m * NFFT * 8
        ceil = ceiling(spec, out, b_in, b_out, o.reps, o.burst)
        floor = f64_floor(p, T, nch)
        report(f"rows_rate_{rate:g}", f", resident rows -> {m} output rows per channel", t, check, output_rows=m,
               bytes_read_once=b_in, bytes_written=b_out, GBps=round((b_in + b_out) / t[0] / 1e6, 1), ceiling=ceil,
               f64_floor=floor, times_ceiling=round(t[0] / ceil["ms"], 3), times_f64_floor=round(t[0] / floor["ms"], 3),
               calls_counted=calls == 2 + o.reps + o.burst,
               scratch_bytes=8 * nch * K * ((m + pu.S - 1) // pu.S + 1))
        if rate == 1.25:
            rows_job()               # the ceiling wrote over the rows
            rows_125 = out
        else:
            del out
    torch.cuda.empty_cache()

    # signal -> signal at 1.25
    rate = 1.25
    m, ln = st.time_stretch_length(n, rate)
    y = torch.empty((nch, ln), dtype=torch.float32, device="cuda")

    def signal_job():
        st.time_stretch(x, rate, out=y)
    ts = timed(signal_job, o.reps, o.burst)
    same = True
    for c in sorted({0, nch - 1}):
        acc = torch.zeros(ln, dtype=torch.float32, device="cuda")
        norm = torch.zeros(ln, dtype=torch.float32, device="cuda")
        st.reconstruct(rows_125[c], acc, norm)
        a, w = acc.cpu().numpy(), norm.cpu().numpy()
        with np.errstate(all="ignore"):
            want = np.where(w > pu.NORM_FLOOR, a / w, np.float32(0))
        same &= bool(np.array_equal(want.view(np.uint32), y[c].cpu().numpy().view(np.uint32)))

    def spectrum_job():
        st.spectrogram(x, out=spec, complex_out=True)
    tspec = timed(spectrum_job, o.reps, o.burst)
    report("signal_rate_1.25", f", signal -> signal of {ln} samples per channel, rows in scratch by channel groups", ts,
           {"ok": same, "what": "first and last channel bit-identical to spectrum -> rows_rate_1.25 -> reconstruct -> "
            "float division"}, output_samples=ln, spectrum_alone_ms=round(tspec[0], 4))

    # the torch expression at 1.25
    p = pu.uniform_positions(0.0, rate, m)
    pt = torch.from_numpy(p).cuda()

    def torch_job():
        res["t"] = None
        res["t"] = torch_pvoc(spec, pt)
    tt = timed(torch_job, 2, 2)
    check = check_rows(res["t"], spec, p, 7, limit=1e-5)
    lib_ms = next(j["ms"] for j in jobs if j["job"] == "rows_rate_1.25")
    report("torch_rate_1.25", ", the definition as a float64 torch expression (angle, cumsum, polar)", tt, check,
           library_speedup=round(tt[0] / lib_ms, 2))

    line = {"bench": "phase_vocoder", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "segment": pu.S, "f64_per_row_load": [F64_PER_ROW, F64_PER_ROW_MAG], "f64_per_output": F64_PER_OUT,
            "f64_counted_on": F64_COUNTED_ON, "hip_runtime": str(torch.version.hip),
            "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
