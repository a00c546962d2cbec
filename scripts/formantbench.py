#!/usr/bin/env python3
"""LSF / reflection coefficients and formants of LPC rows on one MI355X: 32 channels
x 10 minutes at 16 kHz, frames of 400, hop 160, Hamming (1.92 M rows).

  lpc_frames_<p>          signal -> LPC rows alone, for scale (orders 16 and 32);
  rows_lsf_<p>            resident LPC rows -> lsf + rc + flags;
  rows_formants_<p>       resident LPC rows -> freq + bw + count + flags;
  signal_lsf_<p>, signal_formants_<p>   both from the signal (LPC rows in scratch).

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.  A
seeded sample of rows of every job is checked in the run against the numpy models
of tests/lsf_util.py and tests/formant_util.py: rc, flags and counts equal, lsf,
freq and bw equal or adjacent floats; the jobs from the signal bit-identical to
the jobs on the rows.

Beside each time stands its floor: the f64 vector operations of the definition
(one per add, multiply or divide; acos, atan2 and log not counted), with the
sample's mean iteration count for Aberth, at the chip's 78.65 T/s f64 vector peak --
and at half of it, since the definition fuses nothing and an unfused operation is
one instruction where the peak counts two.  And its baselines on the same rows:
torch.linalg.eigvals of the companion matrices on the device (on a slice, if this
torch build has it there; the line says if not), and np.roots on one host core
over a sample.  Prints one JSON line.

    python scripts/formantbench.py [--reps 5] [--seconds 600] [--channels 32] [--json FILE]
"""
import argparse
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
import formant_util as fu  # noqa: E402
import lsf_util as lu  # noqa: E402
from frames_util import hamming  # noqa: E402

FRAME, HOP, RATE = 400, 160, 16000
ORDERS = (16, 32)
SAMPLE = 48
PEAK = 78.65e12          # f64 vector operations per second, an FMA counted as two
LSF_OUT = ("lsf", "rc", "flags")
FMT_OUT = ("freq", "bw", "count", "flags")


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


def signal(nch, n, seed):
    """per channel: a gliding pulse-like source through three slowly moving resonances, over
    noise -- built as a sum of harmonics weighted by the resonances; float32 on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / RATE
    x = torch.empty(nch, n, device="cuda", dtype=torch.float32)
    for c in range(nch):
        f0 = 110.0 + 6.0 * c + 25.0 * torch.sin(2 * np.pi * 0.17 * t + c)
        ph = 2 * np.pi * torch.cumsum(f0.double(), 0).float() / RATE
        acc = torch.zeros_like(t)
        for h in range(1, 28):
            fh = h * (110.0 + 6.0 * c)
            w = sum(1.0 / (1.0 + ((fh - fc) / bw) ** 2) for fc, bw in
                    ((600.0 + 20 * c, 90.0), (1400.0 + 30 * c, 120.0), (2700.0, 160.0)))
            acc += float(w) * torch.sin(h * ph + 0.37 * h)
        noise = torch.randn(n, device="cuda", generator=g, dtype=torch.float32)
        x[c] = 0.2 * acc / acc.abs().max() + 0.01 * noise
    return x


def lsf_ops(p):
    """f64 operations of one row of lpc_to_lsf (include/vv_dsp/envelope/lsf.h)"""
    step_down = sum(2 + 3 * (m - 1) for m in range(1, p + 1))
    M1, M2 = (p + 1) // 2, p // 2
    series = 2 * (p + 2) + 2 * (M1 + M2) + (M1 + M2)
    clen = lambda M: 1 + 3 * M + 3
    scan = (lu.G + 1) * (clen(M1) + clen(M2))
    bisect = sum(M * (clen(M) + lu.BISECTIONS * (2 + clen(M)) + 2) for M in (M1, M2))
    return step_down + series + scan + bisect


def formant_ops(p, iters):
    """f64 operations of one row of the Aberth iteration at `iters` iterations, plus the candidates"""
    per_root = 15 * p + 11 + 15 * (p - 1) + 6 + 1 + 11 + 2 + 3
    return iters * p * per_root + p * 7


def sample_index(rows, seed):
    rng = np.random.default_rng(seed)
    pick = {0, 1, rows - 1}
    while len(pick) < SAMPLE:
        pick.add(int(rng.integers(rows)))
    return np.array(sorted(pick))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burst", type=int, default=3)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "formant_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("formantbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    nch, n = o.channels, o.seconds * RATE
    x = signal(nch, n, 20261021)
    win = torch.from_numpy(np.asarray(hamming(FRAME), np.float32)).cuda()
    fr = vv.num_frames(n, FRAME, HOP)
    rows = nch * fr
    workload = f"{nch} ch x {o.seconds} s at {RATE} Hz, frame {FRAME} hop {HOP} Hamming: {rows} rows"
    pick = sample_index(rows, 11)
    prm_m = fu.default_params(float(RATE))
    prm = vv.FormantParams(*(getattr(prm_m, f) for f, _ in prm_m._fields_))
    jobs, res = [], {}

    def report(name, what, t, check, **extra):
        med, mn, b2b = t
        job = {"job": name, "workload": workload + what, "rows": rows, "ms": round(med, 4), "ms_min": round(mn, 4),
               "ms_back_to_back": round(b2b, 4), "rows_per_s": round(rows / med * 1e3, 1), "check": check}
        job.update(extra)
        jobs.append(job)
        return job

    def floors(ops_per_row):
        total = ops_per_row * rows
        return {"f64_ops_per_row": round(ops_per_row, 1), "floor_ms": round(total / PEAK * 1e3, 4),
                "floor_unfused_ms": round(total / (PEAK / 2) * 1e3, 4)}

    eig = {}
    for p in ORDERS:
        a = torch.empty((nch, fr, p + 1), dtype=torch.float32, device="cuda")
        err = torch.empty((nch, fr), dtype=torch.float32, device="cuda")
        t_lpc = timed(lambda: vv.lpc_frames(x, FRAME, HOP, p, window=win, out=(a, err)), o.reps, o.burst)
        report(f"lpc_frames_{p}", f", signal -> LPC rows of order {p} alone", t_lpc,
               {"ok": bool(torch.isfinite(a).all().item()), "what": "finite (the rows are the other jobs' input)"})
        a2 = a.reshape(rows, p + 1)
        samp = a2[torch.from_numpy(pick).cuda()].cpu().numpy()

        # ---- rows -> lsf + rc + flags
        def lsf_job():
            res["l"] = vv.lpc_to_lsf(a2, LSF_OUT)
        t = timed(lsf_job, o.reps, o.burst)
        m_lsf, m_rc, m_fl = lu.lpc_to_lsf_vec(samp)
        got = {k: v[torch.from_numpy(pick).cuda()].cpu().numpy() for k, v in res["l"].items()}
        try:
            lu.assert_bits(got["rc"], m_rc, "rc")
            lu.assert_bits(got["flags"], m_fl, "flags")
            ex, ulp = lu.assert_adjacent(got["lsf"], m_lsf, "lsf")
            check = {"ok": True, "lsf_exact": ex, "lsf_one_ulp": ulp}
        except AssertionError as e:
            check = {"ok": False, "error": str(e)[:200]}
        check.update(rows=len(pick), complete=int(np.sum(m_fl & lu.COMPLETE != 0)),
                     what="seeded rows vs the numpy model: rc and flags equal, lsf equal or adjacent floats")
        report(f"rows_lsf_{p}", f", resident rows of order {p} -> lsf + rc + flags", t, check, **floors(lsf_ops(p)),
               times_floor_unfused=round(t[0] / floors(lsf_ops(p))["floor_unfused_ms"], 2))

        # ---- rows -> formants
        def fmt_job():
            res["f"] = vv.formants(a2, prm, FMT_OUT)
        t_f = timed(fmt_job, o.reps, o.burst)
        start = vv.formant_start_points(p).numpy()
        m = fu.formants_vec(samp, start, prm_m)
        got = {k: v[torch.from_numpy(pick).cuda()].cpu().numpy() for k, v in res["f"].items()}
        try:
            lu.assert_bits(got["count"], m["count"], "count")
            lu.assert_bits(got["flags"], m["flags"], "flags")
            ef, uf = lu.assert_adjacent(got["freq"], m["freq"], "freq")
            eb, ub = lu.assert_adjacent(got["bw"], m["bw"], "bw")
            check = {"ok": True, "freq_exact": ef, "freq_one_ulp": uf, "bw_exact": eb, "bw_one_ulp": ub}
        except AssertionError as e:
            check = {"ok": False, "error": str(e)[:200]}
        iters = float(np.mean(m["iters"]))
        check.update(rows=len(pick), converged=int(np.sum(m["flags"])), mean_iterations=round(iters, 2),
                     max_iterations=int(np.max(m["iters"])),
                     what="seeded rows vs the numpy model: count and flags equal, freq and bw equal or adjacent floats")
        fl = floors(formant_ops(p, iters))
        # baselines on the same rows
        t0 = time.perf_counter()
        for r in samp:
            np.roots(r.astype(np.float64))
        np_rows_per_s = len(samp) / (time.perf_counter() - t0)
        base = {"np_roots_one_core_rows_per_s": round(np_rows_per_s, 1)}
        if p not in eig:
            sl = min(rows, 8192)
            try:
                comp = torch.zeros((sl, p, p), dtype=torch.float64, device="cuda")
                comp[:, 0, :] = -a2[:sl, 1:].double()
                comp[:, torch.arange(1, p), torch.arange(0, p - 1)] = 1.0
                torch.linalg.eigvals(comp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev = torch.linalg.eigvals(comp)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ours = torch.sort(torch.view_as_complex(vv.formants(a2[:sl], prm, "roots")["roots"]).abs(), -1)[0]
                gap = float((torch.sort(ev.abs(), -1)[0] - ours).abs().nan_to_num(0.0).max().item())
                eig[p] = {"torch_eigvals_rows": sl, "torch_eigvals_rows_per_s": round(sl / dt, 1),
                          "torch_eigvals_max_modulus_gap": float(f"{gap:.3g}")}
            except Exception as e:   # this torch build has no device eigvals
                eig[p] = {"torch_eigvals": "not supported on the device by this torch build: " + str(e)[:120]}
        base.update(eig[p])
        report(f"rows_formants_{p}", f", resident rows of order {p} -> freq + bw + count + flags", t_f, check, **fl,
               times_floor_unfused=round(t_f[0] / fl["floor_unfused_ms"], 2), baselines=base)

        # ---- from the signal
        def sig_lsf():
            res["sl"] = vv.lsf_frames(x, FRAME, HOP, p, LSF_OUT, window=win)
        t = timed(sig_lsf, o.reps, o.burst)
        same = all(torch.equal(res["sl"][k].reshape(res["l"][k].shape).view(torch.int32), res["l"][k].view(torch.int32))
                   for k in LSF_OUT)
        report(f"signal_lsf_{p}", f", signal -> LPC rows of order {p} in scratch -> lsf + rc + flags", t,
               {"ok": bool(same), "what": f"every plane bit-identical to rows_lsf_{p}"},
               scratch_bytes=4 * rows * (p + 2))
        res.pop("sl")
        res.pop("l")

        def sig_fmt():
            res["sf"] = vv.formant_frames(x, FRAME, HOP, p, prm, FMT_OUT, window=win)
        t = timed(sig_fmt, o.reps, o.burst)
        same = all(torch.equal(res["sf"][k].reshape(res["f"][k].shape).view(torch.int32), res["f"][k].view(torch.int32))
                   for k in FMT_OUT)
        report(f"signal_formants_{p}", f", signal -> LPC rows of order {p} in scratch -> formant planes", t,
               {"ok": bool(same), "what": f"every plane bit-identical to rows_formants_{p}"},
               scratch_bytes=4 * rows * (p + 2))
        res.pop("sf")
        res.pop("f")
        del a, a2, err
        torch.cuda.empty_cache()

    line = {"bench": "lsf_formants", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "floor_what": "f64 operations of the definition x rows / 78.65e12 per s (floor_ms) and / 39.3e12 "
                          "(floor_unfused_ms: nothing is fused, so an operation is an instruction); library "
                          "functions not counted",
            "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
