#!/usr/bin/env python3
"""The filter module on one MI355X: 32 channels x 10 minutes of audio at 16 kHz.

Jobs:
  iir4_default  the 4-stage low-pass of the fixtures over the 32 long rows: the
                default route (chunks of 1024, three launches);
  iir4_short    the same cascade over 1024 rows of 4800 samples: the exact route,
                one lane per row;
  iir1_default  one stage (the first-order DC blocker) over the 32 long rows;
  savgol_11     window 11, cubic, reflect, over the 32 long rows;
  savgol_257    window 257, order 5, reflect, over the 32 long rows.
With --sweep the 4-stage job is also timed at forced chunk lengths (knob
IIR_CHUNK), which is how N0 and L were chosen.

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.  Every
job moves at least one read and one write of 4 B per sample, which is what a
copy moves: the ceiling is a streaming copy kernel (scripts/membench.hip k_rw)
over the same samples, timed in the same process in the same way, and each job
reports its fraction of it.  Each job is checked in the run against an f64
model: windows of the long rows (a cascade's window is computed from zero state
4000 samples earlier, where the slowest pole's transient is below 1e-8), whole
short rows.  Prints one JSON line.

    python scripts/filterbench.py [--reps 10] [--seconds 600] [--channels 32] [--sweep] [--json FILE]
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
import filter_util as fu  # noqa: E402

WARM = 4000        # samples of run-in before a checked window of a cascade
IIR_RTOL = 2e-5    # of the window's peak: ten times the reference's own error on the fixture rows
SG_RTOL = 1e-6     # one float rounding of a sum of like-signed terms, with room for cancellation


def timed(fn, reps, burst):
    for _ in range(3):
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


def copy_ceiling(x, y, reps, burst):
    path = os.path.join(ROOT, "scripts", "libmembench.so")
    if not os.path.exists(path):
        raise SystemExit("scripts/libmembench.so missing: run `make -C vv-dsp_amd membench`")
    mb = C.CDLL(path)
    mb.membench_rw.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    s = torch.cuda.current_stream().cuda_stream
    best = None
    for blocks in (2048, 4096, 8192):
        def fn(blocks=blocks):
            assert mb.membench_rw(x.data_ptr(), y.data_ptr(), x.numel() // 4, 1, blocks, s) == 0
        t = timed(fn, reps, burst)
        if best is None or t[0] < best[1][0]:
            best = (blocks, t)
    assert torch.equal(x.view(-1)[:x.numel() // 4 * 4], y.view(-1)[:x.numel() // 4 * 4])
    return {"what": "streaming copy of the same samples (membench k_rw, float4 per lane, best of 3 grid sizes)",
            "blocks": best[0], "ms": round(best[1][0], 4), "ms_min": round(best[1][1], 4),
            "ms_back_to_back": round(best[1][2], 4)}


def windows(n):
    """starts of the checked windows of a long row: the row's start, a chunk
    boundary in the middle, the row's end"""
    return sorted({0, max(0, (n // 2) // 1024 * 1024 - 1500), max(0, n - 3000)})


def check_iir(x, y, sos, rows, whole):
    worst, ok = 0.0, True
    n = x.shape[1]
    for r in rows:
        for s in ([0] if whole else windows(n)):
            e = n if whole else min(n, s + 3000)
            s0 = max(0, s - WARM)
            want = fu.cascade_model(sos, x[r, s0:e].cpu().numpy(), dtype=np.float64)[0][s - s0:]
            d = np.abs(y[r, s:e].cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
            worst = max(worst, float(d))
            ok = ok and bool(d <= IIR_RTOL)
    return {"ok": bool(ok), "max_err_of_peak": worst,
            "what": f"{'whole rows' if whole else 'windows of 3000 samples'} of rows {list(rows)} vs the f64 cascade, "
                    f"max error <= {IIR_RTOL} of the window's peak"}


def check_savgol(x, y, h, rows):
    worst, ok = 0.0, True
    n, half = x.shape[1], len(h) // 2
    h64 = h.astype(np.float64)
    for r in rows:
        for s in windows(n):
            e = min(n, s + 3000)
            lo, hi = max(0, s - half), min(n, e + half)
            seg = x[r, lo:hi].cpu().numpy()
            # the model pads what it is given: only outputs whose window lies inside the
            # segment, or at a true end of the row, are compared
            want = fu.savgol_model(seg, h, 0).astype(np.float64)
            a = 0 if lo == 0 else half
            b = len(seg) if hi == n else len(seg) - half
            got = y[r, lo + a:lo + b].cpu().numpy().astype(np.float64)
            scale = np.abs(seg).max() * np.abs(h64).sum()
            d = np.abs(got - want[a:b]).max() / scale
            worst = max(worst, float(d))
            ok = ok and bool(d <= SG_RTOL)
    return {"ok": bool(ok), "max_err_of_scale": worst,
            "what": f"windows of rows {list(rows)} vs the f64 convolution with reflect padding, max error <= {SG_RTOL} "
                    "of max|x| * sum|h|"}


def report(name, workload, samples, byts, t, ceil_ms, check, **extra):
    med, mn, b2b = t
    job = {"job": name, "workload": workload, "samples": samples, "bytes_moved": byts, "ms": round(med, 4),
           "ms_min": round(mn, 4), "ms_back_to_back": round(b2b, 4), "samples_per_s": round(samples / med * 1e3, 1),
           "frac_of_copy_ceiling": round(ceil_ms / med, 4), "check": check}
    job.update(extra)
    return job


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--json", default=None)
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("filterbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    nch, n = o.channels, o.seconds * 16000
    total = nch * n
    x = torch.rand(nch, n, device="cuda") - 0.5
    y = torch.empty_like(x)
    ceil = copy_ceiling(x, y, o.reps, o.burst)
    casc = fu.make_cascades()
    rows = sorted({0, nch // 2, nch - 1})
    jobs = []
    long_load = f"{nch} ch x {o.seconds} s at 16 kHz"

    def iir_job(name, sos_np, xs, ys, workload, whole, check_rows, ceil_ms):
        sos = torch.from_numpy(sos_np).cuda()
        vv.debug_clear("STAT_IIR_EXACT")
        vv.debug_clear("STAT_IIR_CHUNKED")
        t = timed(lambda: vv.iir(xs, sos, out=ys), o.reps, o.burst)   # zero state in, none written
        chunked = vv.debug_get("STAT_IIR_CHUNKED") > 0
        passes = 3 if chunked else 2      # x read twice and y written once on the chunked route
        return report(name, workload, xs.numel(), 4 * passes * xs.numel(), t, ceil_ms,
                      check_iir(xs, ys, sos_np, check_rows, whole), route="chunked" if chunked else "exact",
                      stages=len(sos_np))

    jobs.append(iir_job("iir4_default", casc["a"], x, y, long_load + ", 4 stages", False, rows, ceil["ms"]))
    xs = x.view(-1)[:1024 * 4800].view(1024, 4800)
    ys = y.view(-1)[:1024 * 4800].view(1024, 4800)
    short_ceil = ceil["ms"] * xs.numel() / total
    jobs.append(iir_job("iir4_short", casc["a"], xs, ys, "1024 rows x 4800 samples, 4 stages", True, [0, 511, 1023],
                        short_ceil))
    jobs[-1]["ceiling_note"] = "the long rows' copy time scaled to this job's samples"
    jobs.append(iir_job("iir1_default", casc["c"], x, y, long_load + ", 1 stage", False, rows, ceil["ms"]))
    for m, p in ((11, 3), (257, 5)):
        h = vv.savgol_coeffs(m, p).numpy()
        t = timed(lambda: vv.savgol(x, m, p, out=y), o.reps, o.burst)
        jobs.append(report(f"savgol_{m}", long_load + f", window {m} order {p} reflect", total, 8 * total, t, ceil["ms"],
                           check_savgol(x, y, h, rows), f64_fma=total * m))
    sweep = []
    if o.sweep:
        sos = torch.from_numpy(casc["a"]).cuda()
        for chunk in (256, 512, 1024, 2048, 4096, 8192):
            with vv.knobs(IIR_CHUNK=chunk):
                t = timed(lambda: vv.iir(x, sos, out=y), o.reps, o.burst)
            sweep.append({"job": "iir4", "rows": nch, "n": n, "IIR_CHUNK": chunk, "ms": round(t[0], 4),
                          "ms_min": round(t[1], 4)})
        # where the exact route stops paying: 1024 rows at the candidate row lengths, exact against chunked
        for n0 in (4096, 8192, 16384):
            xa = x.view(-1)[:1024 * n0].view(1024, n0)
            ya = y.view(-1)[:1024 * n0].view(1024, n0)
            for chunk in (0, 1024):
                with vv.knobs(IIR_CHUNK=chunk):
                    t = timed(lambda: vv.iir(xa, sos, out=ya), o.reps, o.burst)
                sweep.append({"job": "iir4", "rows": 1024, "n": n0, "IIR_CHUNK": chunk, "ms": round(t[0], 4),
                              "ms_min": round(t[1], 4)})
        for n0 in (4096, 8192, 16384):
            xa = x.view(-1)[:32 * n0].view(32, n0)
            ya = y.view(-1)[:32 * n0].view(32, n0)
            for chunk in (0, 1024):
                with vv.knobs(IIR_CHUNK=chunk):
                    t = timed(lambda: vv.iir(xa, sos, out=ya), o.reps, o.burst)
                sweep.append({"job": "iir4", "rows": 32, "n": n0, "IIR_CHUNK": chunk, "ms": round(t[0], 4),
                              "ms_min": round(t[1], 4)})
    line = {"bench": "filter", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "copy_ceiling": ceil, "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    if sweep:
        line["chunk_sweep"] = sweep
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
