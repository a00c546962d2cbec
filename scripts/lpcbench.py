#!/usr/bin/env python3
"""Batched LPC on one MI355X: 32 channels x 10 minutes of audio.

Jobs:
  fused_16k    16 kHz, frame 400 / hop 160 / Hamming / order 16: signal -> a, err
               in one kernel (vv_dsp_lpc_frames_device);
  pipeline_16k the same through vv_dsp_fetch_frames_device (one launch per
               channel, frame rows in HBM) -> vv_dsp_lpc_device, in the same run;
  fused_48k    48 kHz, 1200 / 480 / order 32;
  lpspec_16k   order 16 -> 512 bins over fused_16k's coefficient rows
               (levinson_sign, so the rows feed it directly).

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.
Per job: ms, frames/s, the fraction of the 8 TB/s HBM peak by algorithmic
bytes (signal or coefficient rows read once, outputs written once; the
pipeline's frame rows are not algorithmic bytes) and the fraction of the f32
FMA peak (78.65 T FMA/s) by frame_len x (order + 1) FMAs per frame (lpspec: 2 x
order x nfft per row).  A few rows of every job are checked in the run
against an f64 model (f64 autocorrelation and recursion of the same windowed
frames; the spectrum with the exact residue (m k) mod nfft).  Prints one
JSON line.

    python scripts/lpcbench.py [--reps 20] [--seconds 600] [--channels 32] [--json FILE]
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
import lpc_util as lu  # noqa: E402

PEAK_GBS = 8000.0
PEAK_FMA = 78.65e12   # 157.3 TFLOPS f32 vector


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


def levinson_f64(r):
    order = len(r) - 1
    a = np.zeros(order + 1)
    a[0] = 1.0
    e = r[0]
    for m in range(1, order + 1):
        k = -(r[m] + np.dot(a[1:m], r[m - 1:0:-1])) / e
        a[1:m] = a[1:m] + k * a[m - 1:0:-1]
        a[m] = k
        e *= 1.0 - k * k
    return a, e


def sample_rows(nch, frames):
    return sorted({(0, 0), (0, frames // 2), (nch // 2, frames // 3), (nch - 1, frames - 1)})


def check_lpc(x, a, err, frame, hop, order, win):
    """sampled frames against f64 autocorrelation + recursion of the same f32 frames"""
    worst, ok = 0.0, True
    w = win.cpu().numpy()
    for c, f in sample_rows(a.shape[0], a.shape[1]):
        fr = x[c, f * hop:f * hop + frame].cpu().numpy() * w
        want, e = levinson_f64(lu.autocorr_f64(fr, order))
        d = np.abs(a[c, f].cpu().numpy().astype(np.float64) - want)
        worst = max(worst, float(d.max()))
        ok = ok and bool(np.all(d <= 5e-5 + 5e-5 * np.abs(want))) and abs(float(err[c, f]) - e) <= 5e-5 * e + 5e-5
    return {"ok": bool(ok), "max_abs_diff": worst,
            "what": "a and err of 4 frames vs f64 autocorrelation + Levinson, rtol = atol = 5e-5"}


def report(name, workload, frames, byts, fmas, t, check, **extra):
    med, mn, b2b = t
    job = {"job": name, "workload": workload, "frames": frames, "bytes": byts, "fma": fmas, "ms": round(med, 4),
           "ms_min": round(mn, 4), "ms_back_to_back": round(b2b, 4), "frames_per_s": round(frames / med * 1e3, 1),
           "frac_of_8TBs": round(byts / med / 1e6 / PEAK_GBS, 4),
           "frac_of_fma_peak": round(fmas / med * 1e3 / PEAK_FMA, 4), "check": check}
    job.update(extra)
    return job


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=None)
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("lpcbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    L = vv.lib()
    L.vv_dsp_fetch_frames_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                             C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    nch = o.channels
    jobs = []
    a16 = None
    for name, rate, frame, hop, order in (("16k", 16000, 400, 160, 16), ("48k", 48000, 1200, 480, 32)):
        n = o.seconds * rate
        x = torch.rand(nch, n, device="cuda") * 2 - 1
        win = torch.from_numpy(lu.hamming(frame)).cuda()
        fr = vv.num_frames(n, frame, hop)
        a = torch.empty(nch, fr, order + 1, device="cuda")
        err = torch.empty(nch, fr, device="cuda")
        workload = f"{nch} ch x {o.seconds} s at {rate} Hz, frame {frame} hop {hop} Hamming order {order}"
        byts = 4 * nch * n + 4 * nch * fr * (order + 2)
        fmas = nch * fr * frame * (order + 1)
        vv.debug_clear("STAT_LPC_WAVE")
        t = timed(lambda: vv.lpc_frames(x, frame, hop, order, window=win, out=(a, err)), o.reps, o.burst)
        jobs.append(report("fused_" + name, workload, nch * fr, byts, fmas, t,
                           check_lpc(x, a, err, frame, hop, order, win),
                           wave_kernel_launches=vv.debug_get("STAT_LPC_WAVE")))
        if name == "16k":
            rows = torch.empty(nch * fr, frame, device="cuda")
            a2 = torch.empty(nch * fr, order + 1, device="cuda")
            err2 = torch.empty(nch * fr, device="cuda")
            s = torch.cuda.current_stream().cuda_stream

            def pipeline():
                for c in range(nch):
                    st = L.vv_dsp_fetch_frames_device(x[c].data_ptr(), n, rows[c * fr].data_ptr(), frame, hop, 0, fr, 0,
                                                      win.data_ptr(), s)
                    assert st == 0
                st = L.vv_dsp_lpc_device(rows.data_ptr(), frame, order, nch * fr, a2.data_ptr(), err2.data_ptr(), s)
                assert st == 0

            t2 = timed(pipeline, o.reps, o.burst)
            same = bool(torch.equal(a.view(torch.int32).reshape(-1), a2.view(torch.int32).reshape(-1)) and
                        torch.equal(err.view(torch.int32).reshape(-1), err2.view(torch.int32)))
            jobs.append(report("pipeline_" + name, workload + f" ({nch} fetch_frames launches + lpc)", nch * fr, byts,
                               fmas, t2, {"ok": same, "what": "a and err bit-identical to fused_16k"},
                               frame_rows_bytes=8 * nch * fr * frame, fused_speedup=round(t2[0] / t[0], 3)))
            del rows, a2, err2
            a16 = a.reshape(nch * fr, order + 1)
            nfft = 512
            mag = torch.empty(nch * fr, nfft, device="cuda")

            def spec():
                st = L.vv_dsp_lpspec_device(a16.data_ptr(), order, None, nfft, nch * fr, 1, mag.data_ptr(), s)
                assert st == 0

            t3 = timed(spec, o.reps, o.burst)
            worst, ok = 0.0, True
            for c, f in sample_rows(nch, fr):
                i = c * fr + f
                want = lu.lpspec_f64(a16[i].cpu().numpy(), 1.0, nfft, True)
                d = np.abs(mag[i].cpu().numpy().astype(np.float64) - want) / want
                worst = max(worst, float(d.max()))
                ok = ok and bool(d.max() <= 1e-5)
            jobs.append(report("lpspec_" + name, f"{nch * fr} rows of order {order} -> {nfft} bins", nch * fr,
                               4 * nch * fr * (order + 1 + nfft), nch * fr * 2 * order * nfft, t3,
                               {"ok": ok, "max_rel_diff": worst,
                                "what": "4 rows vs the f64 model with exact residues, relative 1e-5"}))
            del mag, a16
        del x, a, err
        torch.cuda.empty_cache()
    line = {"bench": "lpc", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "peaks": {"GBs": PEAK_GBS, "fma_per_s": PEAK_FMA},
            "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
