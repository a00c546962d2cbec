#!/usr/bin/env python3
"""The resampler on one MI355X: 32 channels x 10 minutes of audio, sinc at 32
taps and linear, for 44.1 -> 16 kHz (160/441), 48 -> 16 kHz (1/3) and
16 -> 48 kHz (3/1).

Each job is one vv_dsp_resampler_process_device launch on device-resident
rows, timed with HIP events on the launch stream (median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst).
Bytes are the algorithm's 4 (in + out) per channel; the fraction of the 8 TB/s
HBM peak is bytes over the median.  The same byte mix moved by a streaming
kernel with no arithmetic (scripts/membench.hip k_rwmix, best of a few grid
sizes, timed the same way) is the box's own ceiling for the job.  Sampled
windows of two output rows are checked in the run against the f64 model
(tests/resample_util.py: f64 table, f64 sum) with the harness tolerance;
linear rows must equal the model bit for bit.  Prints one JSON line.

    python scripts/resamplebench.py [--reps 20] [--seconds 600] [--channels 32] [--json FILE]
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
import resample_util as ru  # noqa: E402

PEAK = 8000.0   # GB/s
JOBS = (("44.1k_to_16k", 160, 441, 44100), ("48k_to_16k", 1, 3, 48000), ("16k_to_48k", 3, 1, 16000))


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


def ceiling(n_in, n_out, reps, burst):
    """ms of the same bytes through membench k_rwmix (None without scripts/libmembench.so)"""
    path = os.path.join(ROOT, "scripts", "libmembench.so")
    if not os.path.exists(path):
        return None
    mb = C.CDLL(path)
    if not hasattr(mb, "membench_rwmix"):
        return None
    mb.membench_rwmix.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
    a = torch.rand(n_in, device="cuda")
    b = torch.empty(n_out, device="cuda")
    s = torch.cuda.current_stream()
    best = None
    for blocks in (2048, 4096, 16384):
        fn = (lambda blocks=blocks: mb.membench_rwmix(a.data_ptr(), b.data_ptr(), n_in // 4, n_out // 4, blocks,
                                                      s.cuda_stream))
        assert fn() == 0
        med, mn, b2b = timed(fn, reps, burst)
        if best is None or med < best["ms"]:
            best = {"ms": round(med, 4), "ms_min": round(mn, 4), "ms_back_to_back": round(b2b, 4), "blocks": blocks}
    del a, b
    return best


def model_sinc_f64(x, num, den, taps, ks):
    _, W = ru.model_table(num, den, taps)
    centre, row = ru.model_centres(num, den, ks)
    T = W.shape[1]
    acc = np.zeros(len(ks))
    for m in range(T):
        acc += x[np.clip(centre + (m - T // 2), 0, len(x) - 1)].astype(np.float64) * W[row, m]
    low = np.flatnonzero(row == W.shape[0] - 1)
    if len(low):
        acc[low] = ru.model_exact(x, num, den, T, ks[low])
    return acc


def check(x_dev, y_dev, num, den, sinc):
    """sampled windows of the first and last rows against the model"""
    out_n = y_dev.shape[1]
    worst, ok = 0.0, True
    for c in sorted({0, x_dev.shape[0] - 1}):
        x = x_dev[c].cpu().numpy()
        y = y_dev[c].cpu().numpy()
        if not sinc:
            same = y.tobytes() == ru.model_linear(x, num, den).tobytes()
            ok = ok and same
            continue
        for k0 in (0, out_n // 2 - 1024, out_n - 2048):
            ks = np.arange(max(k0, 0), min(max(k0, 0) + 2048, out_n), dtype=np.int64)
            want = model_sinc_f64(x, num, den, 32, ks)
            d = np.abs(y[ks].astype(np.float64) - want)
            worst = max(worst, float(d.max()))
            ok = ok and bool(np.all(d <= 5e-5 + 5e-5 * np.abs(want)))
    return {"ok": bool(ok), "max_abs_diff": worst if sinc else 0.0,
            "what": "2 rows x 3 windows of 2048 outputs vs the f64 model, rtol = atol = 5e-5" if sinc
            else "2 whole rows bit-identical to the model"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("resamplebench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    jobs = []
    for name, num, den, rate in JOBS:
        n = a.seconds * rate
        x = torch.rand(a.channels, n, device="cuda") * 2 - 1
        ceil = None
        for sinc in (True, False):
            rs = vv.Resampler(num, den, sinc=sinc, taps=32)
            m = rs.output_length(n)
            y = torch.empty(a.channels, m, device="cuda")
            vv.debug_clear("STAT_RESAMPLE_TABLE")
            med, mn, b2b = timed(lambda: rs(x, out=y), a.reps, a.burst)
            byts = 4 * a.channels * (n + m)
            if ceil is None:
                ceil = ceiling(a.channels * n, a.channels * m, a.reps, a.burst)
            job = {"job": name, "mode": "sinc32" if sinc else "linear", "ratio": f"{num}/{den}",
                   "workload": f"{a.channels} ch x {a.seconds} s at {rate} Hz", "in_samples": a.channels * n,
                   "out_samples": a.channels * m, "bytes": byts, "ms": round(med, 4), "ms_min": round(mn, 4),
                   "ms_back_to_back": round(b2b, 4), "GBs": round(byts / med / 1e6, 1),
                   "frac_of_8TBs": round(byts / med / 1e6 / PEAK, 4), "copy_ceiling": ceil,
                   "frac_of_copy_ceiling": round(ceil["ms"] / med, 4) if ceil else None,
                   "check": check(x, y, num, den, sinc)}
            if sinc:
                job["table_kernel_launches"] = vv.debug_get("STAT_RESAMPLE_TABLE")
                job["run_length"] = vv.lib().vvhip_resample_run_length(num, den, 32)
            jobs.append(job)
            del y, rs
        del x
        torch.cuda.empty_cache()
    line = {"bench": "resample", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": a.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
