#!/usr/bin/env python3
"""Per-frame statistics on one MI355X: 32 channels x 10 minutes at 16 kHz,
frame 400 / hop 160 / Hamming.

Jobs:
  fused_energy   rms, min, max, crest, zero crossings, argmin, argmax: signal ->
                 planes in one kernel (vv_dsp_stats_frames_device);
  fused_full     all twelve outputs (adds sum, mean, var, skewness, kurtosis: the
                 f64 sum and the second pass about the mean);
  pipeline_full  the same through vv_dsp_fetch_frames_device (one launch per
                 channel, frame rows in HBM) -> vv_dsp_stats_device;
  torch_energy / torch_full   the equivalent torch expression on the same tensors
                 (unfold -> times window -> float32 reductions), in the same run;
  autocorr_64    vv_dsp_autocorrelation_device, 64 lags of 1024 x 4800 rows.

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.
Per job: ms, frames/s and the fraction of the in-run streaming-copy ceiling --
the time a streaming copy kernel (scripts/membench.hip k_rw) takes to move the
job's input samples in this same process.  A few frames of every job are
checked in the run against the f64 model of tests/stats_util.py: the library's
jobs bit for bit on min / max / arg* / crossings and at <= 1 float32 ulp
elsewhere, the torch expression (float32 sums) at rtol 1e-3.  Prints one JSON
line.

    python scripts/statsbench.py [--reps 20] [--seconds 600] [--channels 32] [--json FILE]
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
import stats_util as su  # noqa: E402


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


def copy_ceiling(x, reps, burst):
    path = os.path.join(ROOT, "scripts", "libmembench.so")
    if not os.path.exists(path):
        raise SystemExit("scripts/libmembench.so missing: run `make -C vv-dsp_amd membench`")
    mb = C.CDLL(path)
    mb.membench_rw.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    y = torch.empty_like(x)
    s = torch.cuda.current_stream().cuda_stream
    best = None
    for blocks in (2048, 4096, 8192):
        def fn(blocks=blocks):
            assert mb.membench_rw(x.data_ptr(), y.data_ptr(), x.numel() // 4, 1, blocks, s) == 0
        t = timed(fn, reps, burst)
        if best is None or t[0] < best[1][0]:
            best = (blocks, t)
    assert torch.equal(x.view(-1)[:x.numel() // 4 * 4], y.view(-1)[:x.numel() // 4 * 4])
    return {"what": "streaming copy of the signal (membench k_rw, float4 per lane, best of 3 grid sizes)",
            "samples": x.numel(), "blocks": best[0], "ms": round(best[1][0], 4), "ms_min": round(best[1][1], 4),
            "ms_back_to_back": round(best[1][2], 4)}


def sample_frames(nch, frames):
    return sorted({(0, 0), (0, frames // 2), (nch // 2, frames // 3), (nch - 1, frames - 1)})


def check_planes(x, planes, frame, hop, win, names, exact):
    """sampled frames against the f64 model of the same float32 frames.  exact: the
    library's contract (bits / 1 ulp); else rtol 1e-3, atol 1e-5 and counts exact"""
    w = win.cpu().numpy()
    worst, ok = 0, True
    nch, frames = next(iter(planes.values())).shape
    for c, f in sample_frames(nch, frames):
        fr = x[c, f * hop:f * hop + frame].cpu().numpy() * w
        m = su.model(fr)
        for k in names:
            got = planes[k][c, f].cpu().numpy()
            if k in su.COUNT_NAMES:
                ok = ok and int(got) == m[k]
            elif exact:
                u = int(su.f32_ulps(np.float32(got), np.float32(m[k])))
                worst = max(worst, u)
                ok = ok and u <= (0 if k in su.EXACT_NAMES else 1)
            else:
                ok = ok and bool(abs(float(got) - float(m[k])) <= 1e-5 + 1e-3 * abs(float(m[k])))
    what = ("4 frames vs the f64 model: exact class bit for bit, the others <= 1 ulp" if exact else
            "4 frames vs the f64 model: counts and indices equal, values at rtol 1e-3 + 1e-5")
    return {"ok": bool(ok), "max_ulps": worst, "what": what}


def torch_stats(x, frame, hop, win, names):
    """the torch expression a user would write: unfold -> window -> float32 reductions"""
    fr = x.unfold(1, frame, hop) * win
    out = {}
    if "sum" in names:
        out["sum"] = fr.sum(-1)
        out["mean"] = out["sum"] / frame
        d = fr - out["mean"].unsqueeze(-1)
        d2 = d * d
        var = d2.mean(-1)
        out["var"] = var
        out["skewness"] = (d2 * d).mean(-1) / var.pow(1.5)
        out["kurtosis"] = (d2 * d2).mean(-1) / (var * var) - 3.0
    out["rms"] = fr.square().mean(-1).sqrt()
    out["min"], out["argmin"] = fr.min(-1)
    out["max"], out["argmax"] = fr.max(-1)
    out["crest"] = torch.maximum(out["max"], -out["min"]) / out["rms"]
    a, b = fr[..., :-1], fr[..., 1:]
    out["zero_crossings"] = (((a > 0) & (b < 0)) | ((a < 0) & (b > 0))).sum(-1)
    return out


def report(name, workload, items, samples, t, ceil, check, **extra):
    med, mn, b2b = t
    ceil_ms = ceil["ms"] * samples / ceil["samples"]
    job = {"job": name, "workload": workload, "items": items, "input_bytes": 4 * samples, "ms": round(med, 4),
           "ms_min": round(mn, 4), "ms_back_to_back": round(b2b, 4), "items_per_s": round(items / med * 1e3, 1),
           "frac_of_copy_ceiling": round(ceil_ms / med, 4), "check": check}
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
        raise SystemExit("statsbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    L = vv.lib()
    L.vv_dsp_fetch_frames_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                             C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    nch, rate, frame, hop = o.channels, 16000, 400, 160
    n = o.seconds * rate
    torch.manual_seed(0)
    x = torch.rand(nch, n, device="cuda") * 2 - 1
    win = torch.from_numpy((0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(frame) / (frame - 1))).astype(np.float32)).cuda()
    fr = vv.num_frames(n, frame, hop)
    workload = f"{nch} ch x {o.seconds} s at {rate} Hz, frame {frame} hop {hop} Hamming"
    ceil = copy_ceiling(x, o.reps, o.burst)
    jobs = []
    res = {}

    def fused(names):
        res["p"] = vv.stats_frames(x, frame, hop, names, window=win)

    for name, names in (("fused_energy", su.ENERGY_NAMES), ("fused_full", su.STAT_NAMES)):
        vv.debug_clear("STAT_STATS_WAVE")
        t = timed(lambda: fused(names), o.reps, o.burst)
        jobs.append(report(name, workload + f", {len(names)} outputs", nch * fr, nch * n, t, ceil,
                           check_planes(x, res["p"], frame, hop, win, names, True),
                           wave_kernel_launches=vv.debug_get("STAT_STATS_WAVE")))
    full = res["p"]
    t_full = jobs[-1]["ms"]

    rows = torch.empty(nch * fr, frame, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def pipeline():
        for c in range(nch):
            st = L.vv_dsp_fetch_frames_device(x[c].data_ptr(), n, rows[c * fr].data_ptr(), frame, hop, 0, fr, 0,
                                              win.data_ptr(), s)
            assert st == 0
        res["q"] = vv.stats(rows, su.STAT_NAMES)

    t = timed(pipeline, o.reps, o.burst)
    same = all(torch.equal(full[k].reshape(-1).view(torch.int32), res["q"][k].view(torch.int32)) for k in su.STAT_NAMES)
    jobs.append(report("pipeline_full", workload + f" ({nch} fetch_frames launches + stats)", nch * fr, nch * n, t, ceil,
                       {"ok": bool(same), "what": "every plane bit-identical to fused_full"},
                       frame_rows_bytes=8 * nch * fr * frame, fused_speedup=round(t[0] / t_full, 3)))
    del rows
    res.pop("q")
    torch.cuda.empty_cache()

    treps = max(3, o.reps // 4)
    for name, names, fused_ms in (("torch_energy", su.ENERGY_NAMES, jobs[0]["ms"]), ("torch_full", su.STAT_NAMES, t_full)):
        def run(names=names):
            res["t"] = torch_stats(x, frame, hop, win, names)
        t = timed(run, treps, treps)
        jobs.append(report(name, workload + ", torch unfold -> float32 reductions", nch * fr, nch * n, t, ceil,
                           check_planes(x, res["t"], frame, hop, win, names, False),
                           fused_speedup=round(t[0] / fused_ms, 3)))
        res.pop("t")
        torch.cuda.empty_cache()

    # 64 lags of 1024 rows of 4800 samples
    b, m, lags = 1024, 4800, 64
    xr = x.reshape(-1)[:b * m].reshape(b, m)
    t = timed(lambda: res.__setitem__("r", vv.autocorrelation(xr, lags)), o.reps, o.burst)
    worst = 0
    for i in (0, b // 2, b - 1):
        u = su.f32_ulps(res["r"][i].cpu().numpy(), su.autocorr_model(xr[i].cpu().numpy(), lags, False))
        worst = max(worst, int(u.max()))
    jobs.append(report("autocorr_64", f"{b} rows x {m} samples, {lags} lags, unbiased", b * lags, b * m, t, ceil,
                       {"ok": worst <= 1, "max_ulps": worst, "what": "3 rows vs the f64 model, <= 1 ulp"},
                       f64_fma=b * sum(m - k for k in range(lags))))

    line = {"bench": "stats", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "copy_ceiling": ceil, "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
