#!/usr/bin/env python3
"""Per-frame spectral shape descriptors on one MI355X: 32 channels x 10 minutes at
16 kHz, n_fft 1024 / hop 256 (the features leg's shape), magnitude weights,
roll-off 0.85.

  rows_<layout>_<mask>   vv_dsp_spectral_shape_device on resident power rows, layout
              pitched (544 floats per row) or packed (513), mask all (ten outputs),
              centroid_rolloff or flux; beside each layout a streaming read of the
              same bytes with the job's output bytes written (membench k_rwmix): the
              ceiling, and every job's fraction of it;
  signal_planes          signal -> planes (vv_dsp_stft_spectral_shape_device, all ten);
  signal_power_rows      signal -> pitched power rows alone;
  signal_log_mel         Stft -> log-mel in one kernel (80 mels), for scale;
  torch                  the same definitions as a float32 torch expression on the
              packed rows;
  per_output_ms          the rows kernel on the pitched rows per class of outputs
              (energy; the first-pass outputs; the moments; flatness; roll-off;
              flux; all ten), with magnitude and with power weights.

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.  A
seeded sample of rows of every job is checked in the run against the f64 model of
tests/shape_util.py: the library's jobs by its comparison rule (peak bin and
roll-off equal on decidable rows, the rest <= 1 float32 ulp), the torch
expression at 1e-3 relative (float32 sums) with equal peak bins.  Prints one JSON
line.

    python scripts/shapebench.py [--reps 10] [--seconds 600] [--channels 32] [--json FILE]
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
import shape_util as su  # noqa: E402

NFFT, HOP, K, PITCH = 1024, 256, 513, 544
SAMPLE = 24
MASKS = {"all": su.NAMES, "centroid_rolloff": ("centroid", "rolloff"), "flux": ("flux",)}
# the masks of "per_output_ms": what each class of outputs costs on the pitched rows
PER_OUTPUT = [("energy",), ("energy", "centroid", "crest", "peak_bin"), ("spread",), ("spread", "skewness", "kurtosis"),
              ("flatness",), ("rolloff",), ("flux",), su.NAMES]


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


def read_ceiling(rows, out_bytes, reps, burst):
    path = os.path.join(ROOT, "scripts", "libmembench.so")
    if not os.path.exists(path):
        raise SystemExit("scripts/libmembench.so missing: run `make -C vv-dsp_amd membench`")
    mb = C.CDLL(path)
    mb.membench_rwmix.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
    n_in4, n_out4 = rows.numel() // 4, (out_bytes + 15) // 16
    y = torch.empty(n_out4 * 4, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    best = None
    for blocks in (2048, 4096, 8192):
        def fn(blocks=blocks):
            assert mb.membench_rwmix(rows.data_ptr(), y.data_ptr(), n_in4, n_out4, blocks, s) == 0
        t = timed(fn, reps, burst)
        if best is None or t[0] < best[1][0]:
            best = (blocks, t)
    return {"what": "streaming read of the rows' buffer with the ten planes' bytes written (membench k_rwmix, "
                    "float4 per lane, best of 3 grid sizes)", "bytes_read": n_in4 * 16, "bytes_written": n_out4 * 16,
            "blocks": best[0], "ms": round(best[1][0], 4), "ms_min": round(best[1][1], 4),
            "ms_back_to_back": round(best[1][2], 4), "GBps": round(n_in4 * 16 / best[1][0] / 1e6, 1)}


def sample_rows(nch, frames, seed):
    rng = np.random.default_rng(seed)
    pick = {(0, 0), (0, 1), (nch - 1, frames - 1)}
    while len(pick) < SAMPLE:
        pick.add((int(rng.integers(nch)), int(rng.integers(frames))))
    return sorted(pick)


def model_of(power, pick, prm):
    """the model on the sampled rows of power [ch][fr][>= K], each with its predecessor"""
    res = []
    for c, f in pick:
        row = power[c, f, :K].cpu().numpy()
        prev = power[c, f - 1, :K].cpu().numpy() if f else None
        res.append(su.model_row(row, prev, prm))
    return {n: np.array([r[n] for r in res]) for n in res[0]}


def check_library(planes, m, pick, names):
    got = {n: np.array([planes[n][c, f].item() for c, f in pick]) for n in names}
    worst, ok = 0, True
    for n in names:
        if n == "peak_bin":
            dec = ~m["peak_undecidable"]
            ok &= bool(np.array_equal(got[n][dec].astype(np.int64), m[n][dec]))
        elif n == "rolloff":
            dec = ~m["rolloff_undecidable"]
            ok &= bool(np.array_equal(got[n][dec].astype(np.float32), m[n][dec]))
        else:
            u = su.f32_ulps(got[n].astype(np.float32), m[n])
            if n == "skewness":
                u = np.where(np.abs(got[n] - m[n].astype(np.float64)) <= 1e-9, 0, u)
            worst = max(worst, int(u.max()))
    return {"ok": bool(ok and worst <= 1), "max_ulps": worst, "rows": len(pick),
            "undecidable": int(np.sum(m["rolloff_undecidable"]) + np.sum(m["peak_undecidable"])),
            "what": "seeded rows vs the f64 model: peak bin and roll-off equal on decidable rows, the rest <= 1 ulp"}


def torch_shape(P, fs, rolloff, floor):
    """the definitions as a user would write them in torch, float32, one pass per descriptor"""
    w = P[..., :K].sqrt()
    k = torch.arange(K, device=P.device, dtype=torch.float32)
    S0 = w.sum(-1)
    c = (w * k).sum(-1) / S0
    d = k - c[..., None]
    var = (d * d * w).sum(-1) / S0
    sd = var.sqrt()
    wf = w.clamp_min(floor)
    flux = torch.zeros_like(S0)
    flux[:, 1:] = (w[:, 1:] - w[:, :-1]).pow(2).sum(-1).sqrt()
    mx, peak = w.max(-1)
    roll = (torch.cumsum(w, -1) >= rolloff * S0[..., None]).to(torch.int8).argmax(-1)
    return {"energy": S0, "centroid": c * (fs / NFFT), "spread": sd * (fs / NFFT),
            "skewness": (d ** 3 * w).sum(-1) / S0 / sd ** 3, "kurtosis": (d ** 4 * w).sum(-1) / S0 / var ** 2,
            "flatness": wf.log().mean(-1).exp() / wf.mean(-1), "rolloff": roll.to(torch.float32) * (fs / NFFT),
            "flux": flux, "crest": mx / (S0 / K), "peak_bin": peak}


def check_torch(res, m, pick):
    worst = 0.0
    for n in ("energy", "centroid", "spread", "kurtosis", "flatness", "flux", "crest"):
        got = np.array([res[n][c, f].item() for c, f in pick], np.float64)
        want = m[n].astype(np.float64)
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30))))
    peaks = np.array([res["peak_bin"][c, f].item() for c, f in pick])
    return {"ok": bool(worst <= 1e-3 and np.array_equal(peaks, m["peak_bin"])), "max_rel_err": float(f"{worst:.3g}"),
            "rows": len(pick), "what": "seeded rows vs the f64 model: the float sums at 1e-3 relative, peak bins equal"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "shape_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("shapebench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    nch, rate = o.channels, 16000
    n = o.seconds * rate
    x = signal(nch, n, rate, 20261020)
    st = vv.Stft(NFFT, HOP)
    fr = st.frames(n)
    q = su.params(NFFT, magnitude=1, rolloff=0.85)
    p = vv.SpectralShapeParams(q.n_fft, q.sample_rate, q.magnitude, q.k_min, q.k_max, q.rolloff, q.floor)
    workload = f"{nch} ch x {o.seconds} s at {rate} Hz, n_fft {NFFT} hop {HOP}: {nch * fr} rows of {K} bins"
    pick = sample_rows(nch, fr, 7)
    jobs, ceilings, res = [], {}, {}

    def report(name, what, t, check, **extra):
        med, mn, b2b = t
        job = {"job": name, "workload": workload + what, "rows": nch * fr, "ms": round(med, 4), "ms_min": round(mn, 4),
               "ms_back_to_back": round(b2b, 4), "rows_per_s": round(nch * fr / med * 1e3, 1), "check": check}
        job.update(extra)
        jobs.append(job)
        return job

    layouts = {"pitched": st.power(x, pitch=PITCH)}
    layouts["packed"] = layouts["pitched"][..., :K].contiguous()
    m = model_of(layouts["packed"], pick, q)
    ref = None
    for layout, power in layouts.items():
        pitch = power.shape[-1]
        ceil = ceilings[layout] = read_ceiling(power, 40 * nch * fr, o.reps, o.burst)
        for mask, names in MASKS.items():
            def rows_job(names=names, power=power):
                res["r"] = vv.spectral_shape(power, p, names)
            vv.debug_clear("STAT_SHAPE_WAVE")
            t = timed(rows_job, o.reps, o.burst)
            launches = vv.debug_get("STAT_SHAPE_WAVE") / (2 + o.reps + o.burst)
            check = check_library(res["r"], m, pick, names)
            if ref is None:
                ref = res["r"]
            same = all(torch.equal(ref[k].view(torch.int32), res["r"][k].view(torch.int32)) for k in names)
            check["ok"] = bool(check["ok"] and same)
            check["what"] += "; every plane bit-identical to rows_pitched_all"
            report(f"rows_{layout}_{mask}", f", resident rows {pitch} floats apart, outputs: {', '.join(names)}", t,
                   check, bytes_read=power.numel() * 4, GBps=round(power.numel() * 4 / t[0] / 1e6, 1),
                   frac_of_read_ceiling=round(ceil["ms"] / t[0], 4), kernel_launches_per_call=launches)
    res.pop("r")
    per_output = {}
    for magnitude in (1, 0):
        pm = vv.SpectralShapeParams(q.n_fft, q.sample_rate, magnitude, q.k_min, q.k_max, q.rolloff, q.floor)
        for names in PER_OUTPUT:
            t = timed(lambda: vv.spectral_shape(layouts["pitched"], pm, names), o.reps, o.burst)
            per_output[("magnitude: " if magnitude else "power: ") + " + ".join(names)] = round(t[0], 4)

    def planes_job():
        res["s"] = st.spectral_shape(x, p, su.NAMES)
    tp = timed(planes_job, o.reps, o.burst)
    same = all(torch.equal(ref[k].view(torch.int32), res["s"][k].view(torch.int32)) for k in su.NAMES)
    report("signal_planes", ", signal -> power rows in scratch -> ten planes", tp,
           {"ok": bool(same), "what": "every plane bit-identical to rows_pitched_all"},
           scratch_bytes=4 * nch * fr * PITCH)
    res.pop("s")
    buf = layouts["pitched"]

    def power_job():
        st.power(x, out=buf, pitch=PITCH)
    tw = timed(power_job, o.reps, o.burst)
    report("signal_power_rows", ", signal -> pitched power rows alone", tw,
           {"ok": True, "what": "timing only (the rows are the other jobs' input)"}, bytes_written=4 * nch * fr * PITCH)
    mel = vv.Mfcc(NFFT, 80, 13, float(rate), 0.0, rate / 2.0)

    def mel_job():
        res["m"] = mel.from_signal(st, x, log_mel=True)
    tm = timed(mel_job, o.reps, o.burst)
    report("signal_log_mel", ", Stft -> log-mel (80 mels) in one kernel, for scale", tm,
           {"ok": bool(torch.isfinite(res["m"]).all().item()), "what": "finite"})
    res.pop("m")
    del layouts["pitched"], buf
    torch.cuda.empty_cache()

    def torch_job():
        res["t"] = torch_shape(layouts["packed"], float(rate), 0.85, su.FLOOR)
    tt = timed(torch_job, 2, 2)
    all_ms = next(j["ms"] for j in jobs if j["job"] == "rows_packed_all")
    report("torch", ", the ten definitions as a float32 torch expression on the packed rows", tt,
           check_torch(res["t"], m, pick), rows_kernel_speedup=round(tt[0] / all_ms, 2))

    line = {"bench": "spectral_shape", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "read_ceiling": ceilings, "per_output_ms": per_output,
            "per_output_what": "median ms of the rows kernel on the pitched rows per output mask (timing only)",
            "fused_mode_bound_ms": round(tp[0] - tw[0], 4),
            "fused_mode_bound_what": "signal_planes minus signal_power_rows: the re-read of the rows and the shape "
                                     "kernel; a k_stft_pair mode that keeps the rows in LDS saves at most this plus "
                                     "the rows' write inside signal_power_rows",
            "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
