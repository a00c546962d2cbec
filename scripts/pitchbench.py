#!/usr/bin/env python3
"""Per-frame pitch (YIN) on one MI355X: 32 channels x 10 minutes at 16 kHz.

Two shapes: frame 400 / hop 160, 100-400 Hz (tau 40..160, W 240), and frame
1024 / hop 256, 60-500 Hz (tau 32..267, W 757); threshold 0.15, outputs f0,
aperiodicity and lag.  Per shape:
  fused       signal -> planes in one kernel (vv_dsp_pitch_frames_device);
  fused_f32   the same with the frame kept in LDS as f32 (knob PITCH_F32 = 1;
              the default keeps it as f64 at these sizes; same bits);
  pipeline    vv_dsp_fetch_frames_device (one launch per channel, frame rows in
              HBM) -> vv_dsp_pitch_device;
  torch       the same definition as a torch expression on the same tensors:
              unfold, one float32 difference-and-sum per lag, cumsum, the
              threshold search by masks (no descent, no parabola).

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.  Per
job: ms, frames/s, and for the library's kernels the f64 FMA count ((tau_max +
1) W per frame) with the time that count alone would take at the 78.65 T/s f64
vector peak DESIGN.md section 4 uses (one FMA = 2 FLOP; the kernel also issues
one f64 subtract per FMA).  A seeded sample of frames of every job is checked in
the run against the f64 model of tests/pitch_util.py: the library's jobs at
<= 1 float32 ulp with equal lags on decidable frames, the torch expression's
voiced / unvoiced decision and its lag before the descent.  Prints one JSON line.

    python scripts/pitchbench.py [--reps 10] [--seconds 600] [--channels 32] [--json FILE]
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
import pitch_util as pu  # noqa: E402

F64_PEAK_FLOPS = 78.65e12          # f64 vector peak, DESIGN.md section 4
NAMES = ("f0", "aperiodicity", "lag")
SHAPES = [(400, 160, 100.0, 400.0), (1024, 256, 60.0, 500.0)]
THRESHOLD = 0.15
SAMPLE = 24                        # frames checked per job


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
    """voiced stretches (a gliding three-harmonic tone per channel) between noise, float32 on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / rate
    x = torch.empty(nch, n, device="cuda", dtype=torch.float32)
    for c in range(nch):
        f = 110.0 + 9.0 * c + 40.0 * torch.sin(2 * np.pi * 0.21 * t + c)
        ph = 2 * np.pi * torch.cumsum(f, 0) / rate
        tone = torch.sin(ph) + 0.5 * torch.sin(2 * ph + 0.4) + 0.25 * torch.sin(3 * ph + 1.1)
        gate = (torch.sin(2 * np.pi * 0.9 * t + 0.5 * c) > -0.3).to(torch.float64)
        noise = torch.randn(n, device="cuda", generator=g, dtype=torch.float32)
        x[c] = (0.3 * gate * tone).to(torch.float32) + 0.02 * noise
    return x


def sample_frames(nch, frames, seed):
    rng = np.random.default_rng(seed)
    pick = {(0, 0), (nch - 1, frames - 1)}
    while len(pick) < SAMPLE:
        pick.add((int(rng.integers(nch)), int(rng.integers(frames))))
    return sorted(pick)


def model_of(x, pick, frame, hop, fmin, fmax):
    rows = np.stack([x[c, f * hop:f * hop + frame].cpu().numpy() for c, f in pick])
    return pu.model_rows(rows, fmin, fmax, THRESHOLD), rows


def check_library(planes, m, pick):
    got = {k: np.array([planes[k][c, f].item() for c, f in pick]) for k in NAMES}
    ok = m["margin"] >= pu.MARGIN
    lag_ok = bool(np.array_equal(got["lag"][ok].astype(np.int64), m["lag"][ok]))
    worst = 0
    for k in ("f0", "aperiodicity"):
        worst = max(worst, int(pu.f32_ulps(got[k][ok].astype(np.float32), m[k][ok]).max()))
    return {"ok": lag_ok and worst <= 1, "max_ulps": worst, "frames": len(pick), "undecidable": int(np.sum(~ok)),
            "voiced": int(np.sum(m["f0"] > 0)),
            "what": "seeded frames vs the f64 model: lag equal, f0 and aperiodicity <= 1 ulp on decidable frames"}


def torch_yin(x, frame, hop, rate, tau_min, tau_max):
    """the definition as a user would write it in torch: float32, one pass per lag; the lag is
    the first one below the threshold (no descent, no parabola), f0 = rate / lag"""
    fr = x.unfold(1, frame, hop)
    W = frame - tau_max
    head = fr[..., :W]
    d = torch.empty(fr.shape[:2] + (tau_max + 1,), device=x.device, dtype=torch.float32)
    for tau in range(tau_max + 1):
        df = head - fr[..., tau:tau + W]
        d[..., tau] = (df * df).sum(-1)
    c = torch.cumsum(d[..., 1:], -1)
    taus = torch.arange(1, tau_max + 1, device=x.device, dtype=torch.float32)
    q = torch.where(c == 0, torch.ones_like(c), d[..., 1:] * taus / c)          # q[..., k] = d'(k + 1)
    seg = q[..., tau_min - 1:tau_max]
    below = seg < THRESHOLD
    voiced = below.any(-1)
    first = torch.argmax(below.to(torch.int8), -1) + tau_min
    lag = torch.where(voiced, first, torch.argmin(seg, -1) + tau_min)
    f0 = torch.where(voiced, rate / lag.to(torch.float32), torch.zeros_like(lag, dtype=torch.float32))
    return {"f0": f0, "lag": lag}


def check_torch(res, x, pick, frame, hop, fmin, fmax, tau_min, tau_max, rows):
    """voiced / unvoiced and the first lag below the threshold, against the f64 curve, on frames
    whose threshold comparisons have a margin float32 sums cannot cross (1e-3)"""
    q, _ = pu.cmnd_rows(rows, tau_max)
    good = bad = 0
    for i, (c, f) in enumerate(pick):
        seg = q[i, tau_min:tau_max + 1]
        below = np.nonzero(seg < THRESHOLD)[0]
        upto = seg[:below[0] + 1] if len(below) else seg
        if np.min(np.abs(upto - THRESHOLD)) < 1e-3 * THRESHOLD:
            continue
        want_voiced = len(below) > 0
        got_voiced = bool(res["f0"][c, f].item() > 0)
        same = got_voiced == want_voiced and (not want_voiced or int(res["lag"][c, f].item()) == tau_min + below[0])
        good, bad = good + int(same), bad + int(not same)
    return {"ok": bool(bad == 0 and good > 0), "frames": int(good + bad),
            "what": "seeded frames vs the f64 curve: voiced / unvoiced and the first lag below the threshold"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "pitch_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("pitchbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    L = vv.lib()
    L.vv_dsp_fetch_frames_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                             C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    nch, rate = o.channels, 16000
    n = o.seconds * rate
    x = signal(nch, n, rate, 20261020)
    s = torch.cuda.current_stream().cuda_stream
    jobs = []
    for frame, hop, fmin, fmax in SHAPES:
        p = vv.PitchParams(float(rate), fmin, fmax, THRESHOLD)
        tau_min, tau_max, W = vv.pitch_lag_range(p, frame)
        fr = vv.num_frames(n, frame, hop)
        workload = (f"{nch} ch x {o.seconds} s at {rate} Hz, frame {frame} hop {hop}, {fmin:g}-{fmax:g} Hz "
                    f"(tau {tau_min}..{tau_max}, W {W}), f0 + aperiodicity + lag")
        fma = nch * fr * (tau_max + 1) * W
        floor_ms = 2.0 * fma / F64_PEAK_FLOPS * 1e3
        pick = sample_frames(nch, fr, frame)
        m, rows_np = model_of(x, pick, frame, hop, fmin, fmax)
        res = {}

        def report(name, what, t, check, **extra):
            med, mn, b2b = t
            job = {"job": f"{name}_{frame}", "workload": workload + what, "frames": nch * fr, "ms": round(med, 4),
                   "ms_min": round(mn, 4), "ms_back_to_back": round(b2b, 4),
                   "frames_per_s": round(nch * fr / med * 1e3, 1), "check": check}
            job.update(extra)
            jobs.append(job)
            return job

        def fused():
            res["p"] = vv.pitch_frames(x, frame, hop, p, NAMES)

        vv.debug_clear("STAT_PITCH_WAVE")
        t = timed(fused, o.reps, o.burst)
        launches = vv.debug_get("STAT_PITCH_WAVE")
        fused_job = report("fused", "", t, check_library(res["p"], m, pick), f64_fma=fma,
                           ms_of_f64_fma_at_peak=round(floor_ms, 4), frac_of_f64_fma_peak=round(floor_ms / t[0], 4),
                           kernel_launches_per_call=launches / (2 + o.reps + o.burst))
        full = res["p"]
        with vv.knobs(PITCH_F32=1):
            t32 = timed(fused, o.reps, o.burst)
        same = all(torch.equal(full[k].view(torch.int32), res["p"][k].view(torch.int32)) for k in NAMES)
        report("fused_f32", ", frame in LDS as f32", t32, {"ok": bool(same), "what": "every plane bit-identical to fused"},
               vs_fused=round(t32[0] / t[0], 3))

        rows = torch.empty(nch * fr, frame, device="cuda")

        def pipeline():
            for c in range(nch):
                st = L.vv_dsp_fetch_frames_device(x[c].data_ptr(), n, rows[c * fr].data_ptr(), frame, hop, 0, fr, 0,
                                                  None, s)
                assert st == 0
            res["q"] = vv.pitch(rows, p, NAMES)

        tp = timed(pipeline, o.reps, o.burst)
        same = all(torch.equal(full[k].reshape(-1).view(torch.int32), res["q"][k].view(torch.int32)) for k in NAMES)
        report("pipeline", f" ({nch} fetch_frames launches + pitch)", tp,
               {"ok": bool(same), "what": "every plane bit-identical to fused"}, frame_rows_bytes=8 * nch * fr * frame,
               fused_speedup=round(tp[0] / t[0], 3))
        del rows
        res.pop("q")
        torch.cuda.empty_cache()

        def run_torch():
            res["t"] = torch_yin(x, frame, hop, float(rate), tau_min, tau_max)

        tt = timed(run_torch, 2, 2)
        report("torch", ", torch unfold -> float32 sums per lag, first lag below the threshold", tt,
               check_torch(res["t"], x, pick, frame, hop, fmin, fmax, tau_min, tau_max, rows_np),
               fused_speedup=round(tt[0] / t[0], 3))
        res.pop("t")
        torch.cuda.empty_cache()
        fused_job["voiced_fraction"] = round(float((full["f0"] > 0).float().mean().item()), 4)

    line = {"bench": "pitch", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "f64_peak_flops": F64_PEAK_FLOPS, "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
