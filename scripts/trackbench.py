#!/usr/bin/env python3
"""f0 tracking over the YIN curves on one MI355X: 32 channels x 10 minutes at 16 kHz.

Two shapes: frame 400 / hop 160, 80-400 Hz (tau 40..200, 161 states), and frame
1024 / hop 256, 60-500 Hz (tau 32..267, 236 states); threshold 0.15, the tracker's
default costs (max_step 8), outputs lag, f0, aperiodicity and cost.  Per shape:
  track       the tracker on resident curves (vv_dsp_pitch_track_device);
  forward     the same asking for the cost alone: the forward pass, no backtrace;
  fused       signal -> tracked planes (vv_dsp_pitch_track_frames_device);
  yin         vv_dsp_pitch_frames_device alone, writing the curves the tracker
              reads: the code path that existed before the tracker, the yardstick;
  torch       the same dynamic program as a per-frame torch loop over all channels
              on the same curves (float64, forward pass only, no backtrace), run on
              the first `--torch-frames` frames and scaled to the whole length (the
              loop is sequential in frames);
  track_256   the tracker on 256 channels (the 32 channels' curves eight times):
              how the time scales with the channel count.  One workgroup per
              channel, a wave per 64 states: 32 channels occupy 32 of 256 CUs,
              256 channels all of them.

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after two warm-up calls.  A seeded sample of channels of the
tracker's planes is checked bit for bit in the run against the f64 model of
tests/track_util.py on the GPU's own curves.  Prints one JSON line.

    python scripts/trackbench.py [--reps 10] [--seconds 600] [--channels 32] [--json FILE]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import vvdsp_amd as vv  # noqa: E402
import track_util as tu  # noqa: E402
from pitchbench import signal  # noqa: E402

SHAPES = [(400, 160, 80.0, 400.0), (1024, 256, 60.0, 500.0)]
THRESHOLD = 0.15
CHECKED = 2                        # channels checked per shape


def timed(fn, reps):
    for _ in range(2):
        fn()
    s = torch.cuda.current_stream()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(s)
        fn()
        b.record(s)
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return float(np.median(t)), float(np.min(t))


def torch_forward(curves, tp, frames):
    """the forward pass as a user would write it in torch: float64, one step per frame over
    all channels; returns D of the last frame (no predecessors kept)"""
    tau_min, tau_max, B = tp.tau_min, tp.tau_max, tp.max_step
    S = tau_max - tau_min + 1
    q = curves[:, :frames, tau_min:tau_max + 1].to(torch.float64)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    taus = torch.arange(tau_min, tau_max + 1, device=q.device, dtype=torch.float64)
    k = torch.arange(-B, B + 1, device=q.device, dtype=torch.float64).abs()
    pen = k[None, :] * (float(tp.lambda_) / taus)[:, None]                    # [S][2B + 1]
    D = q[:, 0].clone()
    DU = torch.full((q.shape[0],), float(tp.unvoiced_cost), device=q.device, dtype=torch.float64)
    inf = torch.full((q.shape[0], B), float("inf"), device=q.device, dtype=torch.float64)
    for t in range(1, frames):
        dmin = D.min(1).values
        band = (torch.cat((inf, D, inf), 1).unfold(1, 2 * B + 1, 1) + pen).min(2).values
        best = torch.minimum(torch.minimum(band, (dmin + float(tp.jump_cost))[:, None]),
                             (DU + float(tp.switch_cost))[:, None])
        DU = torch.minimum(DU, dmin + float(tp.switch_cost)) + float(tp.unvoiced_cost)
        D = best + q[:, t]
    assert D.shape[1] == S
    return D, DU


def check_channels(planes, curves, tp, nch, seed):
    rng = np.random.default_rng(seed)
    pick = sorted(set([0] + [int(c) for c in rng.integers(0, nch, CHECKED - 1)]))
    mp = tu.TrackParams(*(getattr(tp, f) for f, _ in tp._fields_))
    ok = True
    for c in pick:
        want = tu.model(curves[c].cpu().numpy(), mp)
        got = {k: planes[k][c].cpu().numpy() for k in vv.TRACK_NAMES}
        got["lag"] = got["lag"].view(np.uint32)
        ok = ok and tu.same(got, want)
    return {"ok": bool(ok), "channels": pick,
            "what": "seeded channels vs the f64 model on the GPU's curves: lag, f0, aperiodicity and cost bit for bit"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--many", type=int, default=256)
    ap.add_argument("--torch-frames", type=int, default=1500)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "track_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("trackbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    nch, rate = o.channels, 16000
    n = o.seconds * rate
    x = signal(nch, n, rate, 20261021)
    jobs = []
    for frame, hop, fmin, fmax in SHAPES:
        p = vv.PitchParams(float(rate), fmin, fmax, THRESHOLD)
        tp = vv.pitch_track_params(p, frame)
        S = tp.tau_max - tp.tau_min + 1
        fr = vv.num_frames(n, frame, hop)
        workload = (f"{nch} ch x {o.seconds} s at {rate} Hz, frame {frame} hop {hop}, {fmin:g}-{fmax:g} Hz "
                    f"(tau {tp.tau_min}..{tp.tau_max}, {S} states, max_step {tp.max_step}), {fr} frames a channel")
        res = {}

        def report(name, what, t, check, frames=nch * fr, **extra):
            job = {"job": f"{name}_{frame}", "workload": workload + what, "frames": frames, "ms": round(t[0], 4),
                   "ms_min": round(t[1], 4), "frames_per_s": round(frames / t[0] * 1e3, 1), "check": check}
            job.update(extra)
            jobs.append(job)
            return job

        def yin():
            res["c"] = vv.pitch_frames(x, frame, hop, p, ("cmnd",))["cmnd"]

        ty = timed(yin, o.reps)
        curves = res["c"]
        report("yin", ", curves only (the yardstick)", ty, {"ok": True, "what": "tests/test_gpu_pitch_yin.py"},
               curve_bytes=curves.numel() * 4)

        def track():
            res["t"] = vv.pitch_track(curves, tp, vv.TRACK_NAMES)

        vv.debug_clear("STAT_PITCH_TRACK")
        tt = timed(track, o.reps)
        launches = vv.debug_get("STAT_PITCH_TRACK") / (2 + o.reps)
        planes = res["t"]
        chk = check_channels(planes, curves, tp, nch, frame)
        report("track", ", tracker on resident curves", tt, chk, vs_yin=round(tt[0] / ty[0], 3),
               launches_per_call=launches, us_per_frame_step=round(tt[0] * 1e3 / fr, 4),
               voiced_fraction=round(float((planes["lag"] > 0).float().mean().item()), 4),
               occupancy=f"{nch} workgroups of {(S + 63) // 64} waves on {min(nch, 256)} of 256 CUs")

        def forward():
            res["w"] = vv.pitch_track(curves, tp, ("cost",))

        tw = timed(forward, o.reps)
        same = torch.equal(res["w"]["cost"].view(torch.int64), planes["cost"].view(torch.int64))
        report("forward", ", the cost alone: the forward pass without the backtrace", tw,
               {"ok": bool(same), "what": "the cost bit-identical to track"}, of_track=round(tw[0] / tt[0], 3),
               us_per_frame_step=round(tw[0] * 1e3 / fr, 4))

        def fused():
            res["f"] = vv.pitch_track_frames(x, frame, hop, p, tp, vv.TRACK_NAMES)

        tf = timed(fused, o.reps)
        same = all(torch.equal(planes[k].view(torch.int64 if k == "cost" else torch.int32),
                               res["f"][k].view(torch.int64 if k == "cost" else torch.int32)) for k in vv.TRACK_NAMES)
        report("fused", ", signal -> tracked planes", tf, {"ok": bool(same), "what": "every plane bit-identical to track"},
               vs_yin=round(tf[0] / ty[0], 3), vs_yin_plus_track=round(tf[0] / (ty[0] + tt[0]), 3))
        res.pop("f")

        tf_n = min(o.torch_frames, fr)
        t0 = time.perf_counter()
        torch_forward(curves, tp, tf_n)
        torch.cuda.synchronize()
        tms = (time.perf_counter() - t0) * 1e3
        report("torch", f", per-frame torch loop, forward pass only, {tf_n} frames measured and scaled to {fr}",
               (tms * fr / tf_n, tms * fr / tf_n), {"ok": True, "what": "timing only"}, measured_ms=round(tms, 2),
               measured_frames=tf_n, track_speedup=round(tms * fr / tf_n / tt[0], 1))

        reps = max(1, o.many // nch)
        many = curves.repeat(reps, 1, 1)

        def track_many():
            res["m"] = vv.pitch_track(many, tp, vv.TRACK_NAMES)

        tm = timed(track_many, o.reps)
        same = all(torch.equal(res["m"][k][-nch:].view(torch.int64 if k == "cost" else torch.int32),
                               planes[k].view(torch.int64 if k == "cost" else torch.int32)) for k in vv.TRACK_NAMES)
        report(f"track_{reps * nch}", f", tracker on {reps * nch} channels", tm,
               {"ok": bool(same), "what": f"the last {nch} channels bit-identical to track"}, frames=reps * nch * fr,
               vs_track=round(tm[0] / tt[0], 3), occupancy=f"{reps * nch} workgroups of {(S + 63) // 64} waves, one per CU at 256")
        del many
        res.clear()
        del curves, planes
        torch.cuda.empty_cache()

    line = {"bench": "pitch_track", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call after two warm-up calls: median (ms) and minimum",
            "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
