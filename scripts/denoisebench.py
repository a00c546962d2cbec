#!/usr/bin/env python3
"""Spectral noise suppression on one MI355X: 32 channels x 10 minutes at 16 kHz, n_fft 1024 /
hop 256, smooth_len 8, bias 4, floor 0.1, WIENER.

  rows_<layout>_gain_<B>   the gain from resident power rows (vv_dsp_denoise_device, one
                           launch), layout pitched (544 floats per row) or packed (513), the
                           minimum's window B = 97 rows (back = ahead = 48, the default), 17
                           and 385;
  rows_pitched_all_97      all three planes (smooth, noise, gain);
  rows_pitched_gain_97_k512
                           the same rows read as 512 bins (n_fft 1022): what the ninth tile of
                           64 bins, which holds bin 512 alone, costs;
  min_ab                   per window the direct and the blockwise minimum (knob DENOISE_MIN);
  segment_ab               the window of 97 at forced segment lengths (knob DENOISE_SEGMENT);
  signal_denoise           signal -> denoised signal (Stft.denoise), next to
  signal_public_calls      the sequence of public calls that defines it, channel by channel
                           (power, denoise gain, spectrogram, the gain product as a torch
                           expression, reconstruct, the division);
  torch_gain_97            the same definition as a torch expression on the same packed rows,
                           float32: avg_pool1d over a copy padded with the first row,
                           -max_pool1d(-S) padded with +inf, the Wiener gain.

Each job is timed with HIP events on the launch stream: median and minimum of `--reps`
single calls after warm-up.  Every library job checks a seeded sample of rows against the
numpy model of tests/denoise_util.py bit for bit inside the run.  The ceiling, measured in
the same run, is a streaming kernel that reads the job's input bytes and writes its output
bytes once (membench k_rwmix).  Prints one JSON line.

    python scripts/denoisebench.py [--reps 10] [--seconds 600] [--channels 32] [--json FILE]
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
import denoise_util as du  # noqa: E402
from hpssbench import timed, signal, stream_ceiling, sample_rows  # noqa: E402

NFFT, HOP, K, PITCH = 1024, 256, 513, 544
W, BIAS, FLOOR = 8, 4.0, 0.1
REACH = {97: (48, 48), 17: (8, 8), 385: (192, 192)}


def prm(B, n_fft=NFFT):
    back, ahead = REACH[B]
    return vv.denoise_params(n_fft, back=back, ahead=ahead)


def model_rows(power, pick, B, nb=K):
    """the model's three rows for each sampled (channel, frame) of power [ch][fr][>= nb]"""
    back, ahead = REACH[B]
    fr = power.shape[1]
    res = {name: [] for name in du.NAMES}
    for c, f in pick:
        lo, hi = max(0, f - back - (W - 1)), min(fr, f + ahead + 1)       # every row the cell depends on
        m = du.denoise_model(power[c, lo:hi, :nb].cpu().numpy(), 2 * (nb - 1), W, back, ahead, BIAS, FLOOR, du.WIENER)
        for name in du.NAMES:
            res[name].append(m[name][f - lo])
    return {k: np.stack(v) for k, v in res.items()}


def check_rows(planes, model, pick):
    ok = True
    for name, t in planes.items():
        got = np.stack([t[c, f].cpu().numpy() for c, f in pick])
        ok &= bool(np.array_equal(du.bits(got), du.bits(model[name])))
    return {"ok": bool(ok), "rows": len(pick), "what": "seeded rows vs the numpy model, bit for bit"}


def torch_gain(p, back, ahead):
    """(ch, fr, K) float32 -> gain, float32 throughout"""
    x = p.transpose(1, 2)                                                  # (ch, K, fr): pooling runs along time
    xs = torch.cat([x[..., :1].expand(-1, -1, W - 1), x], dim=-1)
    S = torch.nn.functional.avg_pool1d(xs, W, 1)
    neg = torch.nn.functional.pad(-S, (back, ahead), value=float("-inf"))
    M = -torch.nn.functional.max_pool1d(neg, back + ahead + 1, 1)
    q = (x - BIAS * M) / x
    g = torch.clamp(torch.where(q > FLOOR, q, torch.full_like(q, FLOOR)), max=1.0)
    return g.transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "denoise_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("denoisebench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    nch, rate = o.channels, 16000
    n = o.seconds * rate
    x = signal(nch, n, rate, 20261021)
    st = vv.Stft(NFFT, HOP)
    fr = st.frames(n)
    rows = nch * fr
    workload = f"{nch} ch x {o.seconds} s at {rate} Hz, n_fft {NFFT} hop {HOP}: {rows} rows of {K} bins"
    pick = sample_rows(nch, fr, 7)
    jobs, res = [], {}

    def report(name, what, t, check, **extra):
        job = {"job": name, "workload": what, "ms": round(t[0], 4), "ms_min": round(t[1], 4), "check": check}
        job.update(extra)
        jobs.append(job)
        print(json.dumps(job), file=sys.stderr, flush=True)
        return job

    # ---- resident rows ------------------------------------------------------------------
    pitched = st.power(x, pitch=PITCH)
    packed = pitched[..., :K].contiguous()
    models = {B: model_rows(packed, pick, B) for B in REACH}
    plane_bytes = 4 * rows * K
    ceil = {("pitched", 1): stream_ceiling(4 * rows * PITCH, plane_bytes, pitched, o.reps),
            ("packed", 1): stream_ceiling(plane_bytes, plane_bytes, packed, o.reps),
            ("pitched", 3): stream_ceiling(4 * rows * PITCH, 3 * plane_bytes, pitched, o.reps)}
    rows_ms = {}
    for layout, power in (("pitched", pitched), ("packed", packed)):
        for B in REACH:
            def gain_job(power=power, B=B):
                res["r"] = vv.denoise(power, prm(B), "gain")
            t = timed(gain_job, o.reps)
            rows_ms[(layout, B)] = t[0]
            c = ceil[(layout, 1)]
            report(f"rows_{layout}_gain_{B}", workload + f", rows {power.shape[-1]} floats apart, smooth_len {W}, "
                   f"window {B} rows, the gain (one launch)", t, check_rows(res.pop("r"), models[B], pick),
                   stream_ceiling_ms=c, x_stream_ceiling=round(t[0] / c, 2))

    def all_job():
        res["r"] = vv.denoise(pitched, prm(97), du.NAMES)
    t = timed(all_job, o.reps)
    c = ceil[("pitched", 3)]
    report("rows_pitched_all_97", workload + ", pitched rows, window 97, smooth, noise and gain (one launch)", t,
           check_rows(res.pop("r"), models[97], pick), stream_ceiling_ms=c, x_stream_ceiling=round(t[0] / c, 2))

    def k512_job():
        res["r"] = vv.denoise(pitched, prm(97, 1022), "gain")
    t = timed(k512_job, o.reps)
    report("rows_pitched_gain_97_k512", workload + ", pitched rows read as 512 bins (n_fft 1022): eight full tiles",
           t, check_rows(res.pop("r"), model_rows(pitched, pick, 97, 512), pick),
           x_513_bins=round(rows_ms[("pitched", 97)] / t[0], 3))

    min_ab, segment_ab = {}, {}
    for B in REACH:
        for how, name in ((1, "direct"), (2, "blockwise")):
            with vv.knobs(DENOISE_MIN=how):
                ts = timed(lambda B=B: res.__setitem__("r", vv.denoise(pitched, prm(B), "gain")), o.reps)
                ok = check_rows(res.pop("r"), models[B], pick)["ok"]
            min_ab[f"B{B}_{name}_ms"] = round(ts[0], 4)
            min_ab[f"B{B}_{name}_ok"] = ok
    for L in (48, 64, 96, 130, 256, 443):
        with vv.knobs(DENOISE_SEGMENT=L):
            ts = timed(lambda: res.__setitem__("r", vv.denoise(pitched, prm(97), "gain")), o.reps)
            ok = check_rows(res.pop("r"), models[97], pick)["ok"]
        segment_ab[f"L{L}_ms"] = round(ts[0], 4)
        segment_ab[f"L{L}_ok"] = ok

    # torch on the packed rows
    back, ahead = REACH[97]
    tt = timed(lambda: res.__setitem__("t", torch_gain(packed, back, ahead)), 3)
    lib = vv.denoise(packed, prm(97), "gain")["gain"]
    diff = (res.pop("t") - lib).abs()
    close = float((diff <= 1e-3).float().mean().item())
    del diff, lib
    report("torch_gain_97", workload + ", packed rows as a float32 torch expression (a copy padded with the first row, "
           "avg_pool1d, -max_pool1d(-S) padded with +inf, the Wiener gain)", tt,
           {"ok": close > 0.999, "share_within_1e-3": round(close, 6),
            "what": "the gain within 1e-3 of the library's (float32 sums in another order)"},
           library_speedup=round(tt[0] / rows_ms[("packed", 97)], 1))
    del packed, pitched
    torch.cuda.empty_cache()

    # ---- signal -> signal ------------------------------------------------------------------
    p9 = prm(97)
    tf = timed(lambda: res.__setitem__("f", st.denoise(x, p9)), o.reps)
    fused = res.pop("f")
    ln = fused.shape[1]
    mirror = torch.from_numpy(np.where(np.arange(NFFT) < K, np.arange(NFFT), NFFT - np.arange(NFFT))).cuda()
    keep = {}

    def public_job():
        for c in range(nch):
            sig = x[c:c + 1]
            gain = vv.denoise(st.power(sig), p9, "gain")["gain"]
            spec = torch.view_as_real(st.spectrogram(sig, complex_out=True)[0])
            rows_c = torch.view_as_complex(spec * gain[0].index_select(1, mirror)[..., None])
            out = torch.zeros(ln, dtype=torch.float32, device="cuda")
            norm = torch.zeros(ln, dtype=torch.float32, device="cuda")
            st.reconstruct(rows_c, out, norm)
            yc = torch.where(norm > 1e-8, out / norm, torch.zeros_like(out))
            if c in (0, nch - 1):
                keep[c] = yc
    tp = timed(public_job, max(3, o.reps // 3))
    same = all(torch.equal(keep[c].view(torch.int32), fused[c].view(torch.int32)) for c in (0, nch - 1))
    keep.clear()
    report("signal_denoise", workload + ", signal -> denoised signal, window 97, in channel groups under 1 GiB of "
           "scratch", tf,
           {"ok": bool(same), "what": "the first and the last channel bit-identical to the public calls"},
           public_calls_ms=round(tp[0], 4), x_public_calls=round(tf[0] / tp[0], 3))
    report("signal_public_calls", "the same result channel by channel through the public calls (the gain product, the "
           "zeroing and the division as torch expressions)", tp, {"ok": bool(same), "what": "see signal_denoise"})

    line = {"bench": "denoise", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms) and minimum after two warm-up calls",
            "stream_ceiling_what": "membench k_rwmix reading the job's input bytes and writing its output bytes once",
            "min_ab": min_ab, "segment_ab": segment_ab,
            "all_checks_ok": bool(all(j["check"]["ok"] for j in jobs) and
                                  all(v for k, v in {**min_ab, **segment_ab}.items() if k.endswith("_ok"))),
            "fused_not_slower_than_public_calls": bool(tf[0] <= tp[0]), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
