#!/usr/bin/env python3
"""The LPC residual and synthesis filters on one MI355X: 32 channels x 480000
samples (30 s at 16 kHz), orders 16 and 32, a new row of coefficients every 256
samples (the rows are the signal's own centred LPC rows, frames of 512, Hamming).

  residual_<p>        signal -> residual, every channel through its own rows;
  synth_exact_<p>     the residual as 1875 rows of 8192 samples -> one recursion per row;
  synth_chunked_<p>   the residual [32][480000] -> chunks of 1024, three launches.

Each job is timed with HIP events on the launch stream: median and minimum of
`--reps` single calls after warm-up, and the mean of a back-to-back burst.  Beside
each time stands the streaming ceiling (a copy kernel over the same samples,
scripts/membench.hip k_rw) and a CPU floor: scipy.signal.lfilter per segment with
zi carried, one channel on one core, in samples per second.  Checked in the run:
windows of the residual and the first 4096 samples of rows of the exact synthesis
against the numpy model (tests/lpc_filter_util.py), bit for bit; the chunked
synthesis against the recursion of the whole rows (knob LPC_SYNTH_CHUNK = 0), float
against float, within one float ulp plus 1e-10 of the peak, with the number of
floats that differ.
No thresholds on speed: the numbers are reported.  Prints one JSON line.

    python scripts/lpcfilterbench.py [--reps 5] [--json FILE]
    python scripts/lpcfilterbench.py --ab [--json FILE]     # the chunk constants' A/B, one line per point
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np
import torch
from scipy.signal import lfilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vv-dsp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vvdsp_amd as vv  # noqa: E402
import lpc_filter_util as fu  # noqa: E402
from frames_util import hamming  # noqa: E402

RATE, SEG, FRAME = 16000, 256, 512
ORDERS = (16, 32)
EXACT_ROW = 8192
with open(os.path.join(ROOT, "include", "vv_dsp", "envelope", "lpc_filter.h")) as _f:
    CHUNK = int(re.search(r"#define\s+VV_DSP_LPC_SYNTH_CHUNK\s+(\d+)", _f.read()).group(1))


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
    return {"what": "streaming copy of the same samples (membench k_rw, float4 per lane, best of 3 grid sizes)",
            "blocks": best[0], "ms": round(best[1][0], 4), "ms_min": round(best[1][1], 4),
            "ms_back_to_back": round(best[1][2], 4)}


def signal(nch, n, seed):
    """per channel: harmonics of a gliding fundamental weighted by three resonances, over noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / RATE
    x = torch.empty(nch, n, device="cuda", dtype=torch.float32)
    for c in range(nch):
        f0 = 110.0 + 6.0 * (c % 32) + 25.0 * torch.sin(2 * np.pi * 0.17 * t + c)
        ph = 2 * np.pi * torch.cumsum(f0.double(), 0).float() / RATE
        acc = torch.zeros_like(t)
        for h in range(1, 20):
            fh = h * (110.0 + 6.0 * (c % 32))
            w = sum(1.0 / (1.0 + ((fh - fc) / bw) ** 2) for fc, bw in
                    ((600.0 + 20 * (c % 32), 90.0), (1400.0 + 30 * (c % 32), 120.0), (2700.0, 160.0)))
            acc += float(w) * torch.sin(h * ph + 0.37 * h)
        x[c] = 0.2 * acc / acc.abs().max() + 0.01 * torch.randn(n, device="cuda", generator=g, dtype=torch.float32)
    return x


def rows_of(x, p):
    win = torch.from_numpy(np.asarray(hamming(FRAME), np.float32)).cuda()
    a, _ = vv.lpc_frames(x, FRAME, SEG, p, window=win, center=True)
    return a


def cpu_floor(x0, a0, which, segments=200):
    """scipy.signal.lfilter per segment with zi carried, one channel, one core -> samples per second"""
    x0 = x0[:segments * SEG].astype(np.float64)
    a0 = a0.astype(np.float64)
    p = a0.shape[1] - 1
    zi = np.zeros(p)
    t0 = time.perf_counter()
    for f in range(segments):
        seg = x0[f * SEG:(f + 1) * SEG]
        if which == "residual":
            _, zi = lfilter(a0[min(f, len(a0) - 1)], [1.0], seg, zi=zi)
        else:
            _, zi = lfilter([1.0], a0[min(f, len(a0) - 1)], seg, zi=zi)
    return segments * SEG / (time.perf_counter() - t0)


def bits_equal(a, b):
    return bool(np.array_equal(fu.bits(a), fu.bits(b)))


def ab(o):
    """the exact / chunked crossover at 1, 32 and 256 channels, and chunks of 256, 1024 and 4096 on
    the workload; one JSON line per point"""
    lines = []
    for p in ORDERS:
        for nch in (1, 32, 256):
            x = signal(min(nch, 32), 65536, 7 + nch).repeat((nch + 31) // 32, 1)[:nch].contiguous()
            a = rows_of(x, p)
            e = vv.lpc_residual(x, a, SEG)
            y = torch.empty_like(e)
            for n in (2048, 4096, 8192, 16384, 32768, 65536):
                line = {"ab": "crossover", "order": p, "channels": nch, "n": n}
                for name, knob in (("exact", 0), ("chunk1024", 1024)):
                    with vv.knobs(LPC_SYNTH_CHUNK=knob):
                        t = timed(lambda: vv.lpc_synth(e[:, :n], a, SEG, out=y[:, :n]), o.reps, o.burst)
                    line[name + "_ms"], line[name + "_ms_min"] = round(t[0], 4), round(t[1], 4)
                lines.append(line)
                print(json.dumps(line), flush=True)
        x = signal(32, 480000, 20261021)
        a = rows_of(x, p)
        e = vv.lpc_residual(x, a, SEG)
        y = torch.empty_like(e)
        line = {"ab": "chunk", "order": p, "channels": 32, "n": 480000}
        for L in (256, 1024, 4096):
            with vv.knobs(LPC_SYNTH_CHUNK=L):
                t = timed(lambda: vv.lpc_synth(e, a, SEG, out=y), o.reps, o.burst)
            line[f"chunk{L}_ms"], line[f"chunk{L}_ms_min"] = round(t[0], 4), round(t[1], 4)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--burst", type=int, default=3)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--samples", type=int, default=480000)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--json", default=None)
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("lpcfilterbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    if o.ab:
        o.json = o.json or os.path.join(ROOT, "profiles", "lpc_filter_chunk_ab.jsonl")
        return ab(o)
    o.json = o.json or os.path.join(ROOT, "profiles", "lpc_filter_bench.json")
    nch, n = o.channels, o.samples
    assert (nch * n) % EXACT_ROW == 0 and n % SEG == 0
    x = signal(nch, n, 20261021)
    ceil = copy_ceiling(x, torch.empty_like(x), o.reps, o.burst)
    workload = f"{nch} ch x {n} samples, seg_len {SEG}"
    jobs = []

    def report(name, what, t, check, **extra):
        med, mn, b2b = t
        job = {"job": name, "workload": workload + what, "samples": nch * n, "ms": round(med, 4),
               "ms_min": round(mn, 4), "ms_back_to_back": round(b2b, 4),
               "samples_per_s": round(nch * n / med * 1e3, 1), "frac_of_copy_ceiling": round(ceil["ms"] / med, 4),
               "check": check}
        job.update(extra)
        jobs.append(job)

    for p in ORDERS:
        a = rows_of(x, p)                       # [nch][n / SEG][p + 1]
        frames = a.shape[1]
        xh, ah = x[0].cpu().numpy(), a[0].cpu().numpy()
        e = torch.empty_like(x)
        # ---- residual
        t = timed(lambda: vv.lpc_residual(x, a, SEG, out=e), o.reps, o.burst)
        ok = True
        for c in (0, nch - 1):
            xc, ac, ec = x[c].cpu().numpy(), a[c].cpu().numpy(), e[c].cpu().numpy()
            for s in (0, n // 2 - 1000, n - 3000):
                st = np.zeros(p) if s == 0 else xc[s - p:s][::-1].astype(np.float64)
                want, _ = fu.residual_vec(xc[s:s + 3000], ac, SEG, s, None, st[None])
                ok = ok and bits_equal(ec[s:s + 3000], want[0])
        report(f"residual_{p}", f", order {p}", t,
               {"ok": ok, "what": "windows of 3000 samples of the first and last channel vs the numpy model, bit for bit"},
               cpu_floor_samples_per_s=round(cpu_floor(xh, ah, "residual"), 1))
        # ---- exact synthesis: the same samples as rows of 8192, 32 rows of coefficients each
        rows = nch * n // EXACT_ROW
        per = EXACT_ROW // SEG
        e2, a2 = e.reshape(rows, EXACT_ROW), a.reshape(-1, p + 1)[:rows * per].reshape(rows, per, p + 1)
        y2 = torch.empty_like(e2)
        vv.debug_clear("STAT_LPC_SYNTH_EXACT")
        t = timed(lambda: vv.lpc_synth(e2, a2, SEG, out=y2), o.reps, o.burst)
        took = vv.debug_get("STAT_LPC_SYNTH_EXACT") > 0
        pick = [0, rows // 2, rows - 1]
        want = fu.synth_seq(e2[pick, :4096].cpu().numpy(), a2[pick].cpu().numpy(), SEG)[0]
        ok = bits_equal(y2[pick, :4096].cpu().numpy(), want)
        report(f"synth_exact_{p}", f", order {p}, as {rows} rows of {EXACT_ROW}", t,
               {"ok": ok and took, "what": "the first 4096 samples of three rows vs the numpy model, bit for bit; "
                                           "the exact route's counter moved"},
               cpu_floor_samples_per_s=round(cpu_floor(e[0].cpu().numpy(), ah, "synth"), 1))
        # ---- chunked synthesis of the long rows
        y = torch.empty_like(e)
        vv.debug_clear("STAT_LPC_SYNTH_CHUNKED")
        t = timed(lambda: vv.lpc_synth(e, a, SEG, out=y), o.reps, o.burst)
        took = vv.debug_get("STAT_LPC_SYNTH_CHUNKED") > 0
        with vv.knobs(LPC_SYNTH_CHUNK=0):
            seq = vv.lpc_synth(e, a, SEG)
        torch.cuda.synchronize()
        yh, sh = y.cpu().numpy(), seq.cpu().numpy()
        peak = float(np.abs(sh).max())
        gap = np.abs(yh.astype(np.float64) - sh.astype(np.float64))
        bound = 2.0 * fu.half_ulp32(sh.astype(np.float64)) + 1e-10 * peak
        differ = int(np.sum(fu.bits(yh) != fu.bits(sh)))
        back = float(np.abs(yh - x.cpu().numpy()).max() / float(x.abs().max()))
        report(f"synth_chunked_{p}", f", order {p}, chunks of {CHUNK}", t,
               {"ok": bool(np.all(gap <= bound)) and took, "floats_differing": differ, "floats": int(yh.size),
                "round_trip_error_of_peak": float(f"{back:.3g}"),
                "what": "every sample vs the one-recursion route (whose bits the tests pin): within a float ulp "
                        "+ 1e-10 of the peak; the chunked route's counter moved"},
               scratch_bytes=8 * p * (p + 2) * ((n + CHUNK - 1) // CHUNK) * nch)
        del a, e, y, y2, seq
        torch.cuda.empty_cache()

    line = {"bench": "lpc_filter", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms), minimum, back-to-back burst mean",
            "copy_ceiling": ceil, "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
