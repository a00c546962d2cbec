#!/usr/bin/env python3
"""Interpolation at arbitrary positions on one MI355X: 32 channels x 10 minutes
of audio at 16 kHz, every job for linear and for cubic.

Jobs:
  vibrato_shared   one explicit curve for every channel: rate 1 with a +-3 %
                   vibrato at 5.5 Hz, as many outputs as inputs;
  vibrato_per_row  the same curve with its own phase per channel, one position
                   row per channel;
  uniform_3, uniform_1_3, uniform_441_160
                   no position array: position k = start + k * step.

Each job is one launch on device-resident rows, timed with HIP events on the
launch stream after warm-up of every shape: `--reps` single calls, reported as
median, minimum and maximum (the spread).  Calls that are compared are timed in
the same loop, alternating: the shared-curve job on the library's default route
(a workgroup takes its run of positions through 8 channels) and with knob
INTERP_ROWS = 1 (one channel per workgroup), and the uniform linear jobs against
the fixed-ratio linear resampler at the same ratio (k_resample_linear: the same
memory traffic).  Every job is also timed against a torch baseline (floor,
index_select / gather, arithmetic on the same tensors).

Bytes are the algorithm's: the outputs, the positions where an array is read
(once when shared), and the span of input the positions cover.  The ceiling of
a job is the same byte mix moved by a streaming kernel with no arithmetic
(scripts/membench.hip k_rwmix, best of a few grid sizes), timed in the same run
in the same way.  Every job's output is checked in the run against the float32
model of tests/interp_util.py on the first and last rows, bit for bit.  Prints
one JSON line and writes it to profiles/interp_bench.json.

    python scripts/interpbench.py [--reps 10] [--seconds 600] [--channels 32] [--json FILE]
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
import interp_util as iu  # noqa: E402

RATE = 16000
UNIFORM = (("uniform_3", 3.0, 1, 3), ("uniform_1_3", 1.0 / 3.0, 3, 1), ("uniform_441_160", 441.0 / 160.0, 160, 441))


def timed_alternating(fns, reps):
    """name -> [ms per call]: every fn warmed up, then `reps` rounds that time each fn once in turn"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    s = torch.cuda.current_stream()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}


def stat(ts):
    return {"ms": round(float(np.median(ts)), 4), "ms_min": round(float(np.min(ts)), 4),
            "ms_max": round(float(np.max(ts)), 4), "reps": len(ts)}


def ceiling(in_floats, out_floats, reps):
    """the job's bytes through membench k_rwmix: best grid size by median"""
    path = os.path.join(ROOT, "scripts", "libmembench.so")
    if not os.path.exists(path):
        raise SystemExit("scripts/libmembench.so missing: run `make -C vv-dsp_amd membench`")
    mb = C.CDLL(path)
    mb.membench_rwmix.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
    a = torch.rand(in_floats, device="cuda")
    b = torch.empty(out_floats, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def run(blocks):
        assert mb.membench_rwmix(a.data_ptr(), b.data_ptr(), in_floats // 4, out_floats // 4, blocks, s) == 0
    ts = timed_alternating({blocks: (lambda blocks=blocks: run(blocks)) for blocks in (2048, 4096, 16384)}, reps)
    blocks = min(ts, key=lambda k: np.median(ts[k]))
    del a, b
    return dict(stat(ts[blocks]), blocks=blocks,
                what="the job's read and written bytes through a streaming kernel (membench k_rwmix)")


def vibrato(n, phase):
    """n float32 positions: k + A sin(w k + phase), A w = 0.03 (rate within +-3 % of 1), 5.5 Hz at 16 kHz"""
    w = 2.0 * np.pi * 5.5 / RATE
    k = torch.arange(n, dtype=torch.float64, device="cuda")
    return (k + (0.03 / w) * torch.sin(w * k + phase)).float()


def torch_baseline(x, pos, method):
    """floor, gather and the arithmetic on the same tensors (positions [m] shared or [b, m])"""
    n = x.shape[1]
    p = pos.clamp(0.0, float(n - 1))
    i = p.floor().clamp(max=float(max(n - 2, 0))).long()
    t = p - i.float()

    def take(idx):
        idx = idx.clamp(0, n - 1)
        return x.index_select(1, idx) if idx.dim() == 1 else x.gather(1, idx)
    if method == "linear":
        return (1.0 - t) * take(i) + t * take(i + 1)
    p0, p1, p2, p3 = take(i - 1), take(i), take(i + 1), take(i + 2)
    m1, m2 = 0.5 * (p2 - p0), 0.5 * (p3 - p1)
    t2 = t * t
    t3 = t2 * t
    return (2 * t3 - 3 * t2 + 1) * p1 + (t3 - 2 * t2 + t) * m1 + (3 * t2 - 2 * t3) * p2 + (t3 - t2) * m2


def check(x, y, pos_of_row, method):
    """first and last rows of y against the float32 model, bit for bit"""
    ok, rows = True, sorted({0, x.shape[0] - 1})
    for r in rows:
        want = iu.model(x[r].cpu().numpy(), pos_of_row(r), method)
        ok = ok and iu.same(y[r].cpu().numpy(), want)
    return {"ok": bool(ok), "what": f"rows {rows} bit-identical to the float32 model"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "interp_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("interpbench needs an MI355X: no timing without a GPU")
    torch.cuda.set_device(0)
    nch, n = o.channels, o.seconds * RATE
    x = torch.rand(nch, n, device="cuda") - 0.5
    workload = f"{nch} ch x {o.seconds} s at 16 kHz"
    jobs = []

    def job(name, method, m, fns, pos_bytes, span, pos_of_row, y, base_fn, extra):
        """fns: label -> call writing y; the first label is the library's own choice of route"""
        ts = timed_alternating(fns, o.reps)
        first = next(iter(fns))
        fns[first]()
        chk = check(x, y, pos_of_row, method)
        routes_same = True
        for label, fn in fns.items():
            if label.startswith("rows_") and label != first:
                ref = y.clone()
                fn()
                routes_same = routes_same and torch.equal(ref.view(torch.int32), y.view(torch.int32))
        chk["ok"] = chk["ok"] and routes_same
        byts = 4 * nch * m + pos_bytes + 4 * nch * span
        ceil = ceiling((pos_bytes + 4 * nch * span) // 4, nch * m, o.reps)
        tb = timed_alternating({"torch": base_fn}, o.torch_reps)["torch"]
        med = float(np.median(ts[first]))
        j = {"job": name, "method": method, "workload": workload, "outputs": nch * m, "bytes": byts,
             "GBs": round(byts / med / 1e6, 1), "copy_ceiling": ceil,
             "frac_of_copy_ceiling": round(ceil["ms"] / med, 4), "torch_baseline": stat(tb),
             "speedup_over_torch": round(float(np.median(tb)) / med, 2), "check": chk}
        j.update(stat(ts[first]))
        j["alternated"] = {k: stat(v) for k, v in ts.items()}
        j.update(extra)
        jobs.append(j)

    for method in iu.METHODS:
        # -- explicit positions: one curve for every channel, then one per channel
        y = torch.empty(nch, n, device="cuda")
        pos = vibrato(n, 0.0)
        pos_np = pos.cpu().numpy()
        vv.debug_clear("STAT_INTERP_ROWS")
        fns = {"default": lambda: vv.interpolate(x, pos, method, out=y),
               "rows_1": lambda: _one_row(lambda: vv.interpolate(x, pos, method, out=y))}
        job("vibrato_shared", method, n, fns, 4 * n, n, lambda r: pos_np, y,
            lambda: torch_baseline(x, pos, method), {"positions": "explicit, shared"})
        jobs[-1]["default_is_rows_route"] = vv.debug_get("STAT_INTERP_ROWS") > 0
        del pos
        posr = torch.stack([vibrato(n, 2.0 * np.pi * r / nch) for r in range(nch)])
        job("vibrato_per_row", method, n, {"default": lambda: vv.interpolate(x, posr, method, out=y)}, 4 * nch * n, n,
            lambda r: posr[r].cpu().numpy(), y, lambda: torch_baseline(x, posr, method),
            {"positions": "explicit, per row"})
        del posr, y
        torch.cuda.empty_cache()
        # -- uniform positions, against the linear resampler at the same ratio
        for name, step, num, den in UNIFORM:
            rs = vv.Resampler(num, den, sinc=False)
            m = rs.output_length(n)
            y = torch.empty(nch, m, device="cuda")
            y2 = torch.empty(nch, m, device="cuda")
            pos_np = iu.uniform_positions(0.0, step, m)
            pos = torch.from_numpy(pos_np).cuda()
            fns = {"default": lambda: vv.interpolate_uniform(x, 0.0, step, m, method, out=y)}
            extra = {"positions": f"uniform, step {step:.6g}", "step": step}
            if method == "linear":
                fns["resampler_linear"] = lambda: rs(x, out=y2)
            job(name, method, m, fns, 0, n, lambda r: pos_np, y, lambda: torch_baseline(x, pos, method), extra)
            if method == "linear":
                j = jobs[-1]
                a, b = j["alternated"]["default"], j["alternated"]["resampler_linear"]
                j["vs_resampler_linear"] = {
                    "ratio": f"{num}/{den}", "interp_ms": a["ms"], "resampler_ms": b["ms"],
                    "interp_over_resampler": round(a["ms"] / b["ms"], 4),
                    "spread_interp": round((a["ms_max"] - a["ms_min"]) / a["ms"], 4),
                    "spread_resampler": round((b["ms_max"] - b["ms_min"]) / b["ms"], 4)}
            del y, y2, pos, rs
            torch.cuda.empty_cache()

    line = {"bench": "interp", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "run_length": vv.interp_run_length(),
            "timing": "HIP events per call, compared calls alternating in one loop: median (ms), minimum, maximum",
            "all_checks_ok": all(j["check"]["ok"] for j in jobs), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


def _one_row(fn):
    with vv.knobs(INTERP_ROWS=1):
        fn()


if __name__ == "__main__":
    main()
