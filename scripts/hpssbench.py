#!/usr/bin/env python3
"""Median filtering and harmonic-percussive separation on one MI355X: 32 channels x
10 minutes at 16 kHz, n_fft 1024 / hop 256, magnitude weights, Wiener masks, margins 1.

  rows_<layout>_masks_<L>  both masks from resident power rows (vv_dsp_hpss_device),
                           layout pitched (544 floats per row) or packed (513), windows
                           31/31 (librosa's default) and 17/17;
  rows_pitched_harm_31, rows_pitched_perc_31
                           one median alone: the time and the frequency direction;
  medfilt_<L>              vv_dsp_medfilt_device on 32 rows of 9.6 M samples, L = 5, 31
                           and 127, and per L the two selects (knob MEDIAN_SELECT);
  signal_hpss              signal -> harmonic and percussive signal (Stft.hpss), next to
  signal_public_calls      the sequence of public calls that defines it, channel by
                           channel (power, hpss masks, spectrogram, the mask product as a
                           torch expression, reconstruct, the division),
  signal_power_rows        the power rows alone, and
  signal_round_trip        spectrogram -> reconstruct -> division with no mask;
  torch_*                  the same definitions as a torch expression on the same
                           tensors: unfold(...).median() over a reflect-padded copy.  The
                           unfolded tensor is L times its input, so the expression runs on
                           a slice (one channel of rows; one row of 9.6 M samples) and its
                           time is multiplied by the number of slices; the JSON says so.

Each job is timed with HIP events on the launch stream: median and minimum of `--reps`
single calls after warm-up.  Every job checks a seeded sample against the numpy model of
tests/median_util.py bit for bit inside the run.  Ceilings, measured in the same run: a
streaming kernel that reads the job's input bytes and writes its output bytes once
(membench k_rwmix), and the select's count of integer compare / add-with-carry
lane-instructions at the vector issue rate (256 CUs x 64 lanes per clock at 2.4 GHz):
2 L^2 per output for the counting select (one compare and one add-with-carry per pair
of a candidate and a key), 64 L for the bitwise one (32 passes), read off the loops of
median_kernels.hip; LDS reads, the halo fill and the masks are not counted, so it is a
floor.  Prints one JSON line.

    python scripts/hpssbench.py [--reps 10] [--seconds 600] [--channels 32] [--json FILE]
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
import median_util as mu  # noqa: E402

NFFT, HOP, K, PITCH = 1024, 256, 513, 544
LANE_RATE = 256 * 64 * 2.4e9          # lane-instructions per second at the vector issue rate
SAMPLE = 24


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


def signal(nch, n, rate, seed):
    """per channel a gliding three-harmonic tone plus a click train over noise: float32 on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / rate
    x = torch.empty(nch, n, device="cuda", dtype=torch.float32)
    for c in range(nch):
        f = 180.0 + 35.0 * c + 60.0 * torch.sin(2 * np.pi * 0.21 * t + c)
        ph = 2 * np.pi * torch.cumsum(f, 0) / rate
        tone = torch.sin(ph) + 0.5 * torch.sin(2 * ph + 0.4) + 0.25 * torch.sin(3 * ph + 1.1)
        noise = torch.randn(n, device="cuda", generator=g, dtype=torch.float32)
        x[c] = (0.3 * tone).to(torch.float32) + 0.02 * noise
        x[c, 1000 + 37 * c::7919] += 0.9
    return x


_mb = None


def stream_ceiling(bytes_read, bytes_written, src, reps):
    """a streaming kernel that reads and writes the job's bytes once (best of 3 grid sizes)"""
    global _mb
    if _mb is None:
        path = os.path.join(ROOT, "scripts", "libmembench.so")
        if not os.path.exists(path):
            raise SystemExit("scripts/libmembench.so missing: run `make -C vv-dsp_amd membench`")
        _mb = C.CDLL(path)
        _mb.membench_rwmix.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_void_p]
    n_in4, n_out4 = bytes_read // 16, bytes_written // 16
    assert src.numel() * src.element_size() >= n_in4 * 16
    y = torch.empty(n_out4 * 4, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    best = None
    for blocks in (2048, 4096, 8192):
        def fn(blocks=blocks):
            assert _mb.membench_rwmix(src.data_ptr(), y.data_ptr(), n_in4, n_out4, blocks, s) == 0
        t = timed(fn, reps)[0]
        best = t if best is None or t < best else best
    del y
    return round(best, 4)


def select_ops(L):
    return 2 * L * L if L < 33 else 64 * L


def floor_ms(outputs_by_window):
    return round(sum(n * select_ops(L) for L, n in outputs_by_window) / LANE_RATE * 1e3, 4)


def sample_rows(nch, frames, seed):
    rng = np.random.default_rng(seed)
    pick = {(0, 0), (0, 1), (nch - 1, frames - 1), (nch - 1, frames - 2)}
    while len(pick) < SAMPLE:
        pick.add((int(rng.integers(nch)), int(rng.integers(frames))))
    return sorted(pick)


def model_rows(power, pick, wh, wp):
    """the model's four rows for each sampled (channel, frame) of power [ch][fr][>= K]"""
    fr = power.shape[1]
    res = {name: [] for name in vv.HPSS_NAMES}
    for c, f in pick:
        idx = mu.fold(np.arange(f - wh // 2, f + wh // 2 + 1), fr, mu.REFLECT)
        block = mu.weights(power[c, torch.from_numpy(idx).cuda(), :K].cpu().numpy(), 1)     # the time window's rows
        H = mu.unkey(np.sort(mu.keys(block), axis=0)[wh // 2])
        P = mu.median_sort(block[wh // 2], wp, mu.REFLECT)
        res["harm"].append(H)
        res["perc"].append(P)
        res["mask_harm"].append(mu.mask_of(H, P, 1.0, mu.WIENER))
        res["mask_perc"].append(mu.mask_of(P, H, 1.0, mu.WIENER))
    return {k: np.stack(v) for k, v in res.items()}


def check_rows(planes, model, pick):
    ok = True
    for name, t in planes.items():
        got = np.stack([t[c, f].cpu().numpy() for c, f in pick])
        ok &= bool(np.array_equal(mu.bits(got), mu.bits(model[name])))
    return {"ok": bool(ok), "rows": len(pick), "what": "seeded rows vs the numpy model, bit for bit"}


def reflect_pad(x, h, dim):
    """x with h reflected values on both ends of dim (h < x.shape[dim])"""
    n = x.shape[dim]
    idx = torch.from_numpy(mu.fold(np.arange(-h, n + h), n, mu.REFLECT)).to(x.device)
    return x.index_select(dim, idx)


def torch_median(x, L, dim):
    return reflect_pad(x, L // 2, dim).unfold(dim, L, 1).median(-1).values


def torch_masks(w, wh, wp):
    H, P = torch_median(w, wh, 0), torch_median(w, wp, 1)
    a, b = H.double() ** 2, P.double() ** 2
    d = a + b
    half = torch.full_like(d, 0.5)
    return H, P, torch.where(d == 0, half, a / d).float(), torch.where(d == 0, half, b / d).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "hpss_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available() or vv.device_count() <= 0:
        raise SystemExit("hpssbench needs an MI355X: no timing without a GPU")
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

    def prm(wh, wp):
        return vv.HpssParams(NFFT, 1, wh, wp, 1.0, 1.0, vv.HPSS_WIENER)

    # ---- resident rows ------------------------------------------------------------------
    pitched = st.power(x, pitch=PITCH)
    packed = pitched[..., :K].contiguous()
    models = {L: model_rows(packed, pick, L, L) for L in (31, 17)}
    plane_bytes = 4 * rows * K
    ceil_masks = {"pitched": stream_ceiling(4 * rows * PITCH, 2 * plane_bytes, pitched, o.reps),
                  "packed": stream_ceiling(plane_bytes, 2 * plane_bytes, packed, o.reps)}
    ceil_one = stream_ceiling(4 * rows * PITCH, plane_bytes, pitched, o.reps)
    rows_ms = {}
    for layout, power in (("pitched", pitched), ("packed", packed)):
        for L in (31, 17):
            def masks_job(power=power, L=L):
                res["r"] = vv.hpss(power, prm(L, L), ("mask_harm", "mask_perc"))
            t = timed(masks_job, o.reps)
            fl = floor_ms([(L, 2 * rows * K)])
            rows_ms[(layout, L)] = t[0]
            report(f"rows_{layout}_masks_{L}", workload + f", rows {power.shape[-1]} floats apart, windows {L}/{L}, "
                   "both masks (two launches: H into scratch; P, H read back, the masks written)", t,
                   check_rows(res["r"], models[L], pick), stream_ceiling_ms=ceil_masks[layout],
                   x_stream_ceiling=round(t[0] / ceil_masks[layout], 2), compare_floor_ms=fl,
                   x_compare_floor=round(t[0] / fl, 2))
            res.pop("r")
    for name in ("harm", "perc"):
        def one_job(name=name):
            res["r"] = vv.hpss(pitched, prm(31, 31), name)
        t = timed(one_job, o.reps)
        fl = floor_ms([(31, rows * K)])
        rows_ms[name] = t[0]
        report(f"rows_pitched_{name}_31", workload + f", pitched rows, window 31, {name} alone (one launch: the "
               + ("time" if name == "harm" else "frequency") + " direction)", t, check_rows(res["r"], models[31], pick),
               stream_ceiling_ms=ceil_one, x_stream_ceiling=round(t[0] / ceil_one, 2), compare_floor_ms=fl,
               x_compare_floor=round(t[0] / fl, 2))
        res.pop("r")

    # torch on one channel of packed rows, times the channels
    w1 = packed[0].sqrt()
    for L in (31, 17):
        def torch_job(L=L):
            res["t"] = torch_masks(w1, L, L)
        tt = timed(torch_job, 3)
        H, P, mh, mp = res.pop("t")
        lib = vv.hpss(packed[0], prm(L, L), vv.HPSS_NAMES)
        ok = bool(torch.equal(H, lib["harm"]) and torch.equal(P, lib["perc"]) and
                  (mh - lib["mask_harm"]).abs().max().item() <= 1e-6 and
                  (mp - lib["mask_perc"]).abs().max().item() <= 1e-6)
        del H, P, mh, mp, lib
        report(f"torch_masks_{L}", f"one channel ({fr} rows) of the packed rows as a torch expression "
               f"(reflect-padded copy, unfold({L}).median() along time and along frequency, f64 masks); ms is the "
               f"slice's time times {nch} channels", (tt[0] * nch, tt[1] * nch),
               {"ok": ok, "what": "both medians equal to the library's on the slice, the masks within 1e-6"},
               slice_ms=round(tt[0], 4), library_speedup=round(tt[0] * nch / rows_ms[("packed", L)], 1))
    del w1, packed, pitched
    torch.cuda.empty_cache()

    # ---- medfilt on 32 rows of n samples -------------------------------------------------
    rng = np.random.default_rng(11)
    pos = np.unique(np.concatenate([np.arange(0, 80), np.arange(n - 80, n), rng.integers(0, n, 400)]))
    y = torch.empty_like(x)
    ceil_med = stream_ceiling(4 * nch * n, 4 * nch * n, x, o.reps)
    xs = {c: x[c].cpu().numpy() for c in (0, nch - 1)}

    def check_medfilt(L):
        ok = True
        for c, xc in xs.items():
            idx = mu.fold(pos[:, None] + np.arange(-(L // 2), L // 2 + 1)[None, :], n, mu.REFLECT)
            want = mu.unkey(np.sort(mu.keys(xc)[idx], axis=1)[:, L // 2])
            got = y[c, torch.from_numpy(pos).cuda()].cpu().numpy()
            ok &= bool(np.array_equal(mu.bits(got), mu.bits(want)))
        return {"ok": bool(ok), "positions": 2 * len(pos), "what": "seeded positions and both ends of two rows vs the "
                "numpy model, bit for bit"}

    med_ms, select_ab = {}, {}
    for L in (5, 31, 127):
        t = timed(lambda L=L: vv.medfilt(x, L, out=y), o.reps)
        med_ms[L] = t[0]
        fl = floor_ms([(L, nch * n)])
        report(f"medfilt_{L}", f"{nch} rows of {n} samples, window {L}, reflect", t, check_medfilt(L),
               stream_ceiling_ms=ceil_med, x_stream_ceiling=round(t[0] / ceil_med, 2), compare_floor_ms=fl,
               x_compare_floor=round(t[0] / fl, 2))
        for sel, name in ((1, "counting"), (2, "bitwise")):
            with vv.knobs(MEDIAN_SELECT=sel):
                ts = timed(lambda L=L: vv.medfilt(x, L, out=y), o.reps)
                ok = check_medfilt(L)["ok"]
            select_ab[f"L{L}_{name}_ms"] = round(ts[0], 4)
            select_ab[f"L{L}_{name}_ok"] = ok
    x1 = x[0]
    for L in (5, 31):
        def torch_med(L=L):
            res["t"] = torch_median(x1, L, 0)
        tt = timed(torch_med, 3)
        ok = bool(torch.equal(res.pop("t"), vv.medfilt(x1, L)))
        report(f"torch_medfilt_{L}", f"one row of {n} samples as a torch expression (reflect-padded copy, "
               f"unfold({L}).median()); ms is the row's time times {nch} rows", (tt[0] * nch, tt[1] * nch),
               {"ok": ok, "what": "equal to the library's row"}, slice_ms=round(tt[0], 4),
               library_speedup=round(tt[0] * nch / med_ms[L], 1))
    del y
    torch.cuda.empty_cache()

    # ---- signal -> two signals -----------------------------------------------------------
    p9 = prm(31, 31)

    def fused_job():
        res["f"] = st.hpss(x, p9)
    tf = timed(fused_job, o.reps)
    fused = res.pop("f")
    ln = fused[0].shape[1]
    mirror = torch.from_numpy(np.where(np.arange(NFFT) < K, np.arange(NFFT), NFFT - np.arange(NFFT))).cuda()
    keep = {}

    def public_job():
        for c in range(nch):
            sig = x[c:c + 1]
            masks = vv.hpss(st.power(sig), p9, ("mask_harm", "mask_perc"))
            spec = torch.view_as_real(st.spectrogram(sig, complex_out=True)[0])
            for i, name in enumerate(("mask_harm", "mask_perc")):
                rows_c = torch.view_as_complex(spec * masks[name][0].index_select(1, mirror)[..., None])
                out = torch.zeros(ln, dtype=torch.float32, device="cuda")
                norm = torch.zeros(ln, dtype=torch.float32, device="cuda")
                st.reconstruct(rows_c, out, norm)
                yc = torch.where(norm > 1e-8, out / norm, torch.zeros_like(out))
                if c in (0, nch - 1):
                    keep[(c, i)] = yc
    tp = timed(public_job, max(3, o.reps // 3))
    same = all(torch.equal(keep[(c, i)].view(torch.int32), fused[i][c].view(torch.int32))
               for c in (0, nch - 1) for i in (0, 1))
    keep.clear()
    report("signal_hpss", workload + ", signal -> harmonic and percussive signal, windows 31/31, in channel groups "
           "under 1 GiB of scratch", tf,
           {"ok": bool(same), "what": "the first and the last channel, both signals, bit-identical to the public calls"},
           public_calls_ms=round(tp[0], 4), x_public_calls=round(tf[0] / tp[0], 3))
    report("signal_public_calls", "the same result channel by channel through the public calls (the mask product, the "
           "zeroing and the division as torch expressions)", tp, {"ok": bool(same), "what": "see signal_hpss"})
    del fused
    pw = torch.empty((nch, fr, K), dtype=torch.float32, device="cuda")
    tw = timed(lambda: st.power(x, out=pw), o.reps)
    report("signal_power_rows", workload + ", signal -> packed power rows alone", tw,
           {"ok": True, "what": "timing only"})
    del pw

    def round_trip():
        for c in range(nch):
            spec = st.spectrogram(x[c:c + 1], complex_out=True)[0]
            out = torch.zeros(ln, dtype=torch.float32, device="cuda")
            norm = torch.zeros(ln, dtype=torch.float32, device="cuda")
            st.reconstruct(spec, out, norm)
            res["y"] = torch.where(norm > 1e-8, out / norm, torch.zeros_like(out))
    tr = timed(round_trip, max(3, o.reps // 3))
    err = (res.pop("y")[NFFT:n - NFFT] - x[nch - 1, NFFT:n - NFFT]).abs().max().item()
    report("signal_round_trip", workload + ", spectrogram -> reconstruct -> division with no mask, channel by channel",
           tr, {"ok": bool(err < 1e-4), "max_abs_err": float(f"{err:.3g}"), "what": "the signal comes back"})

    def torch_signal():
        w = torch.hann_window(NFFT, device="cuda")
        S = torch.stft(x[0], NFFT, HOP, window=w, return_complex=True).T                    # (frames, K)
        _, _, mh, mp = torch_masks(S.abs(), 31, 31)
        res["t"] = [torch.istft((S * m).T, NFFT, HOP, window=w) for m in (mh, mp)]
    tts = timed(torch_signal, 3)
    res.pop("t")
    report("torch_signal_hpss", f"one channel as a torch expression (stft, the unfold medians, f64 masks, two istft); "
           f"ms is the channel's time times {nch} channels", (tts[0] * nch, tts[1] * nch),
           {"ok": True, "what": "timing only (torch.stft's centred frames)"},
           slice_ms=round(tts[0], 4), library_speedup=round(tts[0] * nch / tf[0], 1))

    line = {"bench": "hpss", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
            "reps": o.reps, "timing": "HIP events per call: median (ms) and minimum after two warm-up calls",
            "compare_floor_what": "2 L^2 (counting select, L < 33) or 64 L (bitwise select) integer compare and "
                                  "add-with-carry lane-instructions per output at 256 CUs x 64 lanes x 2.4 GHz",
            "stream_ceiling_what": "membench k_rwmix reading the job's input bytes and writing its output bytes once",
            "select_ab": select_ab, "all_checks_ok": all(j["check"]["ok"] for j in jobs),
            "fused_not_slower_than_public_calls": bool(tf[0] <= tp[0]), "jobs": jobs}
    text = json.dumps(line)
    print(text, flush=True)
    if o.json:
        with open(o.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
