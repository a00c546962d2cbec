#!/usr/bin/env python3
"""Same-buffer A/B of library builds in ONE process (timing tool, not a test).

Each build (`--libs a.so,b.so,...`) is dlopen'ed on its own (RTLD_LOCAL: its own
kernels, caches and knobs) and every case runs through the C device API of
each build on the SAME device buffers, interleaved A, B, A, B ... per round, so
neither the placement of a fresh allocation (up to 5 % on the headline,
profiles/r03_kbench_placement.jsonl) nor the box separates the builds.  Time =
HIP events around each launch on the launch stream; prints one JSON line per
(case, build) with the median and its ratio to the first build.

    python scripts/ab2.py --libs scripts/ab/prev.so,vv-dsp_amd/lib/libvvdsp_amd.so --cases fir,stft
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
PEAK = 8000.0
vp, sz = C.c_void_p, C.c_size_t


class StftParams(C.Structure):
    _fields_ = [("fft_size", C.c_size_t), ("hop_size", C.c_size_t), ("window", C.c_int)]


def load(spec):
    """`path` or `path@KNOB=V+KNOB2=V2`: knobs set in that build (vvhip_debug_set);
    to compare knob settings of one build, pass copies of the .so under other names
    (one file is loaded once per process)"""
    path, _, knobs = spec.partition("@")
    L = C.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_NOW)
    L.vvhip_debug_set.argtypes = [C.c_char_p, C.c_longlong]
    for kv in filter(None, knobs.split("+")):
        k, v = kv.split("=")
        if L.vvhip_debug_set(k.encode(), int(v)) != 0:
            raise SystemExit(f"{path}: unknown knob {k}")
    L.vvhip_last_error.restype = C.c_char_p
    L.vv_dsp_fir_design_lowpass.argtypes = [vp, sz, C.c_float, C.c_int]
    L.vv_dsp_fir_plan_create.argtypes = [vp, sz, C.POINTER(vp)]
    L.vv_dsp_fir_apply_fft_device.argtypes = [vp, vp, vp, sz, sz, sz, sz, vp]
    L.vv_dsp_stft_create.argtypes = [C.POINTER(StftParams), C.POINTER(vp)]
    for f in ("spectrogram", "power"):
        getattr(L, f"vv_dsp_stft_{f}_device").argtypes = [vp, vp, sz, sz, sz, vp, sz, vp, C.POINTER(sz)]
    if hasattr(L, "vv_dsp_stft_power_pitched_device"):
        L.vv_dsp_stft_power_pitched_device.argtypes = [vp, vp, sz, sz, sz, vp, sz, sz, vp, C.POINTER(sz)]
    for f in ("log_mel", "mfcc"):
        getattr(L, f"vv_dsp_stft_{f}_device").argtypes = [vp, vp, vp, sz, sz, sz, vp, sz, vp, C.POINTER(sz)]
    L.vv_dsp_mfcc_init.argtypes = [sz, sz, sz, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float,
                                   C.c_float, C.POINTER(vp)]
    L.vv_dsp_fft_make_plan_many.argtypes = [sz, C.c_int, C.c_int, sz, C.POINTER(vp)]
    L.vv_dsp_fft_execute_device.argtypes = [vp, vp, vp, vp]
    return L


def ok(L, st, what):
    if st != 0:
        raise RuntimeError(f"{what}: status {st}: {L.vvhip_last_error().decode()}")


_BUF = {}


def buf(key, make):
    if key not in _BUF:
        _BUF[key] = make()
    return _BUF[key]


def frames_of(n, nfft=1024, hop=256):
    return 1 if n < nfft else 1 + (n - nfft + hop) // hop


def case_fir(L, s, nch=8, n=1 << 24, taps=257):
    x, y = buf(("fir", nch, n), lambda: (torch.rand(nch, n, device="cuda") * 2 - 1, torch.empty(nch, n, device="cuda")))
    h = np.zeros(taps, np.float32)
    ok(L, L.vv_dsp_fir_design_lowpass(h.ctypes.data, taps, 0.25, 2), "design")
    p = vp()
    ok(L, L.vv_dsp_fir_plan_create(h.ctypes.data, taps, C.byref(p)), "fir plan")
    return (lambda: ok(L, L.vv_dsp_fir_apply_fft_device(p, x.data_ptr(), y.data_ptr(), n, nch, n, n, s), "fir")), \
        2 * nch * n * 4, (lambda: y.clone())


def _stft(L):
    h = vp()
    ok(L, L.vv_dsp_stft_create(C.byref(StftParams(1024, 256, 1)), C.byref(h)), "stft create")
    return h


def case_stft_nfft(L, s, nfft, hop, nch=32, seconds=600, sr=48000, power=False):
    """magnitude rows (power: rows of bins 0..nfft/2) at any nfft (speech lengths: the
    mixed-radix register kernels)"""
    n = seconds * sr
    fr = frames_of(n, nfft, hop)
    w = nfft // 2 + 1 if power else nfft
    sig, out = buf(("stftn", nfft, hop, nch, n, w), lambda: (torch.rand(nch, n, device="cuda") * 2 - 1,
                                                             torch.empty(nch, fr, w, device="cuda")))
    h = vp()
    ok(L, L.vv_dsp_stft_create(C.byref(StftParams(nfft, hop, 1)), C.byref(h)), "stft create")
    nf = sz()
    f = L.vv_dsp_stft_power_device if power else L.vv_dsp_stft_spectrogram_device
    return (lambda: ok(L, f(h, sig.data_ptr(), n, nch, n, out.data_ptr(), fr * w, s, C.byref(nf)), "stft")), \
        nch * n * 4 + nch * fr * w * 4, (lambda: out.clone())


def case_stft_cpx(L, s, nfft, hop, nch=8, seconds=120, sr=48000):
    """complex rows [ch][frame][nfft] (vv_dsp_stft_spectrum_device)"""
    n = seconds * sr
    fr = frames_of(n, nfft, hop)
    sig, out = buf(("stftc", nfft, hop, nch, n), lambda: (torch.rand(nch, n, device="cuda") * 2 - 1,
                                                          torch.empty(nch, fr, nfft, dtype=torch.complex64,
                                                                      device="cuda")))
    h = vp()
    ok(L, L.vv_dsp_stft_create(C.byref(StftParams(nfft, hop, 1)), C.byref(h)), "stft create")
    nf = sz()
    f = L.vv_dsp_stft_spectrum_device
    f.argtypes = [vp, vp, sz, sz, sz, vp, sz, vp, C.POINTER(sz)]
    return (lambda: ok(L, f(h, sig.data_ptr(), n, nch, n, out.data_ptr(), fr * nfft, s, C.byref(nf)), "stftc")), \
        nch * n * 4 + nch * fr * nfft * 8, (lambda: out.clone())


def case_stft_rows(L, s, kind, nch, seconds):
    """kind mag / pow (packed 513-float rows) / pow544 (rows 544 floats apart;
    bytes counted as the 513 floats written)"""
    n = seconds * 48000
    fr = frames_of(n)
    w = {"mag": 1024, "pow": 513, "pow544": 544}[kind]
    sig, out = buf(("stft", kind, nch, n), lambda: (torch.rand(nch, n, device="cuda") * 2 - 1,
                                                    torch.empty(nch, fr, w, device="cuda")))
    h = _stft(L)
    nf = sz()
    if kind == "pow544":
        f = L.vv_dsp_stft_power_pitched_device
        run = lambda: ok(L, f(h, sig.data_ptr(), n, nch, n, out.data_ptr(), fr * w, w, s, C.byref(nf)), "stft")  # noqa
        return run, nch * n * 4 + nch * fr * 513 * 4, (lambda: out[:, :, :513].clone())
    f = L.vv_dsp_stft_spectrogram_device if kind == "mag" else L.vv_dsp_stft_power_device
    return (lambda: ok(L, f(h, sig.data_ptr(), n, nch, n, out.data_ptr(), fr * w, s, C.byref(nf)), "stft")), \
        nch * n * 4 + nch * fr * w * 4, (lambda: out.clone())


def case_mel(L, s, mfcc, nch=32, seconds=600):
    n = seconds * 48000
    fr = frames_of(n)
    w = 13 if mfcc else 40
    sig, out = buf(("mel", mfcc, nch, n), lambda: (torch.rand(nch, n, device="cuda") * 2 - 1,
                                                   torch.empty(nch, fr, w, device="cuda")))
    h = _stft(L)
    m = vp()
    ok(L, L.vv_dsp_mfcc_init(1024, 40, 13, 48000.0, 20.0, 20000.0, 0, 2, 22.0, 1e-10, C.byref(m)), "mfcc init")
    f = L.vv_dsp_stft_mfcc_device if mfcc else L.vv_dsp_stft_log_mel_device
    nf = sz()
    return (lambda: ok(L, f(h, m, sig.data_ptr(), n, nch, n, out.data_ptr(), fr * w, s, C.byref(nf)), "mel")), \
        nch * n * 4 + nch * fr * w * 4, (lambda: out.clone())


def case_c2c(L, s, n=1024, batch=65536, fwd=1):
    x, y = buf(("c2c", n, batch), lambda: (torch.complex(torch.rand(batch, n, device="cuda") - 0.5,
                                                         torch.rand(batch, n, device="cuda") - 0.5),
                                           torch.empty(batch, n, dtype=torch.complex64, device="cuda")))
    p = vp()
    ok(L, L.vv_dsp_fft_make_plan_many(n, 0, fwd, batch, C.byref(p)), "fft plan")
    return (lambda: ok(L, L.vv_dsp_fft_execute_device(p, x.data_ptr(), y.data_ptr(), s), "fft")), \
        2 * batch * n * 8, (lambda: y.clone())


def case_czt(L, s, n, m, batch):
    """batched chirp-z rows cpx[batch][n] -> cpx[batch][m] (above P = 4096: the element-wise chain)"""
    x, y = buf(("czt", n, m, batch), lambda: (torch.complex(torch.rand(batch, n, device="cuda") - 0.5,
                                                            torch.rand(batch, n, device="cuda") - 0.5),
                                              torch.empty(batch, m, dtype=torch.complex64, device="cuda")))
    L.vv_dsp_czt_plan_create.argtypes = [sz, sz, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(vp)]
    L.vv_dsp_czt_execute_device.argtypes = [vp, vp, C.c_int, sz, vp, vp]
    w = np.exp(-2j * np.pi * 0.13 / m)
    p = vp()
    ok(L, L.vv_dsp_czt_plan_create(n, m, w.real, w.imag, 1.0, 0.0, C.byref(p)), "czt plan")
    return (lambda: ok(L, L.vv_dsp_czt_execute_device(p, x.data_ptr(), 0, batch, y.data_ptr(), s), "czt")), \
        batch * (n + m) * 8, (lambda: y.clone())


def case_real(L, s, n, batch, kind):
    """batched R2C (kind 1: real[n] -> cpx[n/2+1]) or C2R (kind 2, 1/n scaled)"""
    h = n // 2 + 1
    if kind == 1:
        x, y = buf(("r2c", n, batch), lambda: (torch.rand(batch, n, device="cuda") - 0.5,
                                               torch.empty(batch, h, dtype=torch.complex64, device="cuda")))
    else:
        x, y = buf(("c2r", n, batch), lambda: (torch.complex(torch.rand(batch, h, device="cuda") - 0.5,
                                                             torch.rand(batch, h, device="cuda") - 0.5),
                                               torch.empty(batch, n, device="cuda")))
    p = vp()
    ok(L, L.vv_dsp_fft_make_plan_many(n, kind, 1 if kind == 1 else -1, batch, C.byref(p)), "fft plan")
    return (lambda: ok(L, L.vv_dsp_fft_execute_device(p, x.data_ptr(), y.data_ptr(), s), "fft")), \
        batch * (n * 4 + h * 8), (lambda: y.clone())


def case_hilbert(L, s, n=1024, batch=65536):
    """batched Hilbert analytic rows real[batch][n] -> cpx[batch][n] (12 B per point)"""
    x, z = buf(("hil", n, batch), lambda: (torch.rand(batch, n, device="cuda") - 0.5,
                                           torch.empty(batch, n, dtype=torch.complex64, device="cuda")))
    L.vv_dsp_hilbert_analytic_device.argtypes = [vp, sz, sz, vp, vp]
    return (lambda: ok(L, L.vv_dsp_hilbert_analytic_device(x.data_ptr(), n, batch, z.data_ptr(), s), "hilbert")), \
        batch * n * 12, (lambda: z.clone())


def case_dct(L, s, n=1024, batch=131072):
    """batched DCT-II forward rows (8 B per point)"""
    x, y = buf(("dct", n, batch), lambda: (torch.rand(batch, n, device="cuda") - 0.5,
                                           torch.empty(batch, n, device="cuda")))
    L.vv_dsp_dct_make_plan.argtypes = [sz, C.c_int, C.c_int, C.POINTER(vp)]
    L.vv_dsp_dct_execute_device.argtypes = [vp, vp, vp, sz, vp]
    p = vp()
    ok(L, L.vv_dsp_dct_make_plan(n, 2, 1, C.byref(p)), "dct plan")
    return (lambda: ok(L, L.vv_dsp_dct_execute_device(p, x.data_ptr(), y.data_ptr(), batch, s), "dct")), \
        batch * n * 8, (lambda: y.clone())


class PitchParams(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("sample_rate", "fmin", "fmax", "threshold")]


def case_frames(L, s, kind, frame, hop, arg, nch=32, n=600 * 16000, center=0, rows=False):
    """The per-frame features (kind lpc: arg = order; stats: arg = number of outputs, 7 =
    the energy set; pitch: arg = (fmin, fmax, with cmnd)) of a Hamming-windowed signal
    [nch][n] in one fused launch, or (rows) of nch * frames contiguous rows of `frame`
    samples through the row entry point.  Outputs compare as int32 (bit for bit)."""
    fr = (n + hop - 1) // hop if center else 1 + (n - frame) // hop
    b = nch * fr
    w = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(frame) / (frame - 1))).astype(np.float32)
    x, win = buf((kind, frame, hop, nch, n, rows), lambda: (
        torch.rand(b, frame, device="cuda") * 2 - 1 if rows else torch.rand(nch, n, device="cuda") * 2 - 1,
        torch.from_numpy(w).cuda()))
    head = (x.data_ptr(), n, nch, n, frame, hop, center, win.data_ptr())
    if kind == "lpc":
        out = buf(("lpc out", b, arg), lambda: torch.zeros(b * (arg + 2), device="cuda"))
        a, err = out.data_ptr(), out.data_ptr() + 4 * b * (arg + 1)
        L.vv_dsp_lpc_frames_device.argtypes = [vp, sz, sz, sz, sz, sz, C.c_int, vp, sz, vp, sz, vp, sz, vp]
        L.vv_dsp_lpc_device.argtypes = [vp, sz, sz, sz, vp, vp, vp]
        if rows:
            run = lambda: ok(L, L.vv_dsp_lpc_device(x.data_ptr(), frame, arg, b, a, err, s), "lpc")  # noqa: E731
        else:
            run = lambda: ok(L, L.vv_dsp_lpc_frames_device(*head, arg, a, fr * (arg + 1), err, fr, s), "lpc_frames")  # noqa: E731
    elif kind == "stats":
        out = buf(("stats out", b), lambda: torch.zeros(12, b, device="cuda"))
        energy = (3, 4, 5, 6, 9, 10, 11)   # rms min max crest zero_crossings argmin argmax
        so = (vp * 12)(*[out[k].data_ptr() if arg == 12 or k in energy else None for k in range(12)])
        L.vv_dsp_stats_frames_device.argtypes = [vp, sz, sz, sz, sz, sz, C.c_int, vp, vp, sz, vp]
        L.vv_dsp_stats_device.argtypes = [vp, sz, sz, sz, vp, vp]
        if rows:
            run = lambda: ok(L, L.vv_dsp_stats_device(x.data_ptr(), frame, b, frame, so, s), "stats")  # noqa: E731
        else:
            run = lambda: ok(L, L.vv_dsp_stats_frames_device(*head, so, fr, s), "stats_frames")  # noqa: E731
    else:
        fmin, fmax, cmnd = arg
        p = PitchParams(16000.0, fmin, fmax, 0.15)
        curve = int(np.ceil(16000.0 / fmin)) + 1
        out = buf(("pitch out", b, curve, cmnd), lambda: torch.zeros(b * (3 + (curve if cmnd else 0)), device="cuda"))
        po = (vp * 4)(*[out.data_ptr() + 4 * b * k for k in range(3)], out.data_ptr() + 12 * b if cmnd else None)
        L.vv_dsp_pitch_frames_device.argtypes = [vp, sz, sz, sz, sz, sz, C.c_int, vp, vp, vp, sz, sz, vp]
        L.vv_dsp_pitch_device.argtypes = [vp, sz, sz, sz, vp, vp, sz, vp]
        if rows:
            run = lambda: ok(L, L.vv_dsp_pitch_device(x.data_ptr(), frame, b, frame, C.byref(p), po, curve, s), "pitch")  # noqa: E731
        else:
            run = lambda: ok(L, L.vv_dsp_pitch_frames_device(*head, C.byref(p), po, fr, fr * curve, s), "pitch_frames")  # noqa: E731
    return run, 4 * x.numel(), (lambda: (out.view(torch.int32).clone(), out.zero_())[0])   # zeroed for the next build


def burst(case, k):
    """k launches back to back per timed call (the per-launch time is ms / k)"""
    fn, byts, get = case

    def run():
        for _ in range(k):
            fn()
    return run, byts * k, get


CASES = {
    "fir": case_fir,
    # the long-transform routes: two-pass four-step both ways, Bluestein, the chirp-z chain at P = 8192, long FIR
    **{f"c2c2p{lg}{d}": (lambda L, s, lg=lg, b=b, f=f: case_c2c(L, s, 1 << lg, b, f))
       for lg, b in ((16, 64), (20, 4)) for d, f in (("", 1), ("inv", -1))},
    "blue48000": lambda L, s: case_c2c(L, s, 48000, 8),
    "czt8192": lambda L, s: case_czt(L, s, 3000, 1200, 2048),
    "firlong": lambda L, s: case_fir(L, s, nch=8, n=1 << 22, taps=6200),
    "stft": lambda L, s: case_stft_rows(L, s, "mag", 32, 600),
    "stft60": lambda L, s: case_stft_rows(L, s, "mag", 1, 60),
    "stft256ch": lambda L, s: case_stft_rows(L, s, "mag", 256, 600),
    "stft60x10": lambda L, s: burst(case_stft_rows(L, s, "mag", 1, 60), 10),
    "stftpow": lambda L, s: case_stft_rows(L, s, "pow", 32, 600),
    "stftpow544": lambda L, s: case_stft_rows(L, s, "pow544", 32, 600),
    "logmel": lambda L, s: case_mel(L, s, False),
    "logmel8": lambda L, s: case_mel(L, s, False, nch=8),
    "mfcc": lambda L, s: case_mel(L, s, True),
    "c2c1024": case_c2c,
    **{f"c2c{n}": (lambda L, s, n=n: case_c2c(L, s, n, (1 << 26) // n)) for n in (16, 32, 64, 128, 256, 512, 2048, 4096, 8192)},
    **{f"r2c{n}": (lambda L, s, n=n: case_real(L, s, n, (1 << 27) // n, 1)) for n in (16, 32, 64, 128, 256, 400, 480, 960, 1000, 1024, 2000, 2048, 4096, 8192, 16384)},
    **{f"c2r{n}": (lambda L, s, n=n: case_real(L, s, n, (1 << 27) // n, 2)) for n in (16, 32, 64, 128, 256, 1024, 2048, 4096, 8192, 16384)},
    **{f"hilbert{n}": (lambda L, s, n=n: case_hilbert(L, s, n, (1 << 26) // n)) for n in (16, 32, 64, 128, 256, 1024, 2048, 4096, 8192)},
    **{f"dct{n}": (lambda L, s, n=n: case_dct(L, s, n, (1 << 27) // n)) for n in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192)},
    **{f"c2c{n}": (lambda L, s, n=n: case_c2c(L, s, n, (1 << 26) // n)) for n in (320, 400, 441, 480, 600, 640, 720, 800, 900, 960, 1000, 2000, 3000, 4000)},
    **{f"stft{n}": (lambda L, s, n=n: case_stft_nfft(L, s, n, n // 4)) for n in (64, 128, 256, 400, 480, 512, 600, 960, 1000, 1024, 2048, 4096)},
    **{f"stftc{n}": (lambda L, s, n=n: case_stft_cpx(L, s, n, n // 4))
       for n in (256, 400, 512, 900, 960, 1024, 2000, 2048, 4096)},
    # power rows at the mixed-radix lengths (register kernel; 1000: the plan kernel)
    **{f"stftp{n}": (lambda L, s, n=n: case_stft_nfft(L, s, n, n // 4, power=True)) for n in (400, 960, 1000)},
    # per-frame features: the workloads of lpcbench.py, statsbench.py and pitchbench.py, the row entry
    # points, and one centred shape whose frames leave both ends of the signal
    "lpc16k": lambda L, s: case_frames(L, s, "lpc", 400, 160, 16),
    "lpc48k": lambda L, s: case_frames(L, s, "lpc", 1200, 480, 32, n=600 * 48000),
    "statsenergy": lambda L, s: case_frames(L, s, "stats", 400, 160, 7),
    "statsfull": lambda L, s: case_frames(L, s, "stats", 400, 160, 12),
    "pitch400": lambda L, s: case_frames(L, s, "pitch", 400, 160, (100.0, 400.0, False)),
    "pitch1024": lambda L, s: case_frames(L, s, "pitch", 1024, 256, (60.0, 500.0, False)),
    **{k + "rows": (lambda L, s, k=k, a=a: case_frames(L, s, k, 400, 160, a, nch=8, rows=True))
       for k, a in (("lpc", 16), ("stats", 12), ("pitch", (100.0, 400.0, False)))},
    **{k + "edge": (lambda L, s, k=k, a=a: case_frames(L, s, k, 400, 160, a, nch=3, n=1000, center=1))
       for k, a in (("lpc", 16), ("stats", 12), ("pitch", (100.0, 400.0, True)))},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--cases", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--check", action="store_true", help="also compare each build's output with the first's")
    a = ap.parse_args()
    libs = [load(p) for p in a.libs.split(",")]
    tags = [os.path.basename(p) for p in a.libs.split(",")]
    if len(set(p.partition("@")[0] for p in a.libs.split(","))) != len(tags):
        raise SystemExit("each build must be a distinct file (copy the .so to compare knob settings)")
    torch.cuda.init()
    s = torch.cuda.current_stream()
    sp = s.cuda_stream
    for case in a.cases.split(","):
        built = [CASES[case](L, sp) for L in libs]
        res = [[] for _ in libs]
        same = []
        if a.check:
            outs = []
            for fn, _, get in built:
                fn()
                torch.cuda.synchronize()
                outs.append(get())
            same = [bool(torch.equal(outs[0], o)) for o in outs]
            del outs
        for _ in range(a.rounds):
            for i, (fn, _, _) in enumerate(built):
                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.05:
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
                for e0, e1 in ev:
                    e0.record(s)
                    fn()
                    e1.record(s)
                torch.cuda.synchronize()
                res[i] += [e0.elapsed_time(e1) for e0, e1 in ev]
        base = float(np.median(res[0]))
        for i, tag in enumerate(tags):
            med = float(np.median(res[i]))
            byts = built[i][1]
            line = {"case": case, "lib": tag, "ms_median": round(med, 4), "ms_min": round(float(np.min(res[i])), 4),
                    "frac": round(byts / (med * 1e-3) / 1e9 / PEAK, 4), "vs_first": round(med / base, 4)}
            if same:
                line["bit_identical_to_first"] = same[i]
            print(json.dumps(line), flush=True)
        del built
        _BUF.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
