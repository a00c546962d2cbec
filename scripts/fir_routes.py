#!/usr/bin/env python3
"""One tiny call per FIR launch route, for a kernel trace (not a test, not a timing tool).

The sibling of stft_routes.py: every call prints its shape before and a
bit-level checksum of the output after, so that two builds can be compared by
the kernels they launch:

    rocprofv3 --kernel-trace -d out_a -- python scripts/fir_routes.py          # this build
    VVDSP_AMD_LIB=/path/to/other/libvvdsp_amd.so rocprofv3 --kernel-trace -d out_b -- python scripts/fir_routes.py

(kernel tracing alone: no counters, no other tracing).  The sequences of kernel
names, and the printed lines, must be equal.
"""
import numpy as np
import torch

from stft_routes import bits, signal, vv

STATS = ("STAT_FIR_R32", "STAT_FIR_DYN", "STAT_FIR_STATIC")


def lowpass(taps):
    """windowed-sinc low-pass at a quarter of the sample rate (Hamming), f32"""
    k = np.arange(taps) - (taps - 1) / 2
    h = 0.5 * np.sinc(0.5 * k) * np.hamming(taps)
    return torch.from_numpy((h / h.sum()).astype(np.float32))


def run(tag, plan, x, call="ols", **knobs):
    print("%-10s taps %5d %-8s x %s stride %d align %d%s" % (
        tag, plan.taps, call, tuple(x.shape), x.stride(0), x.data_ptr() % 16,
        "".join(" %s=%d" % kv for kv in knobs.items())), flush=True)
    s0 = [vv.debug_get(s) for s in STATS]
    with vv.knobs(**knobs):
        y = plan.filtfilt(x) if call == "filtfilt" else plan(x, direct=call == "direct")
        torch.cuda.synchronize()
    print("    out %s bits %d%s" % (tuple(y.shape), bits(y), "".join(
        " %s +%d" % (s, vv.debug_get(s) - a) for s, a in zip(STATS, s0))), flush=True)


def main():
    # (a) overlap-save at every block size N: taps N/4 + 1 (le = N/4), 2 channels of
    # 2.5 blocks' outputs + 3 samples (a front edge pair and a tail pair with one block);
    # FIR_BLOCK keeps the plan from growing a small block toward 1024
    for N in [2 ** k for k in range(6, 14)]:
        run("a", vv.FirPlan(lowpass(N // 4 + 1)), signal(2, 5 * (3 * N // 4) // 2 + 3), FIR_BLOCK=N)
    # (b) N = 8192 with le = 3000 > N/4
    run("b", vv.FirPlan(lowpass(3001)), signal(2, 5 * (8192 - 3000) // 2 + 3))
    # (c) the 32 x 32 split (N = 1024): 8 B pairs, then dword loads from an allocation offset by one float
    p257 = vv.FirPlan(lowpass(257))
    run("c-paired", p257, signal(3, 3940))
    run("c-dword", p257, signal(3, 3940, offset=1))
    print("c-prefix   skipped: vv_dsp_fir_apply_fft_device takes no history (the binding's overlap-save is zero-state)")
    # (d) the 16 x 16 x 4 kernel: static walk, dynamic walk (>= 8 pairs per wave slot), every pair an edge pair
    run("d-static", p257, signal(3, 5_000_004), FIR_R32=0)
    run("d-dynamic", p257, signal(6, 9_000_004), FIR_R32=0)
    run("d-edges", p257, signal(5, 1540), FIR_R32=0)
    # (e) the LDS-DMA pair kernel plus the edge launch
    run("e-pair", p257, signal(3, 3940), FIR_R32=0, FIR_OLD=1)
    # (f) direct form and filtfilt, from registers and through LDS
    for taps in (17, 257):
        plan = vv.FirPlan(lowpass(taps))
        x = signal(3, 4097)
        for call in ("direct", "filtfilt"):
            run("f", plan, x, call)
            run("f-lds", plan, x, call, FIR_DIRECT_LDS=1)
    # (g) a zero-state filter beyond the fused kernels: gather, four-step FFTs, multiply, scatter
    run("g-long", vv.FirPlan(lowpass(6200)), signal(2, 40000))


if __name__ == "__main__":
    main()
