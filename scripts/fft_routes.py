#!/usr/bin/env python3
"""One tiny call per power-of-two FFT launch route, for a kernel trace (not a test, not a timing tool).

The sibling of stft_routes.py, fir_routes.py and mixed_routes.py for the
launchers of fft_c2c.hip, fft_real.hip, fft_glue.hip and analytic_kernels.hip:
C2C, R2C and C2R at every template geometry and under every grid knob, the
naive DFT, and the fused Hilbert and DCT-II rows.  Every call prints its shape
before and a bit-level checksum of the output after, so that two builds can be
compared by the kernels they launch:

    rocprofv3 --kernel-trace -d out_a -- python scripts/fft_routes.py          # this build
    VVDSP_AMD_LIB=/path/to/other/libvvdsp_amd.so rocprofv3 --kernel-trace -d out_b -- python scripts/fft_routes.py

(kernel tracing alone: no counters, no other tracing).  The sequences of kernel
names, and the printed lines, must be equal.
"""
import ctypes as C

import torch

from stft_routes import bits, signal, vv

C2C_SIZES = (2, 8, 16, 64, 128, 256, 512, 1024, 2048, 4096, 8192)
REAL_SIZES = (4, 16, 32, 128, 256, 1024, 4096, 16384, 32768)
ANALYTIC_SIZES = (8, 16, 128, 256, 1024, 4096)
BATCH = 9   # not a multiple of any kernel's slots per workgroup; an odd count of row pairs


def cpx(batch, n, offset=0):
    """(batch, n) complex rows starting `offset` float2 past a 256 B aligned allocation"""
    return torch.view_as_complex(signal(1, 2 * (offset + batch * n)).view(-1, 2))[offset:].view(batch, n)


def show(tag, n, kind, note, knobs, batch=BATCH):
    print("%-10s n %6d %-8s rows %d%s%s" % (tag, n, kind, batch, note, "".join(" %s=%d" % kv for kv in knobs.items())),
          flush=True)


def done(y):
    torch.cuda.synchronize()
    print("    out %s bits %d" % (tuple(y.shape), bits(y)), flush=True)


def run_fft(tag, n, kind, unaligned=False, batch=BATCH, **knobs):
    """kind c2c / c2c-inv / r2c / c2r; unaligned: the input 8 B past a 16 B boundary"""
    if kind == "r2c":
        x = signal(batch, n, offset=2 if unaligned else 0)
        plan = vv.FftPlan(n, vv.R2C, vv.FWD, batch=batch)
    elif kind == "c2r":
        x = cpx(batch, n // 2 + 1, offset=1 if unaligned else 0)
        plan = vv.FftPlan(n, vv.C2R, vv.BWD, batch=batch)
    else:
        x = cpx(batch, n, offset=1 if unaligned else 0)
        plan = vv.FftPlan(n, vv.C2C, vv.BWD if kind == "c2c-inv" else vv.FWD, batch=batch)
    show(tag, n, kind, " in 8 B past 16 B" if unaligned else "", knobs, batch)
    with vv.knobs(**knobs):
        done(plan(x))


def run_hilbert(tag, n, **knobs):
    x = signal(BATCH, n)
    show(tag, n, "hilbert", "", knobs)
    with vv.knobs(**knobs):
        done(vv.hilbert(x))


def run_dct(tag, n, policy=0, **knobs):
    """DCT-II rows under NaN policy 0 (propagate), 1 (zero) or 3 (clamp); a NaN and an Inf in the input"""
    x = signal(BATCH, n).clone()
    if policy:
        x[1, 0], x[2, n - 1] = float("nan"), float("inf")
    show(tag, n, "dct2", " policy %d" % policy, knobs)
    L = vv.lib()
    L.vv_dsp_set_nan_policy.argtypes = [C.c_int]
    L.vv_dsp_set_nan_policy.restype = None
    L.vv_dsp_set_nan_policy(policy)
    try:
        with vv.knobs(**knobs):
            done(vv.dct(x))
    finally:
        L.vv_dsp_set_nan_policy(0)


def main():
    # (a) C2C both ways: the default route, the looping kernel, the persistent grid,
    # three transforms per slot, the strided kernel at the staged lengths, an
    # unaligned buffer, and 8192 sent to the four-step
    for n in C2C_SIZES:
        for kind in ("c2c", "c2c-inv"):
            run_fft("a-c2c", n, kind)
            run_fft("a-c2c", n, kind, C2C_ONE=0)
            run_fft("a-c2c", n, kind, C2C_TPW=0)
            run_fft("a-c2c", n, kind, C2C_TPW=3)
            if n <= 128:
                run_fft("a-c2c", n, kind, C2C_SMALL=0)
            run_fft("a-c2c", n, kind, unaligned=True)
    run_fft("a-c2c", 8192, "c2c", C2C_MAX=4096)
    run_fft("a-c2c", 8192, "c2c-inv", C2C_MAX=4096)
    # (b) R2C and C2R: default, both grids, the strided kernels at the staged
    # lengths; 32768 (above the fused kernels: the split step around a C2C) also
    # through the promoted complex transform
    for n in REAL_SIZES:
        for kind in ("r2c", "c2r"):
            run_fft("b-real", n, kind)
            run_fft("b-real", n, kind, REAL_TPW=0)
            run_fft("b-real", n, kind, REAL_TPW=1)
            run_fft("b-real", n, kind, R2C_SMALL=0)
            run_fft("b-real", n, kind, REAL_SMALL=0)
    run_fft("b-real", 32768, "r2c", REAL_PROMOTE=1)
    run_fft("b-real", 32768, "c2r", REAL_PROMOTE=1)
    # (c) a length below 1025 that is neither a power of two nor 7-smooth: the naive DFT
    for kind in ("c2c", "c2c-inv", "r2c", "c2r"):
        run_fft("c-naive", 622, kind)
    # (d) fused Hilbert and DCT-II: default, the pair kernels at the staged lengths,
    # the non-persistent grid, and the DCT's NaN policies
    for n in ANALYTIC_SIZES:
        run_hilbert("d-hilbert", n)
        run_hilbert("d-hilbert", n, HIL_SMALL=0)
        run_hilbert("d-hilbert", n, ANA_TPW=1)
        for policy in (0, 1, 3):
            run_dct("d-dct", n, policy)
        run_dct("d-dct", n, DCT_SMALL=0)
        run_dct("d-dct", n, ANA_TPW=1)


if __name__ == "__main__":
    main()
