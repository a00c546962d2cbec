#!/usr/bin/env python3
"""One tiny call per long-transform launch route, for a kernel trace (not a test, not a timing tool).

The sibling of fft_routes.py for the launchers of fourstep_fft.hip,
bluestein.hip, chirp_glue.hip, czt_kernels.hip, ceps_stages.hip and
fir_long.hip: the two-pass four-step kernels at their three geometries under
every variant, the chunked chain, the five-pass path, Bluestein, the chirp-z
transform and the cepstrum family fused and as chains, and one long FIR.  Every
call prints its shape before and a bit-level checksum of the output after, so
that two builds can be compared by the kernels they launch:

    rocprofv3 --kernel-trace -d out_a -- python scripts/long_routes.py          # this build
    VVDSP_AMD_LIB=/path/to/other/libvvdsp_amd.so rocprofv3 --kernel-trace -d out_b -- python scripts/long_routes.py

(kernel tracing alone: no counters, no other tracing).  The sequences of kernel
names, and the printed lines, must be equal.
"""
import cmath

import torch

from fft_routes import BATCH, done, run_fft, show
from fir_routes import lowpass, run as run_fir
from stft_routes import signal, vv

# n and the knob that keeps 8192 out of the one-workgroup kernel: N1 = 64, N1 = N2 = 128, N1 != N2
GEOMETRIES = ((8192, {"C2C_MAX": 4096}), (16384, {}), (32768, {}))


def run_czt(tag, n, m, real, **knobs):
    x = signal(BATCH, n) if real else torch.view_as_complex(signal(BATCH, 2 * n).view(BATCH, n, 2))
    plan = vv.CztPlan(n, m, cmath.exp(-2j * cmath.pi * 0.13 / m), cmath.exp(0.2j))
    show(tag, n, "czt-real" if real else "czt-cpx", " m %d" % m, knobs)
    with vv.knobs(**knobs):
        done(plan(x))


def run_ceps(tag, n, **knobs):
    x = signal(BATCH, n)
    c = (0.1 * signal(BATCH, n)).contiguous()
    for kind, f, arg in (("cepstrum", vv.cepstrum, x), ("icepstrum", vv.icepstrum_minphase, c),
                         ("minphase", vv.minphase_from_cepstrum, c)):
        show(tag, n, kind, "", knobs)
        with vv.knobs(**knobs):
            done(f(arg))


def main():
    # (a) two-pass four-step: geometries x variants x directions, then 17 rows in chunks of
    # 1 MiB (16 + 1, 8 + 8 + 1 and 4 x 4 + 1 transforms: full chunks past the first, and a last one of one)
    for n, route in GEOMETRIES:
        for kind in ("c2c", "c2c-inv"):
            for var in range(4):
                run_fft("a-twopass", n, kind, FS_VAR=var, **route)
            run_fft("a-chunked", n, kind, batch=17, FS_CHUNK_MB=1, **route)
    # (b) the five-pass path: square and N1 != N2
    for n in (16384, 32768):
        for kind in ("c2c", "c2c-inv"):
            run_fft("b-fivepass", n, kind, FS_OLD=1)
    # (c) Bluestein (neither a power of two nor 7-smooth, M = 8192): the glue inside
    # the four-step passes, and as kernels of its own
    for kind in ("c2c", "c2c-inv", "r2c"):
        run_fft("c-blue", 3001, kind)
        run_fft("c-blue", 3001, kind, BLUE_UNFUSED=1)
    # (d) chirp-z: the one-pass kernel (P = 512), its chain, and the chain above it (P = 8192)
    for real in (False, True):
        run_czt("d-czt", 300, 200, real)
        run_czt("d-czt", 300, 200, real, CZT_UNFUSED=1)
        run_czt("d-czt", 3000, 1200, real)
    # (e) the cepstrum family: the one-pass kernels, their chains, and a length above them
    run_ceps("e-ceps", 1024)
    run_ceps("e-ceps", 1024, CEPS_UNFUSED=1)
    run_ceps("e-ceps", 8192)
    # (f) a zero-state filter beyond the fused kernels: gather, four-step FFTs, product, scatter
    run_fir("f-long", vv.FirPlan(lowpass(6200)), signal(2, 40000))


if __name__ == "__main__":
    main()
