#!/usr/bin/env python3
"""One tiny call per mixed-radix launch route, for a kernel trace (not a test, not a timing tool).

The sibling of stft_routes.py and fir_routes.py for mixed_fft.hip's router: the
register kernel (sq_rows.hip, sq_stft.hip), the plan kernel (mixed_plan.hip) and
the four-step (mixed_fourstep.hip).  Every call prints its shape before and a
bit-level checksum of the output after, so that two builds can be compared by
the kernels they launch:

    rocprofv3 --kernel-trace -d out_a -- python scripts/mixed_routes.py          # this build
    VVDSP_AMD_LIB=/path/to/other/libvvdsp_amd.so rocprofv3 --kernel-trace -d out_b -- python scripts/mixed_routes.py

(kernel tracing alone: no counters, no other tracing).  The sequences of kernel
names, and the printed lines, must be equal.
"""
import torch

from stft_routes import KINDS, bits, signal, vv

REGISTER = (320, 400, 441, 480, 600, 640, 720, 800, 900, 960)
PLAN = (100, 500, 1000, 3000)   # one length per thread count of the plan kernel (16, 32, 64, 256)


def run_stft(tag, nfft, nch, frames, kind, unaligned=False, **knobs):
    """`frames` frames per channel at hop nfft / 4, the last one running past the end"""
    hop = nfft // 4
    st = vv.Stft(nfft, hop)
    n = nfft + (frames - 1) * hop - hop // 2
    assert st.frames(n) == frames
    sig = signal(nch, n)
    print("%-10s nfft %5d hop %4d %-9s sig %s%s%s" % (
        tag, nfft, hop, kind, tuple(sig.shape), " out 4 B past 16 B" if unaligned else "",
        "".join(" %s=%d" % kv for kv in knobs.items())), flush=True)
    with vv.knobs(**knobs):
        if kind == "power":
            out = st.power(sig)
        elif unaligned:   # magnitude rows
            out = torch.zeros(nch * frames * nfft + 1, device="cuda")[1:].view(nch, frames, nfft)
            st.spectrogram(sig, out=out)
        else:
            out = st.spectrogram(sig, complex_out=kind == "complex")
        torch.cuda.synchronize()
    print("    rows %s bits %d" % (tuple(out.shape), bits(out)), flush=True)


def run_fft(tag, n, batch, kind, **knobs):
    """kind c2c / c2c-inv / r2c on `batch` rows"""
    if kind == "r2c":
        x = signal(batch, n)
        plan = vv.FftPlan(n, vv.R2C, vv.FWD, batch=batch)
    else:
        x = torch.complex(signal(batch, n), signal(batch, n))
        plan = vv.FftPlan(n, vv.C2C, vv.BWD if kind == "c2c-inv" else vv.FWD, batch=batch)
    print("%-10s n %6d %-7s rows %d%s" % (tag, n, kind, batch, "".join(" %s=%d" % kv for kv in knobs.items())),
          flush=True)
    with vv.knobs(**knobs):
        y = plan(x)
        torch.cuda.synchronize()
    print("    out %s bits %d" % (tuple(y.shape), bits(y)), flush=True)


def main():
    # (a) the register kernel's STFT rows: every length and row kind, 2 channels x 5
    # frames (a tail pair without a second frame, the last frame past the end); the
    # staged flush once from an output that is not 16 B aligned
    for nfft in REGISTER:
        for kind in KINDS:
            run_stft("a-sq", nfft, 2, 5, kind)
    run_stft("a-unalign", 400, 2, 5, "magnitude", unaligned=True)
    # (b) the register kernel's rows: c2c both ways and R2C (whose half length it is)
    for n in REGISTER:
        run_fft("b-sq", n, 9, "c2c")
        run_fft("b-sq", n, 9, "c2c-inv")
    for n in (400, 480) + tuple(2 * m for m in REGISTER):
        run_fft("b-sq", n, 9, "r2c")
    # (c) the plan kernel at each thread count: c2c, real rows (even: the half
    # transform + split step; odd, and even under MIX_R2C_FULL: the full row),
    # the three STFT kinds; STFT_SQ=0 sends a register length through it
    for n in PLAN:
        run_fft("c-plan", n, 9, "c2c")
        run_fft("c-plan", n, 9, "c2c-inv")
        run_fft("c-plan", n, 9, "r2c")
        run_fft("c-plan", n, 9, "r2c", MIX_R2C_FULL=1)
        for kind in KINDS:
            run_stft("c-plan", n, 2, 5, kind)
    for n in (45, 441, 3125):
        run_fft("c-plan", n, 9, "r2c")
    for kind in KINDS:
        run_stft("c-plan", 400, 2, 5, kind, STFT_SQ=0)
    run_fft("c-plan", 400, 9, "c2c", STFT_SQ=0)
    run_fft("c-plan", 400, 9, "r2c", STFT_SQ=0)
    # (d) the four-step, complex and real, once in chunks of 1 MB
    for n in (4800, 44100):
        run_fft("d-fs", n, 3, "c2c")
        run_fft("d-fs", n, 3, "c2c-inv")
        run_fft("d-fs", n, 3, "r2c")
    run_fft("d-fs", 44100, 3, "c2c", MIX_CHUNK_MB=1)
    # (e) the grid knob: persistent and non-persistent, register and plan kernel
    for tpw in (0, 1):
        run_fft("e-grid", 400, 300, "c2c", MIX_TPW=tpw)
        run_fft("e-grid", 1000, 300, "c2c", MIX_TPW=tpw)
        run_stft("e-grid", 400, 2, 5, "magnitude", MIX_TPW=tpw)


if __name__ == "__main__":
    main()
