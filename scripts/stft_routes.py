#!/usr/bin/env python3
"""One tiny call per STFT launch route, for a kernel trace (not a test, not a timing tool).

Several tests compare "knob = 0" with the default bit for bit and would still
pass if a router never took its fast path.  This runs one fixed list of calls
once each, printing the shape before the call and a bit-level checksum of the
rows after it, so that two builds can be compared by the kernels they launch:

    rocprofv3 --kernel-trace -d out_a -- python scripts/stft_routes.py          # this build
    VVDSP_AMD_LIB=/path/to/other/libvvdsp_amd.so rocprofv3 --kernel-trace -d out_b -- python scripts/stft_routes.py

(kernel tracing alone: no counters, no other tracing).  The sequences of kernel
names, and the printed lines, must be equal.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vv-dsp_amd"))
import vvdsp_amd as vv   # noqa: E402

KINDS = ("magnitude", "complex", "power")
GEN = torch.Generator(device="cuda").manual_seed(7)


def signal(nch, n, offset=0):
    """(nch, n) contiguous rows (the channel stride is n) starting `offset` floats
    past a 256 B aligned allocation"""
    base = torch.rand(offset + nch * n, device="cuda", generator=GEN) * 2 - 1
    return base[offset:].view(nch, n)


def nine_frames(nfft, hop, odd):
    """a signal length with 9 frames (the last one zero-padded when hop > 1):
    a multiple of 4, or odd, where the range has one"""
    lens = range(nfft + 7 * hop, nfft + 8 * hop)
    fit = [n for n in lens if (n % 2 == 1 if odd else n % 4 == 0)]
    return fit[len(fit) // 2] if fit else lens[-1]


def bits(t):
    return int(torch.view_as_real(t).contiguous().view(torch.int32).sum(dtype=torch.int64)) if t.is_complex() \
        else int(t.contiguous().view(torch.int32).sum(dtype=torch.int64))


def run(tag, st, sig, kind, pitch=None, **knobs):
    print("%-10s nfft %5d hop %4d %-9s sig %s stride %d align %d%s%s" % (
        tag, st.nfft, st.hop, kind, tuple(sig.shape), sig.stride(0), sig.data_ptr() % 16,
        " pitch %d" % pitch if pitch else "", "".join(" %s=%d" % kv for kv in knobs.items())), flush=True)
    with vv.knobs(**knobs):
        if kind == "power":
            out = st.power(sig, pitch=pitch)
            if pitch:
                out = out[..., :st.nfft // 2 + 1]
        else:
            out = st.spectrogram(sig, complex_out=kind == "complex")
        torch.cuda.synchronize()
    print("    rows %s bits %d" % (tuple(out.shape), bits(out)), flush=True)


def run_mel(tag, mf, st, sig, log_mel, **knobs):
    print("%-10s nfft %5d hop %4d %-9s sig %s stride %d%s" % (
        tag, st.nfft, st.hop, "log-mel" if log_mel else "mfcc", tuple(sig.shape), sig.stride(0),
        "".join(" %s=%d" % kv for kv in knobs.items())), flush=True)
    with vv.knobs(**knobs):
        out = mf.from_signal(st, sig, log_mel=log_mel)
        torch.cuda.synchronize()
    print("    rows %s bits %d" % (tuple(out.shape), bits(out)), flush=True)


def main():
    # (a) every size and row kind: 2 channels x 9 frames (a tail pair without a second
    # frame; the last frame zero-padded), (b) the same from an unaligned start and with
    # an odd channel stride (an odd length: the rows are contiguous)
    for nfft in [2 ** k for k in range(1, 14)]:
        hop = max(nfft // 4, 1)
        st = vv.Stft(nfft, hop)
        n, n_odd = nine_frames(nfft, hop, False), nine_frames(nfft, hop, True)
        assert st.frames(n) == 9 and st.frames(n_odd) == 9
        for kind in KINDS:
            run("a", st, signal(2, n), kind)
            run("b-offset", st, signal(2, n, offset=1), kind)
            run("b-stride", st, signal(2, n_odd), kind)
    # (c) nfft 1024 at hop 256 and hop 200; power rows 544 floats apart
    for hop in (256, 200):
        st = vv.Stft(1024, hop)
        for kind in KINDS:
            run("c", st, signal(3, 1024 + 20 * hop + 40), kind)
    st1024 = vv.Stft(1024, 256)
    run("c-pitch", st1024, signal(3, 1024 + 20 * 256 + 40), "power", pitch=544)
    # (d) the small sizes' routes: the staged kernel (hop 64), not staged (hop 128), one pair per slot (4096)
    for hop in (64, 128):
        run("d", vv.Stft(256, hop), signal(3, 256 + 40 * hop), "magnitude")
    run("d", vv.Stft(4096, 1024), signal(3, 4096 + 11 * 1024), "magnitude")
    # (e) fused log-mel / MFCC with a small plan, the 32 x 32 split of every row kind that has one
    mf = vv.Mfcc(1024, 40, 13, 48000.0, 20.0, 20000.0, lifter=22.0)
    sig = signal(3, 1024 + 20 * 256 + 40)
    for log_mel in (True, False):
        run_mel("e", mf, st1024, sig, log_mel)
        run_mel("e-r32", mf, st1024, sig, log_mel, POW_R32=1, MEL_R32=1)
    run("e-r32", st1024, sig, "power", POW_R32=1)
    run("e-r32", st1024, sig, "magnitude", MAG_R32=1)
    # (f) the dynamic walk: pairs >= 16 * F * cap with F = 4 slots and cap <= 4 x 256
    # resident workgroups -- 2 x 35,001 pairs, an odd frame count, a zero-padded tail
    frames = 70001
    big = signal(2, 1024 + (frames - 2) * 256 + 80)
    assert st1024.frames(big.shape[1]) == frames
    for kind in KINDS:
        d0 = vv.debug_get("STAT_STFT_DYN")
        run("f", st1024, big, kind)
        print("    STAT_STFT_DYN +%d" % (vv.debug_get("STAT_STFT_DYN") - d0))
    run("f", st1024, big, "power", STFT_DYN=1)
    for log_mel in (True, False):
        run_mel("f", mf, st1024, big, log_mel)


if __name__ == "__main__":
    main()
