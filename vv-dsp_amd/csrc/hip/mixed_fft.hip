// mixed_fft.hip -- batched mixed-radix FFT for 7-smooth lengths that are not
// powers of two (n = 2^a 3^b 5^c 7^d, n >= 6) on gfx950: the plans and the
// router to the kernel families.
//
// The reference runs every non-power-of-two length through its O(n^2) DFT
// (src/spectral/fft_kiss.c:76-92, dispatched at :114-116, and for all C2R).
// The common audio lengths are 7-smooth (STFT frames of 400, 480, 960 or 2000
// samples; 44100 = 2^2 3^2 5^2 7^2), so these kernels replace that O(n^2) work
// with a Stockham autosort FFT whose radices are read from a per-length plan:
//   n <= 4096             the LDS plan kernel k_fft_mixed (mixed_plan.hip), or for
//                         the ten common frame lengths 320..960 the two-pass
//                         register kernel k_stft_sq (sq_kernel.hpp: sq_rows.hip,
//                         sq_stft.hip)
//   n = N1 x N2 <= 4096^2 the four-step k_fft_mixed_fs (mixed_fourstep.hip)
#include "mixed_common.hpp"

namespace vvh {

bool make_plan(long long n, MixedPlan* pl) {
    if (n < 2 || n > MIX_MAXN) return false;
    int m = (int)n, np = 0;
    int rad[32];
    while (m % 8 == 0) { rad[np++] = 8; m /= 8; }
    if (m % 4 == 0) { rad[np++] = 4; m /= 4; }
    if (m % 2 == 0) { rad[np++] = 2; m /= 2; }
    for (int p : {7, 5, 3})
        while (m % p == 0) { rad[np++] = p; m /= p; }
    if (m != 1 || np > MIX_MAXP) return false;
    pl->n = (int)n;
    pl->np = np;
    int ns = 1;
    for (int p = 0; p < np; ++p) {
        pl->radix[p] = rad[p];
        pl->ns[p] = ns;
        pl->tstep[p] = (int)n / (ns * rad[p]);
        pl->rns[p] = 1.0f / (float)ns;
        ns *= rad[p];
    }
    return true;
}

int mixed_threads(long long n) { return n <= 256 ? 16 : n <= 512 ? 32 : n <= 1024 ? 64 : 256; }

bool mixed_supported(long long n) {
    if ((n & (n - 1)) == 0) return false;
    MixedPlan pl;
    int n1, n2;
    return make_plan(n, &pl) || fs_split(n, &n1, &n2);
}

// the fused STFT (launch_stft_mixed) needs a single-pass plan: n <= MIX_MAXN.
// Larger smooth nfft take the generic gather + FFT path (which uses the four-step).
bool stft_mixed_supported(long long n) {
    if ((n & (n - 1)) == 0) return false;
    MixedPlan pl;
    return make_plan(n, &pl);
}

hipError_t launch_fft_mixed(long long n, int fwd, const void* in, int real_in, float2* out, long long nout,
                            long long batch, long long in_dist, long long out_dist, float scale, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    MixedPlan pl;
    if (!make_plan(n, &pl))
        return launch_fft_mixed_fs(n, fwd, in, real_in, out, nout, batch, in_dist, out_dist, scale, s);
    MixIO io{};
    io.in = in;
    io.out = out;
    io.nout = nout;
    io.in_dist = in_dist;
    io.out_dist = out_dist;
    io.scale = scale;
    io.isign = fwd ? 1.0f : -1.0f;
    hipError_t e = hipSuccess;
    // Real rows are not paired across the batch (unlike STFT frames), so a row's
    // result does not depend on the batch it came in.  Even n with a plannable
    // n/2 (forward, the R2C case): the n/2-point transform of the row's
    // even/odd pairs and the split step (MODE 5, half the FFT work); otherwise
    // the row with imaginary part zero (MODE 4).
    if (real_in) {
        MixedPlan ph;
        // knob MIX_R2C_FULL = 1: MODE 4 for even n too (A/B)
        const bool half = fwd && n % 2 == 0 && nout <= n / 2 + 1 && knob(KNOB_MIX_R2C_FULL, 0) != 1 && make_plan(n / 2, &ph);
        if (!half) return run_mixed(4, pl, io, batch, s);
        io.twn = twiddle_table((int)n);
        if (!io.twn) return hipErrorOutOfMemory;
        return sq_r2c(n, io, batch, s, &e) ? e : run_mixed(5, ph, io, batch, s);
    }
    return sq_c2c(n, io, batch, s, &e) ? e : run_mixed(0, pl, io, batch, s);
}

hipError_t launch_stft_mixed(long long nfft, long long hop, int kind, const float* sig, long long n, long long nch,
                             long long ch_stride, long long frames, const float* win, void* out,
                             long long out_ch_stride, hipStream_t s) {
    MixedPlan pl;
    if (!make_plan(nfft, &pl) || kind < 0 || kind > 2) return hipErrorInvalidValue;
    const long long ppc = (frames + 1) / 2;
    const long long batch = nch * ppc;
    if (batch <= 0) return hipSuccess;
    MixIO io{};
    io.in = sig;
    io.out = reinterpret_cast<float2*>(out);
    io.sig_n = n;
    io.ch_stride = ch_stride;
    io.frames = frames;
    io.ppc = ppc;
    io.hop = hop;
    io.out_ch_stride = out_ch_stride;
    io.win = win;
    io.a16 = ((uintptr_t)out & 15) == 0 && (out_ch_stride & 3) == 0;
    // speech lengths: the two-pass register kernel; else MODE 1 / 2 / 3 of the plan kernel
    hipError_t e = hipSuccess;
    return sq_stft(nfft, kind, io, batch, s, &e) ? e : run_mixed(1 + kind, pl, io, batch, s);
}

}  // namespace vvh
