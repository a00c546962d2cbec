// formant_kernels.hip -- the poles of 1/A(z) of LPC rows as formants for gfx950,
// as include/vv_dsp/features/formant.h defines them: Aberth-Ehrlich in IEEE f64,
// every operation in the header's order, nothing fused.
//
// One lane per root.  A row takes a group of W = 8, 16 or 32 lanes (the smallest
// that holds its order), so a wave iterates 8, 4 or 2 rows side by side.  Lane i
// of a group holds z_i and a[i+1]; Horner reads a[m] and the sum over the other
// roots reads z_j as group broadcasts, j ascending, which is the header's order.
// A group that has converged, failed or run out keeps its iterate while the
// wave goes on for the others (its lanes still serve the cross-lane reads of
// nothing but their own group), so no row depends on its neighbours.  The
// candidates are ranked by counting, inside the group, the kept candidates
// that sort before each one.
#include "vvhip_internal.hpp"
#include "../../../include/vv_dsp/features/formant.h"

#pragma clang fp contract(off)

namespace vvh {

namespace {

struct Cpx {
    double re, im;
};
__device__ __forceinline__ Cpx cmul(Cpx a, Cpx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Cpx cdiv(Cpx x, Cpx u) {
    const double n = u.re * u.re + u.im * u.im;
    return {(x.re * u.re + x.im * u.im) / n, (x.im * u.re - x.re * u.im) / n};
}

template <int W>
__global__ void __launch_bounds__(256)
k_formants(const float* __restrict__ a, int p, long long rows, long long a_pitch, FormantCfg cfg, FormantOut out) {
    constexpr int RPW = 64 / W;   // rows per wave
    const int lane = threadIdx.x & 63, sub = lane / W, i = lane % W;
    const long long row = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + sub;
    const bool valid = row < rows, active = valid && i < p;
    const unsigned long long gmask = (W == 64 ? ~0ull : ((1ull << W) - 1ull)) << (sub * W);
    const double am = active ? (double)a[row * a_pitch + i + 1] : 0.0;   // lane i holds a[i+1]
    const bool silent = (__ballot(am != 0.0) & gmask) == 0ull;

    Cpx z = {cfg.start[2 * i], cfg.start[2 * i + 1]};   // i < 32 = LSF_MAX_ORDER
    bool done = !valid || silent, converged = valid && silent, failed = false;
    for (int it = 0; it < VV_DSP_FORMANT_MAX_ITER; ++it) {
        if (__ballot(!done) == 0ull) break;
        Cpx b = {1.0, 0.0}, d = {0.0, 0.0};
        for (int m = 1; m <= p; ++m) {
            const double amb = __shfl(am, m - 1, W);
            const Cpx dz = cmul(d, z);
            d = {dz.re + b.re, dz.im + b.im};
            b = cmul(b, z);
            b.re = b.re + amb;
        }
        const Cpx w = cdiv(b, d);
        Cpx s = {0.0, 0.0};
        for (int j = 0; j < p; ++j) {
            const Cpx zj = {__shfl(z.re, j, W), __shfl(z.im, j, W)};
            if (j != i) {
                const Cpx r = cdiv(Cpx{1.0, 0.0}, Cpx{z.re - zj.re, z.im - zj.im});
                s = {s.re + r.re, s.im + r.im};
            }
        }
        const Cpx t = cmul(w, s);
        const Cpx dl = cdiv(w, Cpx{1.0 - t.re, -t.im});
        const bool bad = active && !(isfinite(dl.re) && isfinite(dl.im));
        const bool small = !active || dl.re * dl.re + dl.im * dl.im < 1e-26;
        const bool anybad = (__ballot(bad) & gmask) != 0ull;
        const bool allsmall = (__ballot(small) & gmask) == gmask;
        if (!done) {
            z = {z.re - dl.re, z.im - dl.im};
            if (anybad) failed = done = true;
            else if (allsmall) converged = done = true;
        }
    }

    // candidates of a converged row that was iterated
    const double c = cfg.sample_rate / 6.283185307179586;
    const double f = atan2(z.im, z.re) * c;
    const double r2 = z.re * z.re + z.im * z.im;
    const double bw = -(log(r2) * c);
    const bool kept = active && converged && !silent && z.im > 0.0 && f >= cfg.f_min && f <= cfg.f_max && bw > 0.0 &&
                      bw <= cfg.bw_max;
    int rank = 0;
    for (int j = 0; j < p; ++j) {
        const double fj = __shfl(f, j, W);
        const int kj = __shfl((int)kept, j, W);
        if (kj && (fj < f || (fj == f && j < i))) ++rank;
    }
    const int nf = cfg.n_formants;
    const int nkept = __popcll(__ballot(kept) & gmask);
    const int count = nkept < nf ? nkept : nf;
    if (!valid) return;
    const float qn = __uint_as_float(0x7FC00000u);
    if (kept && rank < nf) {
        if (out.freq) out.freq[row * nf + rank] = (float)f;
        if (out.bw) out.bw[row * nf + rank] = (float)bw;
    }
    for (int e = i; e < nf; e += W)
        if (e >= count) {
            if (out.freq) out.freq[row * nf + e] = qn;
            if (out.bw) out.bw[row * nf + e] = qn;
        }
    if (i == 0) {
        if (out.count) out.count[row] = count;
        if (out.flags) out.flags[row] = converged ? VV_DSP_FORMANT_CONVERGED : 0;
    }
    if (out.roots && active) {
        const double qd = __longlong_as_double(0x7FF8000000000000ll);
        double* r = out.roots + (row * p + i) * 2;
        r[0] = failed ? qd : z.re;
        r[1] = failed ? qd : z.im;
    }
}

template <int W>
hipError_t launch_w(const float* a, int order, long long rows, long long a_pitch, const FormantCfg& cfg,
                    const FormantOut& out, hipStream_t s) {
    const long long per_block = 4 * (64 / W);
    const unsigned grid = (unsigned)((rows + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_formants<W>, dim3(grid), dim3(256), 0, s, a, order, rows, a_pitch, cfg, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_formants(const float* a, int order, long long rows, long long a_pitch, const FormantCfg& cfg,
                           const FormantOut& out, hipStream_t s) {
    if (order <= 8) return launch_w<8>(a, order, rows, a_pitch, cfg, out, s);
    if (order <= 16) return launch_w<16>(a, order, rows, a_pitch, cfg, out, s);
    return launch_w<32>(a, order, rows, a_pitch, cfg, out, s);
}

}  // namespace vvh
