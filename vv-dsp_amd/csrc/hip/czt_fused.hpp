// czt_fused.hpp -- the chirp-z transform (src/spectral/czt.c:58-178; the stages:
// chirp_glue.hip) in one pass per row.  Launcher: czt_kernels.hip.
// The preamble (LDS, stage_twiddles, slot and t, the persistent row loop with its
// register prefetch) is the same text as k_ceps_fused (ceps_fused.hpp)'s: a device helper that
// returned the slot changed 19 of the 60 kernels of the unit (k_czt_fused<512, false>
// 2009 -> 2021 lines), so each kernel keeps the text ("The long-transform units").
#pragma once
#include "fft_core.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// k_czt_fused<P>: the whole chirp-z chain for P = next_pow2(N + M - 1) <= 4096
// in one pass per row: x * g on load, the P-point forward FFT in registers,
// the product with B / P re-indexed in registers (after the forward Stockham
// passes register q holds bin t + T*m, exactly the inverse transform's input
// set, as in the FIR overlap-save kernel), the inverse FFT, and W^(k^2/2) on
// the M outputs at positions N-1+k.  HBM traffic: the row in and the M outputs
// (plus the L2-resident g, B, post tables) instead of ~4 x 16 P bytes.
// Rows are walked grid-stride by a persistent grid, the next row's samples
// prefetched into registers during the current row's transforms.
// ------------------------------------------------------------------------
template <int P, bool REAL>
__global__ void __launch_bounds__(Wg<P>::value)
k_czt_fused(const void* __restrict__ x, long long n, long long m, long long rows, const float2* __restrict__ g,
            const float2* __restrict__ Bs, const float2* __restrict__ post, float2* __restrict__ X,
            const float2* gpass, const float2* gtab) {
    using G = Geo<P>;
    constexpr int WG = Wg<P>::value, F = Wg<P>::F;
    constexpr int LDSN = G::NPASS > 1 ? F * G::LDS : 1;
    __shared__ float2 lds[LDSN];
    __shared__ float2 ltab[TwLayout<P>::ENTRIES];
    stage_twiddles<P, WG>(ltab, gpass, gtab);
    __syncthreads();
    const TwTab<P> tw{ltab};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + (G::NPASS > 1 ? slot * G::LDS : 0);
    const long long stride = (long long)gridDim.x * F;
    long long f = uni<G::T>((long long)blockIdx.x * F + slot);
    float2 nx[G::P];
    auto load = [&](long long row) {
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            const long long e = t + r * G::T;
            float2 v = make_float2(0.0f, 0.0f);
            if (e < n) {
                if constexpr (REAL) v = make_float2(static_cast<const float*>(x)[row * n + e], 0.0f);
                else v = static_cast<const float2*>(x)[row * n + e];
            }
            nx[r] = v;
        }
    };
    if (f < rows) load(f);
    for (; f < rows; f += stride) {
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            const long long e = t + r * G::T;
            v[r] = e < n ? cmul(nx[r], g[e]) : make_float2(0.0f, 0.0f);
        }
        if (f + stride < rows) load(f + stride);
        fft_regs<P, true>(v, t, my, tw);
        float2 u[G::P];
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            const int mm = q / G::RL + G::NPT * (q % G::RL);   // out_pos<P>(t, q) = t + T*mm
            u[mm] = cmul(v[q], Bs[t + G::T * mm]);
        }
        fft_regs<P, false>(u, t, my, tw);
        float2* dst = X + f * m;
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            const long long k = (long long)out_pos<P>(t, q) - (n - 1);
            if (k >= 0 && k < m) dst[k] = cmul(u[q], post[k]);
        }
    }
}

}  // namespace vvh
