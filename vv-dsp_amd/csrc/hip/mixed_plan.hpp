// mixed_plan.hpp -- the Stockham passes of a runtime radix plan on an
// LDS-resident transform, for the two kernels that run one: k_fft_mixed
// (mixed_plan.hip) and k_fft_mixed_fs (mixed_fourstep.hip).
//
//   pass p, radix R, Ns = product of the earlier radices, butterfly j < n/R:
//     inputs   j + r*n/R                        (r < R)
//     twiddle  W_{Ns*R}^{(j mod Ns)*r} = W_n^{r*(j mod Ns)*n/(Ns*R)}
//     outputs  (j div Ns)*Ns*R + (j mod Ns) + r*Ns
//
// One transform lives in LDS (n float2) and is owned by T threads, each holding
// at most 16 points per pass in VGPRs: a pass reads all of a thread's
// butterflies, synchronises, and writes them back in place.  The W_n table
// (rounded once from double on the host, tables.hip) is staged in LDS with the
// transforms.  Radix-2/4/8 butterflies are the exact in-register DFTs of
// fft_core.hpp; radix 3/5/7 use the symmetric-pair form with constants written
// to 20 digits.
#pragma once
#include "mixed_common.hpp"

namespace vvh {

constexpr int MIX_PTS = 16;     // points per thread per pass at most

// One middle Stockham pass of radix R on the LDS-resident transform `buf`.
template <int R, int T>
__device__ __forceinline__ void mpass(float2* buf, const float2* tab, int t, int n, int Ns, int tstep, float rns,
                                      bool act) {
    constexpr int MAXB = (MIX_PTS + R - 1) / R;
    const int nb = n / R;
    float2 v[MAXB][R];
    if (act) {
#pragma unroll
        for (int b = 0; b < MAXB; ++b) {
            const int j = t + b * T;
            if (j < nb) {
#pragma unroll
                for (int r = 0; r < R; ++r) v[b][r] = buf[j + r * nb];
            }
        }
    }
    xsync<T>();
    if (act) {
#pragma unroll
        for (int b = 0; b < MAXB; ++b) {
            const int j = t + b * T;
            if (j < nb) {
                int q = (int)((float)j * rns);
                int k = j - q * Ns;
                if (k >= Ns) { k -= Ns; ++q; }
                else if (k < 0) { k += Ns; --q; }
                if (Ns > 1) {
                    const int kt = k * tstep;
#pragma unroll
                    for (int r = 1; r < R; ++r) v[b][r] = cmul(v[b][r], tab[r * kt]);
                }
                dft_fwd<R>(v[b]);
                float2* dst = buf + q * Ns * R + k;
#pragma unroll
                for (int r = 0; r < R; ++r) dst[r * Ns] = v[b][r];
            }
        }
    }
    xsync<T>();
}

// Every pass of plan `pl` on `buf`: one call site for all of them, so the radix
// switch is instantiated once per kernel.  A macro, expanded in the kernel's own
// loop nest: as a function taking the plan by reference it compiled to other
// code in every kernel (8 more VGPRs, about 40 more instructions).
#define VVH_MIX_RUN_PASSES(T, buf, tab, t, n, pl, act)                              \
    for (int p_ = 0; p_ < (pl).np; ++p_) {                                          \
        const int Ns_ = (pl).ns[p_], ts_ = (pl).tstep[p_];                          \
        const float rn_ = (pl).rns[p_];                                             \
        switch ((pl).radix[p_]) {                                                   \
            case 2: mpass<2, T>(buf, tab, t, n, Ns_, ts_, rn_, act); break;         \
            case 3: mpass<3, T>(buf, tab, t, n, Ns_, ts_, rn_, act); break;         \
            case 4: mpass<4, T>(buf, tab, t, n, Ns_, ts_, rn_, act); break;         \
            case 5: mpass<5, T>(buf, tab, t, n, Ns_, ts_, rn_, act); break;         \
            case 7: mpass<7, T>(buf, tab, t, n, Ns_, ts_, rn_, act); break;         \
            default: mpass<8, T>(buf, tab, t, n, Ns_, ts_, rn_, act); break;        \
        }                                                                           \
    }

}  // namespace vvh
