// fir_ols.hip -- overlap-save launches (launch_fir_ols): the block geometry, the
// router over the three routes, and the route every block size can take
// (k_fir_pair, fir_pair.hpp).  The N = 1024 routes are in fir_1024.hip.
#include "fir_launch.hpp"
#include "fir_pair.hpp"

#include <cstdint>

namespace vvh {

// Effective history of the block geometry (see fir_pair.hpp's header comment).
long long fir_effective_history(long long nfft, long long taps) {
    long long le = taps - 1;
    if (le < nfft / 4) le = nfft / 4;
    return (le + 3) & ~3LL;
}

FirGeo fir_geometry(long long nfft, long long le, long long n) {
    FirGeo g;
    g.le = le;
    g.lout = nfft - le;
    g.nblk = (n + g.lout - 1) / g.lout;
    g.ppc = (g.nblk + 1) / 2;
    g.qf = (le + 2 * g.lout - 1) / (2 * g.lout);
    g.ql = n / (2 * g.lout);   // (2q+2)*lout <= n  <=>  q < n/(2 lout)
    if (g.ql > g.ppc) g.ql = g.ppc;
    if (g.qf >= g.ql) g.qf = g.ql = g.ppc;
    return g;
}

// LDS-DMA bulk variant: one wave per transform, where span + exchange + H +
// twiddles (80 KB per 4 transforms) still leave two workgroups per CU
template <int N>
constexpr bool FIR_BULK = Geo<N>::T == 64;

// The bulk pairs (16 B aligned channels, FIR_BULK sizes) through the LDS-DMA
// kernel, the edge pairs [0, qf) and [ql, ppc) -- every pair, without bulk pairs --
// through the bounds-checked one in a second launch.
template <int N>
static hipError_t fir_route_pair(const FirJob& j, FirGeo g) {
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    if (!FIR_BULK<N> || !fir_span_aligned(j)) g.qf = g.ql = g.ppc;
    const bool bulk = g.ql > g.qf;
    const float2* tN = twiddle_table(N);
    const float2* pN = pass_twiddles(N);
    float* sink = bulk ? store_sink() : nullptr;
    if (!tN || !pN || (bulk && !sink)) return hipErrorOutOfMemory;
    const long long lm1 = j.taps - 1;
    static std::atomic<int> capc_b, capc_e;
    if constexpr (FIR_BULK<N>) {
        if (bulk) {
            const long long cnt = g.ql - g.qf;
            // persistent (chunked launches measured slower)
            const int grid = capped_grid(capc_b, (const void*)k_fir_pair<N, true>, WG, (j.nch * cnt + F - 1) / F);
            hipLaunchKernelGGL((k_fir_pair<N, true>), dim3(grid), dim3(WG), 0, j.s, lm1, g.le, j.H, j.x, j.y, j.n, j.nch,
                               j.x_stride, j.y_stride, j.prefix, cnt, 0LL, g.qf, pN, tN, sink, 0LL);
        }
    }
    const long long ecnt = g.qf + (g.ppc - g.ql);   // edge pairs per channel
    if (ecnt > 0) {
        const int grid = capped_grid(capc_e, (const void*)k_fir_pair<N, false>, WG, (j.nch * ecnt + F - 1) / F);
        hipLaunchKernelGGL((k_fir_pair<N, false>), dim3(grid), dim3(WG), 0, j.s, lm1, g.le, j.H, j.x, j.y, j.n, j.nch,
                           j.x_stride, j.y_stride, j.prefix, ecnt, g.qf, g.ql, pN, tN, sink, 0LL);
    }
    return hipGetLastError();
}

template <int N>
static hipError_t run_fir(const FirJob& j) {
    const long long le = fir_effective_history(N, j.taps);
    if (N - le < N / 4) return hipErrorInvalidValue;
    const FirGeo g = fir_geometry(N, le, j.n);
    // the bulk kernels read spans [2q*lout - le, (2q+2)*lout) and write outputs
    // below (2q+2)*lout without bounds checks: verify the range on the host
    if (g.ql > g.qf && (2 * g.qf * g.lout < le || 2 * g.ql * g.lout > j.n || N + g.lout > N + (3 * N) / 4))
        return hipErrorInvalidValue;
    if constexpr (N == 1024) {
        // le == N/4 holds for every filter fir_block gives N = 1024 (taps <= 257)
        if (le == N / 4) {
            // Knob FIR_R32 = 0: the 16 x 16 x 4 kernels (A/B); FIR_OLD = 1: of those, k_fir_pair (A/B, scripts/kbench.py)
            if (knob(KNOB_FIR_R32, 1) != 0) return fir_route_r32(j, g);
            if (g.ql > g.qf && fir_span_aligned(j) && knob(KNOB_FIR_OLD, 0) != 1) return fir_route_bulk_reg(j, g);
        }
    }
    return fir_route_pair<N>(j, g);
}

bool fir_ols_supported(long long nfft) { return nfft >= 64 && nfft <= 8192 && (nfft & (nfft - 1)) == 0; }

// H: N complex bins of FFT(h zero-padded to N) / N
hipError_t launch_fir_ols(long long nfft, long long taps, const float2* H, const float* x, float* y,
                          long long n, long long nch, long long x_stride, long long y_stride,
                          const float* prefix, hipStream_t s) {
    const FirJob j{taps, H, x, y, n, nch, x_stride, y_stride, prefix, s};
    switch (nfft) {
        case 64: return run_fir<64>(j); case 128: return run_fir<128>(j); case 256: return run_fir<256>(j);
        case 512: return run_fir<512>(j); case 1024: return run_fir<1024>(j); case 2048: return run_fir<2048>(j);
        case 4096: return run_fir<4096>(j); case 8192: return run_fir<8192>(j);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vvh
