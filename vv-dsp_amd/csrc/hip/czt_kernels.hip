// czt_kernels.hip -- the unit of the one-pass chirp-z kernel (czt_fused.hpp:
// k_czt_fused) and the one-pass cepstrum family (ceps_fused.hpp: k_ceps_fused),
// with their launchers.  Both kernels walk rows with a persistent grid, one
// transform slot per row, so one launch rule serves them.
#include "czt_fused.hpp"
#include "ceps_fused.hpp"
#include "pow2_launch.hpp"

namespace vvh {

// `kern` over `rows` rows of an N-point transform on its resident grid (cached
// in `cap`, one per kernel instance); the kernel takes args..., then the
// pass-major and W_N^k tables.
template <int N, class K, class... A>
static hipError_t launch_fused_rows(std::atomic<int>& cap, K kern, long long rows, hipStream_t s, A... args) {
    const Pow2Tables tb(N);
    if (!tb.ok()) return hipErrorOutOfMemory;
    constexpr int WG = Wg<N>::value;
    const int grid = slot_grid(rows, Wg<N>::F, cached_grid(cap, (const void*)kern, WG, 0, 1LL << 40), true);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WG), 0, s, args..., tb.pass, tb.tab);
    return hipGetLastError();
}

bool czt_fused_supported(long long p) { return p >= 2 && p <= 4096 && (p & (p - 1)) == 0; }

// Bs = B / P (the inverse transform's scale folded into the chirp spectrum)
hipError_t launch_czt_fused(long long p, const void* x, int real_in, long long n, long long m, long long rows,
                            const float2* g, const float2* Bs, const float2* post, float2* X, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    return pow2_dispatch<2, 4096>(p, [&](auto pp) {
        constexpr int P = decltype(pp)::value;
        static std::atomic<int> cap[2];
        return real_in ? launch_fused_rows<P>(cap[1], k_czt_fused<P, true>, rows, s, x, n, m, rows, g, Bs, post, X)
                       : launch_fused_rows<P>(cap[0], k_czt_fused<P, false>, rows, s, x, n, m, rows, g, Bs, post, X);
    });
}

bool ceps_fused_supported(long long n) { return n >= 2 && n <= 4096 && (n & (n - 1)) == 0; }

// kind 0 cepstrum, 1 icepstrum_minphase, 2 minphase_from_cepstrum (y complex[rows][n])
hipError_t launch_ceps_fused(int kind, long long n, const float* x, long long rows, float* y, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    return pow2_dispatch<2, 4096>(n, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        static std::atomic<int> cap[3];
        if (kind == 0) return launch_fused_rows<N>(cap[0], k_ceps_fused<N, 0>, rows, s, x, rows, y);
        if (kind == 1) return launch_fused_rows<N>(cap[1], k_ceps_fused<N, 1>, rows, s, x, rows, y);
        return launch_fused_rows<N>(cap[2], k_ceps_fused<N, 2>, rows, s, x, rows, y);
    });
}

}  // namespace vvh
