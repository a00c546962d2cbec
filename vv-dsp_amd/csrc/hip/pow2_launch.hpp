// pow2_launch.hpp -- what the launchers of the power-of-two register/LDS kernels
// (fft_c2c.hip, fft_real.hip, analytic_kernels.hip, czt_kernels.hip) and of the
// two-pass four-step (fourstep_fft.hip) share.  Host code only; private to these units.
#pragma once
#include "vvhip_internal.hpp"

#include <type_traits>

namespace vvh {

// f(std::integral_constant<int, N>{}) for the power of two N == n in LO..HI; any
// other n is hipErrorInvalidValue.  f is a generic callable, instantiated once per
// size: a `static std::atomic<int>` grid cache inside it is one per size.
template <int LO, int HI, class F>
inline hipError_t pow2_dispatch(long long n, F&& f) {
    if constexpr (LO > HI) {
        return hipErrorInvalidValue;
    } else {
        if (n == LO) return f(std::integral_constant<int, LO>{});
        return pow2_dispatch<2 * LO, HI>(n, f);
    }
}

// The device tables of an N-point transform: W_N^k, the pass-major inter-pass
// twiddles and, for the real transforms' split step, W_2N^k.
struct Pow2Tables {
    const float2 *tab, *pass, *post2M = nullptr;
    bool real;
    explicit Pow2Tables(int n, bool real_split = false) : tab(twiddle_table(n)), pass(pass_twiddles(n)), real(real_split) {
        if (real) post2M = twiddle_table(2 * n);
    }
    bool ok() const { return tab && pass && (!real || post2M); }   // false: hipErrorOutOfMemory
};

// Workgroups for `batch` units at F per workgroup: a persistent grid takes at most
// its `cap` resident workgroups, any other grid every workgroup (at most 2^30).
inline int slot_grid(long long batch, long long F, long long cap, bool persistent) {
    const long long need = (batch + F - 1) / F, lim = persistent ? cap : (1LL << 30);
    return (int)(need < lim ? need : lim);
}

}  // namespace vvh
