// sq_rows.hip -- the register kernel's row instances: c2c rows (k_stft_sq
// MODE 0) at every length of the list, real rows of twice a half length (MODE 5).
#include "sq_kernel.hpp"

namespace vvh {

bool sq_c2c(long long n, const MixIO& io, long long batch, hipStream_t s, hipError_t* e) {
    return sq_dispatch<false>(n, [&](auto n1, auto n2) {
        *e = run_stft_sq<decltype(n1)::value, decltype(n2)::value, 0>(io, batch, s);
    });
}

bool sq_r2c(long long n2, const MixIO& io, long long batch, hipStream_t s, hipError_t* e) {
    if (n2 % 2) return false;
    return sq_dispatch<true>(n2 / 2, [&](auto n1, auto n2c) {
        *e = run_stft_sq<decltype(n1)::value, decltype(n2c)::value, 5>(io, batch, s);
    });
}

}  // namespace vvh
