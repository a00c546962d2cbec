// sq_stft.hip -- the register kernel's STFT instances: |X|, complex and |X|^2
// rows of frame pairs (k_stft_sq MODE 1, 2, 3) at every length of the list.
#include "sq_kernel.hpp"

namespace vvh {

bool sq_stft(long long nfft, int kind, const MixIO& io, long long pairs, hipStream_t s, hipError_t* e) {
    return sq_dispatch<false>(nfft, [&](auto n1, auto n2) {
        constexpr int N1 = decltype(n1)::value, N2 = decltype(n2)::value;
        switch (kind) {
            case 0: *e = run_stft_sq<N1, N2, 1>(io, pairs, s); break;
            case 1: *e = run_stft_sq<N1, N2, 2>(io, pairs, s); break;
            default: *e = run_stft_sq<N1, N2, 3>(io, pairs, s); break;
        }
    });
}

}  // namespace vvh
