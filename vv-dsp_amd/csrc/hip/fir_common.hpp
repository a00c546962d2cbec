// fir_common.hpp -- what the FIR kernel families (fir_pair.hpp, fir_bulk_reg.hpp,
// fir_r32.hpp, fir_direct.hpp) share on the device: where a filter's input
// sample comes from.
#pragma once
#include "fft_core.hpp"

namespace vvh {

// vv_dsp_filtfilt_fir's reflect padding (common.c:6-21): sample idx of
// ext = [reflection | x | reflection] counted from x[0] (idx < 0: the left pad,
// idx >= xn: the right pad) is x[fir_reflect(idx, xn)]:
// left pad ext[pad-1-i] = x[min(i+1, xn) - 1], right pad ext[pad+xn+i] = x[i + 1 <= xn ? xn-1-i : 0]
__device__ __forceinline__ long long fir_reflect(long long idx, long long xn) {
    if (idx < 0) return (-idx < xn ? -idx : xn) - 1;
    if (idx < xn) return idx;
    return (idx - xn + 1 <= xn) ? 2 * xn - 1 - idx : 0;
}

// Input sample idx of a channel (xc its sample 0, n samples).
// SRC 0: x[idx] for 0 <= idx < n; a sample before 0 comes from the history
//        prefix if it has one there (pc: the channel's lm1 = taps - 1 samples,
//        chronological; NULL: none), else 0 -- samples before -lm1 never meet a
//        tap and must not be read past the prefix; a sample at or past n is 0.
// SRC 1: the reflect-padded input of filtfilt's forward pass; `xn` is x's
//        length, n the pass's output count (zero at or past n).
template <int SRC>
__device__ __forceinline__ float fir_fetch(const float* xc, const float* pc, long long idx, long long n, long long lm1,
                                           long long xn) {
    if constexpr (SRC == 0) {
        if (idx < 0) return (pc && idx >= -lm1) ? pc[lm1 + idx] : 0.0f;
        return idx < n ? xc[idx] : 0.0f;
    } else {
        if (idx >= n) return 0.0f;
        return xc[fir_reflect(idx, xn)];
    }
}

}  // namespace vvh
