// fir_direct.hip -- launches of the bit-exact direct form and of filtfilt
// (k_fir_reg, and k_fir_direct behind knob FIR_DIRECT_LDS = 1; fir_direct.hpp).
#include "fir_direct.hpp"

#include <cstdint>

namespace vvh {

// One direct-form pass over nch rows: from registers, or through LDS under the
// A/B knob (1 = the LDS kernel) and for taps that are not 16 B aligned (k_fir_reg
// loads 16 B of taps at a time).  One workgroup per tile of outputs per row.
template <int SRC, bool REV>
static hipError_t run_fir_direct(const float* h, long long taps, const float* x, float* y, long long n, long long nch,
                                 long long x_stride, long long y_stride, const float* prefix,
                                 long long prefix_stride, long long xn, hipStream_t s) {
    const bool reg = knob(KNOB_FIR_DIRECT_LDS, 0) != 1 && ((uintptr_t)h & 15) == 0;
    const long long tiles = reg ? (n + REG_TILE - 1) / REG_TILE : (n + DIRECT_TILE - 1) / DIRECT_TILE;
    if (tiles * nch <= 0) return hipSuccess;
    if (taps < 1 || tiles * nch > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(tiles * nch));
    if (reg) {
        // the fast sample loads need 16 B aligned rows (a 4-float multiple stride)
        const int aligned = ((uintptr_t)x & 15) == 0 && (x_stride & 3) == 0;
        hipLaunchKernelGGL((k_fir_reg<SRC, REV>), grid, dim3(256), 0, s, h, taps, x, y, n, x_stride, y_stride, prefix,
                           prefix_stride, xn, tiles, aligned);
    } else {
        hipLaunchKernelGGL((k_fir_direct<SRC, REV>), grid, dim3(256), 0, s, h, taps, x, y, n, x_stride, y_stride,
                           prefix, prefix_stride, xn, tiles);
    }
    return hipGetLastError();
}

hipError_t launch_fir_direct(const float* h, long long taps, const float* x, float* y, long long n,
                             long long nch, long long x_stride, long long y_stride,
                             const float* prefix, hipStream_t s) {
    return run_fir_direct<0, false>(h, taps, x, y, n, nch, x_stride, y_stride, prefix, taps - 1, n, s);
}

// vv_dsp_filtfilt_fir (common.c:23-80) over nch rows of n samples: the forward
// pass writes the n + pad outputs of ext that the backward pass reads, already
// reversed (tmp_rev[j] = tmp[ext_n - 1 - j]); the backward pass is then a plain
// direct form over tmp_rev whose first pad samples are its history, and its n
// outputs are stored reversed into y.  Both passes keep the reference's
// summation order (acc = 0, += h[k] * s[i-k], k ascending, no FMA); every
// output needed has all its taps inside ext, so the reference's maxk bound
// never cuts a sum short and the results are bit-identical.
hipError_t launch_filtfilt(const float* h, long long taps, const float* x, float* y, long long n, long long nch,
                           long long x_stride, long long y_stride, float* tmp, hipStream_t s) {
    const long long pad = taps - 1, m = n + pad;
    if (n <= 0 || nch <= 0) return hipSuccess;
    if (taps < 1) return hipErrorInvalidValue;
    hipError_t e = run_fir_direct<1, true>(h, taps, x, tmp, m, nch, x_stride, m, nullptr, 0, n, s);
    if (e != hipSuccess) return e;
    return run_fir_direct<0, true>(h, taps, tmp + pad, y, n, nch, m, y_stride, tmp, m, n, s);
}

}  // namespace vvh
