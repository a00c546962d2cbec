// ceps_stages.hip -- element-wise stages of the real cepstrum / minimum-phase
// family for gfx950, for the lengths the one-pass kernels (ceps_fused.hpp) do
// not take.  The transforms between them are the library's own FFT launches
// (fft_run in shim_fft.hip).
//
// Cepstrum (src/envelope/cepstrum.c:7-41): c = Re IFFT(log(|FFT(x)| + 1e-12)),
// computed as R2C -> log-magnitude of the n/2+1 bins -> C2R (the log-magnitude
// spectrum of a real signal is real and even, so C2R gives its real inverse).
// Minimum phase (cepstrum.c:43-78, minphase.c:7-31): the causal fold of a
// cepstrum (c0, 2c1 .. 2c(n/2-1), 0 ..), a C2C FFT, then exp of the real part.
#include "vvhip_internal.hpp"

namespace vvh {

// Y[i] = (logf(sqrtf(re^2 + im^2) + 1e-12f), 0)  (cepstrum.c:26-32, float build)
__global__ void k_log_magnitude(float2* Y, long long count) {
    VVH_GRID_STRIDE(i, count) {
        const float2 v = Y[i];
        Y[i] = make_float2(logf(sqrtf(v.x * v.x + v.y * v.y) + 1e-12f), 0.0f);
    }
}

hipError_t launch_log_magnitude(float2* Y, long long count, hipStream_t s) {
    hipLaunchKernelGGL(k_log_magnitude, dim3(stride_blocks(count)), dim3(256), 0, s, Y, count);
    return hipGetLastError();
}

// C[r][i] = (c0, 0), (2 c[i], 0) for 1 <= i < n/2, else 0  (cepstrum.c:50-55, minphase.c:15-19)
__global__ void k_cepstrum_fold(const float* __restrict__ c, long long n, long long rows, float2* __restrict__ C) {
    const long long nh = n / 2;
    VVH_GRID_STRIDE(i, n * rows) {
        const long long j = i % n;
        float v = 0.0f;
        if (j == 0) v = c[i];
        else if (j < nh) v = 2.0f * c[i];
        C[i] = make_float2(v, 0.0f);
    }
}

hipError_t launch_cepstrum_fold(const float* c, long long n, long long rows, float2* C, hipStream_t s) {
    hipLaunchKernelGGL(k_cepstrum_fold, dim3(stride_blocks(n * rows)), dim3(256), 0, s, c, n, rows, C);
    return hipGetLastError();
}

// H[i] = (exp(Re H[i]), 0): dbl = 0 expf (cepstrum.c:64-69), 1 (float)exp((double)..) (minphase.c:24)
__global__ void k_exp_real(float2* H, long long count, int dbl) {
    VVH_GRID_STRIDE(i, count) {
        const float re = H[i].x;
        H[i] = make_float2(dbl ? (float)exp((double)re) : expf(re), 0.0f);
    }
}

hipError_t launch_exp_real(float2* H, long long count, int dbl, hipStream_t s) {
    hipLaunchKernelGGL(k_exp_real, dim3(stride_blocks(count)), dim3(256), 0, s, H, count, dbl);
    return hipGetLastError();
}

}  // namespace vvh
