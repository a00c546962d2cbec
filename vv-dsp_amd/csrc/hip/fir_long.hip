// fir_long.hip -- the glue kernels of overlap-save for filters longer than the
// fused kernels take (shim_fir.hip fir_ols_long).
#include "fir_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// Overlap-save for filters longer than the fused kernels take (N > 8192):
// blocks j (2 per complex row: z = a + i b, as k_fir_pair) gathered into rows
// of an N-point batch, FFT, x H (FFT(h) unscaled; the inverse applies 1/N),
// inverse FFT, and the block outputs LE..N-1 scattered back.  The FFTs are the
// four-step kernels (large_fft.hip); these three kernels are the glue.
// Row q of a chunk is pair p = p0 + q over (channel, pair) items.
// ------------------------------------------------------------------------
__global__ void k_fir_long_gather(const float* x, long long n, long long x_stride, long long nfft, long long le,
                                  long long lout, long long ppc, long long p0, long long rows, float2* z) {
    const long long total = rows * nfft;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long q = i / nfft, e = i - q * nfft, p = p0 + q;
        const long long c = p / ppc, j = 2 * (p - c * ppc);
        const float* xc = x + c * x_stride;
        const long long ia = j * lout - le + e, ib = ia + lout;
        const float a = fir_fetch<0>(xc, nullptr, ia, n, 0, n);   // zero state: no history
        const float b = fir_fetch<0>(xc, nullptr, ib, n, 0, n);
        z[i] = make_float2(a, b);
    }
}

__global__ void k_fir_long_mul(float2* Z, const float2* H, long long nfft, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x)
        Z[i] = cmul(Z[i], H[i % nfft]);
}

__global__ void k_fir_long_scatter(const float2* z, float* y, long long n, long long y_stride, long long nfft,
                                   long long le, long long lout, long long ppc, long long p0, long long rows) {
    const long long total = rows * lout;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long q = i / lout, k = i - q * lout, p = p0 + q;
        const long long c = p / ppc, j = 2 * (p - c * ppc);
        const float2 v = z[q * nfft + le + k];
        float* yc = y + c * y_stride;
        const long long oa = j * lout + k, ob = oa + lout;
        if (oa < n) yc[oa] = v.x;
        if (ob < n) yc[ob] = v.y;
    }
}

static unsigned glue_grid(long long total) {
    long long b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

hipError_t launch_fir_long_gather(const float* x, long long n, long long x_stride, long long nfft, long long le,
                                  long long lout, long long ppc, long long p0, long long rows, float2* z,
                                  hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fir_long_gather, dim3(glue_grid(rows * nfft)), dim3(256), 0, s, x, n, x_stride, nfft, le,
                       lout, ppc, p0, rows, z);
    return hipGetLastError();
}

hipError_t launch_fir_long_mul(float2* Z, const float2* H, long long nfft, long long rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fir_long_mul, dim3(glue_grid(rows * nfft)), dim3(256), 0, s, Z, H, nfft, rows * nfft);
    return hipGetLastError();
}

hipError_t launch_fir_long_scatter(const float2* z, float* y, long long n, long long y_stride, long long nfft,
                                   long long le, long long lout, long long ppc, long long p0, long long rows,
                                   hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fir_long_scatter, dim3(glue_grid(rows * lout)), dim3(256), 0, s, z, y, n, y_stride, nfft,
                       le, lout, ppc, p0, rows);
    return hipGetLastError();
}

}  // namespace vvh
