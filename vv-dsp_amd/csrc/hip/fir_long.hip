// fir_long.hip -- the gather and scatter kernels of overlap-save for filters
// longer than the fused kernels take (shim_fir.hip fir_ols_long).
#include "fir_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// Overlap-save for filters longer than the fused kernels take (N > 8192):
// blocks j (2 per complex row: z = a + i b, as k_fir_pair) gathered into rows
// of an N-point batch, FFT, x H (FFT(h) unscaled; the inverse applies 1/N),
// inverse FFT, and the block outputs LE..N-1 scattered back.  The FFTs are the
// four-step kernels (fourstep_fft.hip) and the product is k_cmul_rows
// (chirp_glue.hip); these two kernels are the rest of the glue.
// Row q of a chunk is pair p = p0 + q over (channel, pair) items.
// ------------------------------------------------------------------------
__global__ void k_fir_long_gather(const float* x, long long n, long long x_stride, long long nfft, long long le,
                                  long long lout, long long ppc, long long p0, long long rows, float2* z) {
    const long long total = rows * nfft;
    VVH_GRID_STRIDE(i, total) {
        const long long q = i / nfft, e = i - q * nfft, p = p0 + q;
        const long long c = p / ppc, j = 2 * (p - c * ppc);
        const float* xc = x + c * x_stride;
        const long long ia = j * lout - le + e, ib = ia + lout;
        const float a = fir_fetch<0>(xc, nullptr, ia, n, 0, n);   // zero state: no history
        const float b = fir_fetch<0>(xc, nullptr, ib, n, 0, n);
        z[i] = make_float2(a, b);
    }
}

__global__ void k_fir_long_scatter(const float2* z, float* y, long long n, long long y_stride, long long nfft,
                                   long long le, long long lout, long long ppc, long long p0, long long rows) {
    const long long total = rows * lout;
    VVH_GRID_STRIDE(i, total) {
        const long long q = i / lout, k = i - q * lout, p = p0 + q;
        const long long c = p / ppc, j = 2 * (p - c * ppc);
        const float2 v = z[q * nfft + le + k];
        float* yc = y + c * y_stride;
        const long long oa = j * lout + k, ob = oa + lout;
        if (oa < n) yc[oa] = v.x;
        if (ob < n) yc[ob] = v.y;
    }
}

hipError_t launch_fir_long_gather(const float* x, long long n, long long x_stride, long long nfft, long long le,
                                  long long lout, long long ppc, long long p0, long long rows, float2* z,
                                  hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fir_long_gather, dim3(stride_blocks(rows * nfft)), dim3(256), 0, s, x, n, x_stride, nfft, le,
                       lout, ppc, p0, rows, z);
    return hipGetLastError();
}

hipError_t launch_fir_long_scatter(const float2* z, float* y, long long n, long long y_stride, long long nfft,
                                   long long le, long long lout, long long ppc, long long p0, long long rows,
                                   hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fir_long_scatter, dim3(stride_blocks(rows * lout)), dim3(256), 0, s, z, y, n, y_stride, nfft,
                       le, lout, ppc, p0, rows);
    return hipGetLastError();
}

}  // namespace vvh
