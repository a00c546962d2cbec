// chirp_glue.hip -- the element-wise stages of a chirp convolution through a
// pair of p-point FFTs, one copy for its three callers:
//   Bluestein (bluestein.hip): tab = a, p = M, off = 0, scaled by the caller's scale;
//   the chirp-z transform (shim_spectral.hip; czt.c:58-178), X[k] = sum_n x[n] A^-n W^(nk),
//     k < M, with P = next_pow2(N + M - 1):
//       a[i] = x[i] g[i] (i < N, else 0),  g[n] = A^-n W^(n^2/2)      k_chirp_pre
//       a <- IFFT(FFT(a) * B),  B = FFT(b), b[i] = W^(-(i-N+1)^2/2)    k_cmul_rows
//       X[k] = a[N-1+k] W^(k^2/2)                                      k_chirp_post, off = N - 1
//     (g, W^(k^2/2) and b are tabulated once per plan on the host in extended
//     precision: the reference rounds n^2/2 and its angle to float, which loses
//     the phase for N beyond a few hundred);
//   the long overlap-save FIR (shim_fir.hip): k_cmul_rows with H.
#include "fft_core.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// u[r][i] = x[r][i] * tab[i] for i < n, 0 for n <= i < p; real_in: x is float[r][n]
__global__ void k_chirp_pre(const void* __restrict__ x, int real_in, long long n, long long p, long long rows,
                            long long in_dist, const float2* __restrict__ g, float2* __restrict__ a) {
    VVH_GRID_STRIDE(i, p * rows) {
        const long long r = i / p, j = i - r * p;
        float2 v = make_float2(0.0f, 0.0f);
        if (j < n) {
            const float2 xv = real_in ? make_float2(static_cast<const float*>(x)[r * in_dist + j], 0.0f)
                                      : static_cast<const float2*>(x)[r * in_dist + j];
            v = cmul(xv, g[j]);
        }
        a[i] = v;
    }
}

hipError_t launch_chirp_pre(const void* x, int real_in, long long n, long long p, long long rows, long long in_dist,
                            const float2* tab, float2* u, hipStream_t s) {
    hipLaunchKernelGGL(k_chirp_pre, dim3(stride_blocks(p * rows)), dim3(256), 0, s, x, real_in, n, p, rows, in_dist,
                       tab, u);
    return hipGetLastError();
}

// a[r][i] *= B[i] (one spectrum shared by every row)
__global__ void k_cmul_rows(float2* __restrict__ a, const float2* __restrict__ B, long long p, long long rows) {
    VVH_GRID_STRIDE(i, p * rows) {
        const long long j = i % p;
        a[i] = cmul(a[i], B[j]);
    }
}

hipError_t launch_cmul_rows(float2* a, const float2* B, long long p, long long rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;   // the long FIR's rule (the CZT chain launched one idle block)
    hipLaunchKernelGGL(k_cmul_rows, dim3(stride_blocks(p * rows)), dim3(256), 0, s, a, B, p, rows);
    return hipGetLastError();
}

// X[r][k] = y[r][off + k] * tab[k], k < nout; SCALED: times scale, rounded after the product
template <bool SCALED>
__global__ void k_chirp_post(const float2* __restrict__ y, long long off, long long p, long long nout, long long rows,
                             const float2* __restrict__ tab, float2* __restrict__ X, long long out_dist, float scale) {
    VVH_GRID_STRIDE(i, nout * rows) {
        const long long r = i / nout, k = i - r * nout;
        float2 v = cmul(y[r * p + off + k], tab[k]);
        if constexpr (SCALED) v = cscale(v, scale);
        X[r * out_dist + k] = v;
    }
}

template <bool SCALED>
static hipError_t chirp_post(const float2* y, long long off, long long p, long long nout, long long rows,
                             const float2* tab, float2* X, long long out_dist, float scale, hipStream_t s) {
    hipLaunchKernelGGL(k_chirp_post<SCALED>, dim3(stride_blocks(nout * rows)), dim3(256), 0, s, y, off, p, nout, rows,
                       tab, X, out_dist, scale);
    return hipGetLastError();
}

hipError_t launch_chirp_post(const float2* y, long long off, long long p, long long nout, long long rows,
                             const float2* tab, float2* X, long long out_dist, hipStream_t s) {
    return chirp_post<false>(y, off, p, nout, rows, tab, X, out_dist, 1.0f, s);   // the kernel does not read scale
}

hipError_t launch_chirp_post_scaled(const float2* y, long long off, long long p, long long nout, long long rows,
                                    const float2* tab, float2* X, long long out_dist, float scale, hipStream_t s) {
    return chirp_post<true>(y, off, p, nout, rows, tab, X, out_dist, scale, s);
}

}  // namespace vvh
