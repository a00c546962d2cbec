// fft_glue.hip -- what surrounds the fused FFT kernels: the O(n^2) DFT for
// lengths that are neither powers of two nor 7-smooth (f64 accumulation, the
// reference's own complexity for them: fft_kiss.c:76-92), the split step of
// real power-of-two lengths above 16384, and the element-wise glue kernels.
#include "fft_rules.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// O(n^2) DFT for arbitrary n (f64 accumulation, exact index reduction)
// ------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_dft_naive(long long n, int fwd, const void* in, int real_in, float2* out, long long nout,
            long long in_dist, long long out_dist, float scale, const double2* __restrict__ tab,
            long long kblocks) {
    __shared__ double2 tile[256];
    const long long f = (long long)blockIdx.x / kblocks;
    const long long k = ((long long)blockIdx.x % kblocks) * 256 + threadIdx.x;
    const float* rin = reinterpret_cast<const float*>(in) + (real_in ? f * in_dist : 0);
    const float2* cin = reinterpret_cast<const float2*>(in) + (real_in ? 0 : f * in_dist);
    double ar = 0.0, ai = 0.0;
    long long idx = 0;   // (k * t) mod n, advanced incrementally
    const long long kk = (k < n) ? k : 0;
    for (long long t0 = 0; t0 < n; t0 += 256) {
        const long long tt = t0 + threadIdx.x;
        if (tt < n) {
            if (real_in) tile[threadIdx.x] = make_double2((double)rin[tt], 0.0);
            else { const float2 c = cin[tt]; tile[threadIdx.x] = make_double2((double)c.x, (double)c.y); }
        }
        __syncthreads();
        const long long lim = (n - t0 < 256) ? (n - t0) : 256;
        for (long long j = 0; j < lim; ++j) {
            const double2 w = tab[idx];
            const double wi = fwd ? w.y : -w.y;
            const double2 x = tile[j];
            ar += x.x * w.x - x.y * wi;
            ai += x.x * wi + x.y * w.x;
            idx += kk;
            if (idx >= n) idx -= n;
        }
        __syncthreads();
    }
    if (k < nout) out[f * out_dist + k] = make_float2((float)(ar * scale), (float)(ai * scale));
}

hipError_t launch_dft_naive(long long n, int fwd, const void* in, int real_in, float2* out,
                            long long nout, long long batch, long long in_dist, long long out_dist,
                            float scale, hipStream_t s) {
    const double2* tab = twiddle_table_d(n);
    if (!tab) return hipErrorOutOfMemory;
    const long long kblocks = (nout + 255) / 256;
    if (kblocks * batch <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_dft_naive, dim3((unsigned)(kblocks * batch)), dim3(256), 0, s, n, fwd, in,
                       real_in, out, nout, in_dist, out_dist, scale, tab, kblocks);
    return hipGetLastError();
}

// ------------------------------------------------------------------------
// Real transforms above the fused kernels (pow2 n = 2M > 16384): the M-point
// complex transform of z[m] = x[2m] + i x[2m+1] (the real rows reinterpreted,
// no copy) and the split step, as k_r2c / k_c2r do in registers.  W_n^k from
// the two-level table lo[k & mask] * hi[k >> lo_bits].
// ------------------------------------------------------------------------
__device__ __forceinline__ float2 tw_split_at(const float2* __restrict__ tab, long long k, int lo_bits) {
    const long long mask = (1LL << lo_bits) - 1;
    return cmul(tab[k & mask], tab[(1LL << lo_bits) + (k >> lo_bits)]);
}

// Z: [batch][M] -> X: [batch][M+1] (bins 0..n/2 of the real rows).  Thread j of
// row f (blockIdx.y) makes bins j and M - j from the same two loads z[j], z[M-j]
// (each bin's twiddle from the table as before, so the bins are unchanged);
// 32-bit indices within a row.
__global__ void k_real_split_fwd(const float2* __restrict__ Z, float2* __restrict__ X, long long M, long long batch,
                                 const float2* __restrict__ tab, int lo_bits) {
    const int m = (int)M, h = m / 2;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > h) return;
    for (long long f = blockIdx.y; f < batch; f += gridDim.y) {
        const float2* z = Z + f * M;
        float2* x = X + f * (M + 1);
        const float2 a = z[j];
        if (j == 0) {   // DC and Nyquist (fft_kiss.c:141-143: imaginary part 0)
            x[0] = split_fwd_dc(a.x, a.y);
            x[m] = split_fwd_nyq(a.x, a.y);
        } else if (j == h && 2 * h == m) {
            x[j] = split_fwd(a, cconj(a), tw_split_at(tab, j, lo_bits));
        } else {
            const float2 b = z[m - j];
            x[j] = split_fwd(a, cconj(b), tw_split_at(tab, j, lo_bits));
            x[m - j] = split_fwd(b, cconj(a), tw_split_at(tab, m - j, lo_bits));
        }
    }
}

// X: [batch][M+1] -> V: [batch][M], the inverse split (imaginary parts of DC and
// Nyquist ignored, the fft_kiss.c:158-171 result), before the M-point inverse;
// thread j makes V[j] and V[M-j] from x[j], x[M-j]
__global__ void k_real_split_inv(const float2* __restrict__ X, float2* __restrict__ V, long long M, long long batch,
                                 const float2* __restrict__ tab, int lo_bits) {
    const int m = (int)M, h = m / 2;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > h) return;
    for (long long f = blockIdx.y; f < batch; f += gridDim.y) {
        const float2* x = X + f * (M + 1);
        float2* v = V + f * M;
        float2 a = x[j];
        if (j == 0) {
            v[0] = split_inv(split_inv_edge(a), split_inv_edge(x[m]), tw_split_at(tab, 0, lo_bits));
        } else if (j == h && 2 * h == m) {
            v[j] = split_inv(a, a, tw_split_at(tab, j, lo_bits));
        } else {
            const float2 b = x[m - j];
            v[j] = split_inv(a, b, tw_split_at(tab, j, lo_bits));
            v[m - j] = split_inv(b, a, tw_split_at(tab, m - j, lo_bits));
        }
    }
}

static dim3 split_grid(long long M, long long batch) {
    const long long bx = (M / 2 + 1 + 255) / 256;
    return dim3((unsigned)bx, (unsigned)(batch < 65535 ? (batch < 1 ? 1 : batch) : 65535));
}

hipError_t launch_real_split_fwd(const float2* Z, float2* X, long long M, long long batch, hipStream_t s) {
    int lo_bits = 0;
    const float2* tab = twiddle_split(2 * M, &lo_bits);
    if (!tab) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(k_real_split_fwd, split_grid(M, batch), dim3(256), 0, s, Z, X, M, batch, tab, lo_bits);
    return hipGetLastError();
}

hipError_t launch_real_split_inv(const float2* X, float2* V, long long M, long long batch, hipStream_t s) {
    int lo_bits = 0;
    const float2* tab = twiddle_split(2 * M, &lo_bits);
    if (!tab) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(k_real_split_inv, split_grid(M, batch), dim3(256), 0, s, X, V, M, batch, tab, lo_bits);
    return hipGetLastError();
}

// ------------------------------------------------------------------------
// Element-wise glue
// ------------------------------------------------------------------------
__global__ void k_herm_expand(long long n, const float2* half, float2* full, long long half_dist,
                              int zero_imag, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long f = i / n, k = i % n;
    const long long nh = n / 2 + 1;
    const float2* h = half + f * half_dist;
    float2 v;
    if (k < nh) {
        v = h[k];
        if (zero_imag && (k == 0 || (2 * k == n))) v.y = 0.0f;
    } else {
        const long long m = n - k;
        v = (m > 0 && m < nh) ? cconj(h[m]) : make_float2(0.0f, 0.0f);
    }
    full[i] = v;
}

hipError_t launch_hermitian_expand(long long n, const float2* half, float2* full, long long batch,
                                   long long half_dist, int zero_dc_nyq_imag, hipStream_t s) {
    const long long total = n * batch;
    hipLaunchKernelGGL(k_herm_expand, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n, half,
                       full, half_dist, zero_dc_nyq_imag, total);
    return hipGetLastError();
}

__global__ void k_take_real(const float2* in, float* out, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = in[i].x;
}

hipError_t launch_take_real(const float2* in, float* out, long long count, hipStream_t s) {
    hipLaunchKernelGGL(k_take_real, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, in, out, count);
    return hipGetLastError();
}

__global__ void k_promote_real(const float* __restrict__ in, float2* __restrict__ out, long long count) {
    VVH_GRID_STRIDE(i, count) out[i] = make_float2(in[i], 0.0f);
}

hipError_t launch_promote_real(const float* in, float2* out, long long count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_promote_real, dim3(stride_blocks(count)), dim3(256), 0, s, in, out, count);
    return hipGetLastError();
}

__global__ void k_zero_nyq(float2* out, long long n, long long batch, long long dist) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f < batch) out[f * dist + n / 2].y = 0.0f;
}

hipError_t launch_zero_nyquist_imag(float2* out, long long n, long long batch, long long dist,
                                    hipStream_t s) {
    if (n % 2) return hipSuccess;
    hipLaunchKernelGGL(k_zero_nyq, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, out, n, batch,
                       dist);
    return hipGetLastError();
}

__global__ void k_scale_r(float* p, long long count, float s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] *= s;
}
__global__ void k_scale_c(float2* p, long long count, float s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = cscale(p[i], s);
}
hipError_t launch_scale_real(float* p, long long count, float s, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_scale_r, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, p, count, s);
    return hipGetLastError();
}
hipError_t launch_scale_cpx(float2* p, long long count, float s, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_scale_c, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, p, count, s);
    return hipGetLastError();
}

}  // namespace vvh
