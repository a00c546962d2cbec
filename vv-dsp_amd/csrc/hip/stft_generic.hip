// stft_generic.hip -- the element-wise kernels around the generic STFT path (any
// nfft: frame gather, a batched FFT plan, magnitudes or power) and the
// half-spectrum packing of magnitude rows.
#include "stft_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ---- generic path (any nfft): gather windowed complex frames, then a batched
// C2C plan, then magnitudes.
__global__ void k_frame_gather(long long nfft, long long hop, const float* sig, long long n,
                               long long nch, long long ch_stride, long long frames,
                               const float* win, float2* out) {
    const long long total = nch * frames * nfft;
    VVH_GRID_STRIDE(i, total) {
        const long long e = i % nfft, fr = (i / nfft) % frames, c = i / (nfft * frames);
        const long long idx = fr * hop + e;
        const float v = (idx < n) ? sig[c * ch_stride + idx] : 0.0f;
        out[i] = make_float2(v * win[e], 0.0f);
    }
}

hipError_t launch_frame_gather(long long nfft, long long hop, const float* sig, long long n,
                               long long nch, long long ch_stride, long long frames, const float* win,
                               float2* out, hipStream_t s) {
    const long long total = nch * frames * nfft;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_frame_gather, dim3(stride_blocks(total)), dim3(256), 0, s, nfft, hop, sig, n, nch,
                       ch_stride, frames, win, out);
    return hipGetLastError();
}

__global__ void k_magnitude(const float2* in, float* out, long long count) {
    VVH_GRID_STRIDE(i, count) {
        const float2 v = in[i];
        out[i] = cmag(v.x, v.y);
    }
}

hipError_t launch_magnitude(const float2* in, float* out, long long count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_magnitude, dim3(stride_blocks(count)), dim3(256), 0, s, in, out, count);
    return hipGetLastError();
}

// Half-spectrum packing for the config-5 gather (SURVEY 8e row note 1): the
// magnitude rows of real frames are mirror-symmetric, |X[n-k]| = |X[k]|, so
// bins 0..n/2 carry the whole row.  Pack: [rows][n] -> [rows][n/2+1]; unpack:
// out[k] = in[k <= n/2 ? k : n-k].  One workgroup per row (grid-stride over rows).
__global__ void __launch_bounds__(256) k_rows_half_pack(const float* in, float* out, long long rows, long long n) {
    const long long h = n / 2 + 1;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* src = in + r * n;
        float* dst = out + r * h;
        for (long long k = threadIdx.x; k < h; k += 256) dst[k] = src[k];
    }
}

__global__ void __launch_bounds__(256) k_rows_half_unpack(const float* in, float* out, long long rows, long long n) {
    const long long h = n / 2 + 1;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* src = in + r * h;
        float* dst = out + r * n;
        for (long long k = threadIdx.x; k < n; k += 256) dst[k] = src[k < h ? k : n - k];
    }
}

hipError_t launch_rows_half(const float* in, float* out, long long rows, long long n, int unpack, hipStream_t s) {
    if (rows <= 0 || n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(rows < 262144 ? rows : 262144);
    if (unpack) hipLaunchKernelGGL(k_rows_half_unpack, dim3(grid), dim3(256), 0, s, in, out, rows, n);
    else hipLaunchKernelGGL(k_rows_half_pack, dim3(grid), dim3(256), 0, s, in, out, rows, n);
    return hipGetLastError();
}

// |X[k]|^2 for k <= nfft/2 of rows [rows][nfft] -> [rows][nfft/2+1]
__global__ void k_power_half(const float2* in, float* out, long long nfft, long long count) {
    const long long nh = nfft / 2 + 1;
    VVH_GRID_STRIDE(i, count) {
        const long long r = i / nh, k = i - r * nh;
        const float2 v = in[r * nfft + k];
        out[i] = __builtin_fmaf(v.x, v.x, v.y * v.y);
    }
}

hipError_t launch_power_half(const float2* in, float* out, long long nfft, long long rows, hipStream_t s) {
    const long long count = rows * (nfft / 2 + 1);
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_power_half, dim3(stride_blocks(count)), dim3(256), 0, s, in, out, nfft, count);
    return hipGetLastError();
}

}  // namespace vvh
