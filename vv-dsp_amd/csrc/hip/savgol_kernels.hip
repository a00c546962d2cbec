// savgol_kernels.hip -- Savitzky-Golay rows (src/filter/savgol.c:164-217): the
// boundary padding resolved as an index map, then
//     y[n] = (float) sum_{k < m} (double)h[k] * (double)xp[n + k]
// accumulated in f64 in window order and rounded once.  The product of two
// floats is exact in f64, so fma(h, x, acc) rounds exactly as the reference's
// multiply-then-add: the outputs are bit-identical to it.
//
// A workgroup of 256 lanes takes SG_SPAN = 1024 consecutive outputs of one row:
// the span plus the m - 1 halo samples go to LDS (coalesced reads, the NaN
// policy applied as a sample is read), the coefficients -- kernel arguments --
// go to LDS as doubles.  A lane owns 4 consecutive outputs and slides an
// 8-sample register window over its part of the span: per 4 taps one
// ds_read_b128 of samples (16 contiguous bytes per lane, conflict-free), 4
// broadcast coefficient reads and 16 f64 FMAs.
#include "vvhip_internal.hpp"

namespace vvh {

namespace {

constexpr int SG_T = 256, SG_PER = 4, SG_SPAN = SG_T * SG_PER;
constexpr int SG_XS = SG_SPAN + SAVGOL_MAX_WINDOW - 1 + 4;   // span + halo + the last window refill

struct SavgolArgs {
    const float* x;
    float* y;
    long long n, spans, x_stride, y_stride;
    int m, mode, policy;
    int* flag;
    float h[SAVGOL_MAX_WINDOW];
};

// sample index behind position t of the padded row, t in [-half, n + half)
// (savgol.c:170-201; i counts outwards from the edge)
__device__ __forceinline__ long long savgol_src(long long t, long long n, int mode) {
    if (t >= 0 && t < n) return t;
    long long src;
    if (t < 0) {
        const long long i = -t - 1;
        if (mode == 0) {
            src = i + 1;
            if (src >= n) src = n - 1;
        } else if (mode == 3) {
            src = (n - (i % n) - 1) % n;
        } else {
            src = 0;
        }
    } else {
        const long long i = t - n;
        if (mode == 0) src = n >= 2 ? n - 2 - i : n - 1;
        else if (mode == 3) src = i % n;
        else src = n - 1;
    }
    return src < 0 ? 0 : src;   // unreachable for m <= n; keeps the read inside the row regardless
}

// src/core/nan_policy.c:40-83: 1 zero, 3 clamp (NaN -> 0, Inf -> +-FLT_MAX); 2 raises `bit` in *flag
__device__ __forceinline__ float savgol_policy(float v, int policy, int* flag, int bit) {
    if (policy == 0 || isfinite(v)) return v;
    if (policy == 1) return 0.0f;
    if (policy == 2) {
        atomicOr(flag, bit);
        return v;
    }
    return isnan(v) ? 0.0f : (v > 0 ? 3.402823466e+38f : -3.402823466e+38f);
}

__global__ void __launch_bounds__(SG_T) k_savgol(const SavgolArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[SG_XS];
    __shared__ double hs[SAVGOL_MAX_WINDOW + 3];
    const int tid = threadIdx.x;
    const long long row = blockIdx.x / a.spans, n0 = (blockIdx.x % a.spans) * SG_SPAN;
    const int m = a.m, half = m / 2;
    const float* xr = a.x + row * a.x_stride;

    for (int k = tid; k < m; k += SG_T) hs[k] = (double)a.h[k];
    const long long padded = a.n + 2 * (long long)half;
    const int need = SG_SPAN + m - 1 + 4;
    for (int i = tid; i < need; i += SG_T) {
        const long long q = n0 + i;   // position in the padded row
        float v = 0.0f;
        if (q < padded) v = savgol_policy(xr[savgol_src(q - half, a.n, a.mode)], a.policy, a.flag, 1);
        xs[i] = v;
    }
    __syncthreads();

    const float4* xs4 = reinterpret_cast<const float4*>(xs) + tid;
    double acc[SG_PER] = {0.0, 0.0, 0.0, 0.0};
    float w[8];
    {
        const float4 f = xs4[0];
        w[0] = f.x, w[1] = f.y, w[2] = f.z, w[3] = f.w;
    }
    for (int kb = 0; kb < m; kb += 4) {
        const float4 f = xs4[kb / 4 + 1];
        w[4] = f.x, w[5] = f.y, w[6] = f.z, w[7] = f.w;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kb + kk < m) {
                const double h = hs[kb + kk];
#pragma unroll
                for (int o = 0; o < SG_PER; ++o) acc[o] = fma(h, (double)w[kk + o], acc[o]);
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) w[o] = w[o + 4];
    }

    const long long o0 = n0 + (long long)tid * SG_PER;
    if (o0 >= a.n) return;
    float out[SG_PER];
#pragma unroll
    for (int o = 0; o < SG_PER; ++o)
        out[o] = o0 + o < a.n ? savgol_policy((float)acc[o], a.policy, a.flag, 2) : 0.0f;
    float* yp = a.y + row * a.y_stride + o0;
    if (o0 + SG_PER <= a.n && (reinterpret_cast<uintptr_t>(yp) & 15) == 0) {
        *reinterpret_cast<float4*>(yp) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int o = 0; o < SG_PER; ++o)
            if (o0 + o < a.n) yp[o] = out[o];
    }
}

}  // namespace

hipError_t launch_savgol(const float* x, long long n, long long batch, long long x_stride, const float* h, int m,
                         int mode, int policy, float* y, long long y_stride, int* flag, hipStream_t s) {
    if (n <= 0 || batch <= 0) return hipSuccess;
    if (m < 1 || m > SAVGOL_MAX_WINDOW || m % 2 == 0 || m > n || mode < 0 || mode > 3 || (policy == 2 && !flag))
        return hipErrorInvalidValue;
    SavgolArgs a;
    a.x = x;
    a.y = y;
    a.n = n;
    a.spans = (n + SG_SPAN - 1) / SG_SPAN;
    a.x_stride = x_stride;
    a.y_stride = y_stride;
    a.m = m;
    a.mode = mode;
    a.policy = policy;
    a.flag = flag;
    for (int k = 0; k < SAVGOL_MAX_WINDOW; ++k) a.h[k] = k < m ? h[k] : 0.0f;
    const long long blocks = a.spans * batch;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_savgol, dim3((unsigned)blocks), dim3(SG_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace vvh
