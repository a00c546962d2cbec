// fourstep_chain.hpp -- the two-pass four-step chain with its optional fused
// element-wise stages, as fourstep_fft.hip gives it to bluestein.hip.  Host
// side; private to these two units (the kernels: fourstep.hpp).
#pragma once
#include <hip/hip_runtime.h>

namespace vvh {

// Optional fused element-wise stages of the two passes (Bluestein):
//   pre  (columns pass input):  x[m] = m < nsig ? raw[b*in_dist + m] * pre_chirp[m] : 0
//   mulv (rows pass output):    X[k] *= mulv[k]
//   post (rows pass output):    post_out[b*out_dist + k] = post_scale * post_chirp[k] * X[k], k < nout
// b counts from b0 (the chunk's first transform).  All null: the plain FFT.
struct FsHooks {
    const float2* mulv = nullptr;
    const float2* pre_chirp = nullptr;
    const void* raw = nullptr;
    long long in_dist = 0, nsig = 0;
    int real_in = 0;
    const float2* post_chirp = nullptr;
    float2* post_out = nullptr;
    long long out_dist = 0, nout = 0;
    float post_scale = 1.0f;
    long long b0 = 0;
};

// One two-pass transform chain over a batch in chunks, n = 2^lg = N1*N2 with
// 64 <= N1 <= N2 <= 1024.  With hooks, the columns pass may read the raw
// Bluestein input (pre) instead of `in`, and the rows pass may multiply by a
// vector (mulv) and/or write scaled, chirped and truncated rows to another
// buffer (post) instead of `out`.
hipError_t twopass_chain(long long n, int lg, int fwd, const float2* in, float2* out, long long batch, hipStream_t s,
                         FsHooks hk);

}  // namespace vvh
