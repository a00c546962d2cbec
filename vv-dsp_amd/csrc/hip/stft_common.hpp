// stft_common.hpp -- the pair arithmetic every STFT analysis kernel shares: two
// real frames a, b ride one complex FFT of z = w/2 (a + i b), and pair_post
// splits its bins back into the two frames' rows.
#pragma once
#include "fft_core.hpp"

namespace vvh {

// samples e = t + r*T of one frame (zero outside [0, n); all zero when !valid).
// `s` must point at a real channel.  The tail path clamps the index and selects
// instead of branching per element, so the loads stay branch-free.
template <int N>
__device__ __forceinline__ void frame_load(float* x, const float* s, long long start, long long n, int t,
                                           bool valid) {
    using G = Geo<N>;
    if (start + N <= n) {
#pragma unroll
        for (int r = 0; r < G::P; ++r) x[r] = s[start + t + r * G::T];
    } else {
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            const long long e = start + t + r * G::T;
            const float val = s[e < n ? e : n - 1];
            x[r] = e < n ? val : 0.0f;
        }
    }
    if (!valid) {
#pragma unroll
        for (int r = 0; r < G::P; ++r) x[r] = 0.0f;
    }
}

// |re + i im| with the hardware v_sqrt_f32 (<=1 ulp).  sqrtf's correctly
// rounded IEEE expansion costs ~10 VALU per bin; the magnitude is compared at
// the reference's float tolerance, never bit-exactly.
__device__ __forceinline__ float cmag(float re, float im) {
    return __builtin_amdgcn_sqrtf(__builtin_fmaf(re, re, im * im));
}

// Spectra of the two frames at bin k from Z = FFT(w/2 * (a + i b)):
//   Xa[k] = Z[k] + conj Z[N-k],  Xb[k] = -i (Z[k] - conj Z[N-k]).
// The 1/2 rides in the window (a power-of-two scale commutes with every
// rounding, so this is bit-identical to halving at the end).  Packed f32 math.
// MODE 0: A.x = |Xa[k]|, B.x = |Xb[k]|;  MODE 1: A = Xa[k], B = Xb[k];
// MODE 2: A.x = |Xa[k]|^2, B.x = |Xb[k]|^2 (power, bins 0..N/2 stored).
template <int MODE>
__device__ __forceinline__ void pair_post(float2 Z, float2 Zm, float2* A, float2* B) {
    const vf2_t z = {Z.x, Z.y}, zm = {Zm.x, Zm.y};
    const vf2_t s = z + zm;   // (Re Xa, Re Xb)
    const vf2_t d = z - zm;   // (-Im Xb, Im Xa)
    if constexpr (MODE == 0 || MODE == 2) {
        const vf2_t dd = d * d;
        // an explicit fused multiply-add: every call site rounds the same way, so
        // bins k and N-k (the same conjugate pair) get bit-identical values
        // wherever they are computed (lane 0's partner bins, tail pairs) -- the
        // half-spectrum gather relies on it (vv_dsp_spectrogram_unpack_half_device)
        const vf2_t m2 = __builtin_elementwise_fma(s, s, dd.yx);   // (|Xa|^2, |Xb|^2)
        A->x = MODE == 0 ? __builtin_amdgcn_sqrtf(m2.x) : m2.x;
        B->x = MODE == 0 ? __builtin_amdgcn_sqrtf(m2.y) : m2.y;
        A->y = B->y = 0.0f;
    } else {
        *A = make_float2(s.x, d.y);
        *B = make_float2(s.y, -d.x);
    }
}

// bin k of an output row (MODE 0: float magnitudes, MODE 1: float2 spectrum,
// MODE 2: float power of the half spectrum -- bins above N/2 are not stored)
template <int MODE, int N>
__device__ __forceinline__ void put_bin(char* row, int k, float2 X) {
    if constexpr (MODE == 0) *(reinterpret_cast<float*>(row) + k) = X.x;
    else if constexpr (MODE == 2) {
        if (k <= N / 2) *(reinterpret_cast<float*>(row) + k) = X.x;
    } else *(reinterpret_cast<float2*>(row) + k) = X;
}

}  // namespace vvh
