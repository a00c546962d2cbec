// fft_rules.hpp -- device rules that the power-of-two kernel families (fft_c2c.hpp,
// fft_real.hpp, hilbert_fused.hpp, dct2_fused.hpp, fft_glue.hip) share, one copy
// each: a slot's row load, the C2C output scale, the wave-block staging of the
// small lengths and the DC / Nyquist bins of the real split step.  The helpers
// return values and the caller loads and stores at its own address expression:
// helpers that took the block's base, or stored a transform, compiled to other
// device code ("The power-of-two units").
#pragma once
#include "fft_core.hpp"

namespace vvh {

// A slot's transform from HBM: register r of thread t holds point t + r T.
template <int N>
__device__ __forceinline__ void rows_load(float2 (&v)[Geo<N>::P], const float2* src, int t) {
#pragma unroll
    for (int r = 0; r < Geo<N>::P; ++r) v[r] = ld_nt(src + t + r * Geo<N>::T);
}

// A C2C output value: the backward transform is scaled.
template <bool FWD>
__device__ __forceinline__ float2 c2c_out(float2 o, float scale) {
    if (!FWD) o = cscale(o, scale);
    return o;
}

// ---- wave-block staging (the 16..128-point kernels) ------------------------
// A wave's 64 / T transforms are one dense block of 1024 float2 = 2048 floats
// (8 KB).  It moves between HBM and the wave's LDS area as 16 B per lane in
// WB_STEPS steps of 1 KB, masked by the count of valid elements, and lies in the
// area padded 1 per 16 elements (Geo::pad for float2, wb_padf for floats).
constexpr int WB_STEPS = 8, WB_CPX = 1024, WB_FLOATS = 2048;
// the lane's first element of step i, counted in float2 (WB_LANE_C per lane, WB_STEP_C
// per step) or in floats
constexpr int WB_LANE_C = 2, WB_STEP_C = 64 * WB_LANE_C, WB_LANE_F = 4, WB_STEP_F = 64 * WB_LANE_F;
__device__ __forceinline__ constexpr int wb_ec(int i, int lane) { return i * WB_STEP_C + WB_LANE_C * lane; }
__device__ __forceinline__ constexpr int wb_ef(int i, int lane) { return i * WB_STEP_F + WB_LANE_F * lane; }
__host__ __device__ constexpr int wb_padf(int e) { return e + (e >> 4); }
static_assert(wb_ec(WB_STEPS, 0) == WB_CPX && wb_ef(WB_STEPS, 0) == WB_FLOATS, "8 steps cover the block");

// 16 B of the block from p, zeros past the valid elements
template <class T>
__device__ __forceinline__ vf4_t wb_ld(const T* p, bool valid) {
    return valid ? __builtin_nontemporal_load(reinterpret_cast<const vf4_t*>(p)) : vf4_t{0.0f, 0.0f, 0.0f, 0.0f};
}
template <class T>
__device__ __forceinline__ void wb_st(vf4_t q, T* p) {
    __builtin_nontemporal_store(q, reinterpret_cast<vf4_t*>(p));
}
// the lane's 16 B to / from the wave's area at element e: two float2, or four floats
template <class G>
__device__ __forceinline__ void wb_put_c(float2* wa, int e, vf4_t q) {
    wa[G::pad(e)] = make_float2(q[0], q[1]);
    wa[G::pad(e + 1)] = make_float2(q[2], q[3]);
}
template <class G>
__device__ __forceinline__ vf4_t wb_get_c(const float2* wa, int e) {
    const float2 a = wa[G::pad(e)], b = wa[G::pad(e + 1)];
    return vf4_t{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void wb_put_f(float* wa, int e, vf4_t q) {
#pragma unroll
    for (int k = 0; k < 4; ++k) wa[wb_padf(e + k)] = q[k];
}
__device__ __forceinline__ vf4_t wb_get_f(const float* wa, int e) {
    vf4_t q;
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = wa[wb_padf(e + k)];
    return q;
}

// ---- the real split step at k = 0 -----------------------------------------
// Forward: bins 0 and M of the real row from Z[0], imaginary parts 0
// (fft_kiss.c:141-143); every other bin is split_fwd(Z[k], conj Z[M-k], W_2M^k).
// (Z[0] as two floats: taking the float2, k_r2c compiled to other code)
__device__ __forceinline__ float2 split_fwd_dc(float re, float im) { return make_float2(re + im, 0.0f); }
__device__ __forceinline__ float2 split_fwd_nyq(float re, float im) { return make_float2(re - im, 0.0f); }
// Inverse: split_inv's (A, B) at k = 0 are bins 0 and M without their imaginary
// parts (the fft_kiss.c:158-171 result); every other k takes (X[k], X[M-k]).
__device__ __forceinline__ float2 split_inv_edge(float2 X) { return make_float2(X.x, 0.0f); }

}  // namespace vvh
