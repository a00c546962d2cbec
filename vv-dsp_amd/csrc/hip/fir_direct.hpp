// fir_direct.hpp -- the bit-exact direct form (vv_dsp_fir_apply) and the two
// passes of vv_dsp_filtfilt_fir: k_fir_direct (through LDS) and k_fir_reg (from
// registers, the default); instantiated by fir_direct.hip.
#pragma once
#include "fir_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// Direct form, bit-identical to vv_dsp_fir_apply (fir.c:170-186):
//   acc = 0; acc += h[0]*x[i]; acc += h[t]*x[i-t] for t = 1..L-1 (newest first)
// with every product and sum rounded separately (no FMA contraction), so the
// f32 result equals the reference's.  Samples before x[0] come from `prefix`.
// A block owns DIRECT_TILE outputs; the taps go through LDS in tiles of
// DIRECT_TAPS (with the matching input window, DIRECT_TILE + DIRECT_TAPS - 1
// samples), the accumulators stay in registers across tiles, so any filter
// length keeps the reference's summation order in 37 KB of LDS.
// ------------------------------------------------------------------------
constexpr int DIRECT_TILE = 1024;
constexpr int DIRECT_TAPS = 4096;
constexpr int DIRECT_OPT = DIRECT_TILE / 256;   // outputs per thread

// SRC (fir_fetch<SRC>) 0: x[i] for 0 <= i < n, samples before x[0] from `prefix`
//        (taps-1 per channel, prefix_stride apart; NULL: zeros), zero past n.
// SRC 1: the reflect-padded input of vv_dsp_filtfilt_fir (common.c:6-21):
//        output i is sample pad + i of ext = [reflection | x | reflection] with
//        pad = taps - 1, so every tap lands inside ext; `xn` is x's length.
// REV:   output i is stored at y[n - 1 - i] (the filtfilt reversals).
template <int SRC, bool REV>
__global__ void __launch_bounds__(256)
k_fir_direct(const float* __restrict__ h, long long taps, const float* __restrict__ x,
             float* __restrict__ y, long long n, long long x_stride, long long y_stride,
             const float* __restrict__ prefix, long long prefix_stride, long long xn, long long tiles_per_ch) {
    __shared__ float hs[DIRECT_TAPS];
    __shared__ float xs[DIRECT_TILE + DIRECT_TAPS];
    const long long c = blockIdx.x / tiles_per_ch;
    const long long i0 = (blockIdx.x % tiles_per_ch) * DIRECT_TILE;
    const long long lm1 = taps - 1;
    const float* xc = x + c * x_stride;
    const float* pc = prefix ? prefix + c * prefix_stride : nullptr;
    float acc[DIRECT_OPT];
#pragma unroll
    for (int j = 0; j < DIRECT_OPT; ++j) acc[j] = 0.0f;
    for (long long t0 = 0; t0 < taps; t0 += DIRECT_TAPS) {
        const int tt = (int)(taps - t0 < DIRECT_TAPS ? taps - t0 : DIRECT_TAPS);
        __syncthreads();   // the previous tile's reads are done
        for (int u = threadIdx.x; u < tt; u += 256) hs[u] = h[t0 + u];
        // xs[e] = x[i0 - t0 - (tt - 1) + e], e < DIRECT_TILE + tt - 1
        const long long base = i0 - t0 - (tt - 1);
        for (int e = threadIdx.x; e < DIRECT_TILE + tt - 1; e += 256) {
            const long long idx = base + e;   // >= -lm1
            float v;
            // fir_fetch<SRC> written out: its idx >= -lm1 test and early return compile to other code here
            if constexpr (SRC == 0) {
                if (idx < 0) v = pc ? pc[lm1 + idx] : 0.0f;
                else v = (idx < n) ? xc[idx] : 0.0f;
            } else {
                const long long src = fir_reflect(idx, xn);
                v = (idx < n) ? xc[src] : 0.0f;
            }
            xs[e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < DIRECT_OPT; ++j) {
            const int o = threadIdx.x + 256 * j;
            const float* xi = xs + (tt - 1) + o;   // xi[-u] = x[i0 + o - (t0 + u)]
            float a = acc[j];
            // hipcc contracts a*b+c into v_fma regardless of pragmas; an empty asm on
            // the product keeps the multiply and the add separately rounded.
            for (int u = 0; u < tt; ++u) {
                float pt = hs[u] * xi[-u];
                asm volatile("" : "+v"(pt));
                a = a + pt;
            }
            acc[j] = a;
        }
    }
    float* yc = y + c * y_stride;
#pragma unroll
    for (int j = 0; j < DIRECT_OPT; ++j) {
        const long long i = i0 + threadIdx.x + 256 * j;
        if (i < n) yc[REV ? n - 1 - i : i] = acc[j];
    }
}

// ------------------------------------------------------------------------
// Direct form from registers (k_fir_reg): the same sums in the same order,
// without LDS.  A thread owns 16 consecutive outputs o0..o0+15 (a workgroup
// 4096) and runs the taps in tiles of 16.  For tile u0 its window is
// E[j] = s[o0 - u0 - 16 + j], j < 32, held as 24 register pairs
// Q[j] = (E[j], E[j+8]), so that the products for outputs (r, r+8) at tap
// u0+k are ONE packed multiply Q[16+r-k] * h[u0+k] (v_pk_mul_f32 with the tap
// broadcast by op_sel) and the sums one packed add: 16 VALU per 16 MACs, every
// product and sum separately rounded (the multiply is an asm statement, so no
// FMA can form).  The next tile's window is the previous one shifted by 16:
// eight pairs carry over, sixteen new samples come in (dwordx4 loads, L1/L2
// hits).  Tiles touching the signal's edges load element by element through
// the kernel's source rule (fir_fetch<SRC>: prefix / zeros / reflection; the
// last tap tile's window reaches up to 15 samples before -lm1), so results
// equal k_fir_direct's bit for bit.
// ------------------------------------------------------------------------
constexpr int REG_OPT = 16;                 // outputs per thread
constexpr int REG_TILE = 256 * REG_OPT;     // outputs per workgroup

template <int SRC, bool REV>
__global__ void __launch_bounds__(256)
k_fir_reg(const float* __restrict__ h, long long taps, const float* __restrict__ x, float* __restrict__ y, long long n,
          long long x_stride, long long y_stride, const float* __restrict__ prefix, long long prefix_stride,
          long long xn, long long tiles_per_ch, int aligned) {
    const long long c = blockIdx.x / tiles_per_ch;
    const long long ob = (blockIdx.x % tiles_per_ch) * REG_TILE;
    const long long o0 = ob + (long long)threadIdx.x * REG_OPT;
    const long long lm1 = taps - 1;
    const long long hi_ok = SRC == 1 ? (xn < n ? xn : n) : n;   // [0, hi_ok): plain loads
    const float* xc = x + c * x_stride;
    const float* pc = prefix ? prefix + c * prefix_stride : nullptr;
    vf2_t acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = vf2_t{0.0f, 0.0f};
    vf2_t Q[24];
    // tile 0 window: E[j] = s[o0 - 16 + j], j < 32
    {
        float E[32];
        const bool fast = aligned && ob - 16 >= 0 && ob + REG_TILE <= hi_ok;
        if (fast) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const vf4_t v = *reinterpret_cast<const vf4_t*>(xc + o0 - 16 + 4 * q);
                E[4 * q] = v.x; E[4 * q + 1] = v.y; E[4 * q + 2] = v.z; E[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 32; ++j) E[j] = fir_fetch<SRC>(xc, pc, o0 - 16 + j, n, lm1, xn);
        }
#pragma unroll
        for (int j = 0; j < 24; ++j) Q[j] = vf2_t{E[j], E[j + 8]};
    }
    const long long full = taps / 16;
    for (long long t = 0;; ++t) {
        const long long u0 = 16 * t;
        const int kn = t < full ? 16 : (int)(taps - u0);   // taps in this tile
        vf2_t H[8];
        if (kn == 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const vf4_t v = *reinterpret_cast<const vf4_t*>(h + u0 + 4 * q);
                H[2 * q] = vf2_t{v.x, v.y};
                H[2 * q + 1] = vf2_t{v.z, v.w};
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const vf2_t p = (k & 1) ? pk_mul_bcast<1>(Q[16 + r - k], H[k >> 1])
                                            : pk_mul_bcast<0>(Q[16 + r - k], H[k >> 1]);
                    acc[r] = acc[r] + p;
                }
            }
        } else {   // the last, partial tile: exactly the remaining taps
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < kn) {
                    const float hk = h[u0 + k];
                    const vf2_t hh = vf2_t{hk, hk};
#pragma unroll
                    for (int r = 0; r < 8; ++r) acc[r] = acc[r] + pk_mul_bcast<0>(Q[16 + r - k], hh);
                }
            }
        }
        if (u0 + 16 >= taps) break;
        // next window: E'[j] = s[o0 - u0 - 32 + j]; Q'[16+j] = Q[j], Q'[8+j] = (N[8+j], E[j]), Q'[j] = (N[j], N[j+8])
        float N[16];
        const long long lo = ob - u0 - 32;
        const bool fast = aligned && lo >= 0 && ob + REG_TILE - u0 - 16 <= hi_ok;
        if (fast) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const vf4_t v = *reinterpret_cast<const vf4_t*>(xc + o0 - u0 - 32 + 4 * q);
                N[4 * q] = v.x; N[4 * q + 1] = v.y; N[4 * q + 2] = v.z; N[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) N[j] = fir_fetch<SRC>(xc, pc, o0 - u0 - 32 + j, n, lm1, xn);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) Q[16 + j] = Q[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) Q[8 + j] = vf2_t{N[8 + j], Q[16 + j].x};
#pragma unroll
        for (int j = 0; j < 8; ++j) Q[j] = vf2_t{N[j], N[j + 8]};
    }
    float* yc = y + c * y_stride;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const long long ia = o0 + r, ib = o0 + r + 8;
        if (ia < n) yc[REV ? n - 1 - ia : ia] = acc[r].x;
        if (ib < n) yc[REV ? n - 1 - ib : ib] = acc[r].y;
    }
}

}  // namespace vvh
