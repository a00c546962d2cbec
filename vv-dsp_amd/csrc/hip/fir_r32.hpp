// fir_r32.hpp -- k_fir_r32: overlap-save at N = 1024 with the transforms split
// 32 x 32 on half-waves, the default for taps <= 257 (instantiated by fir_1024.hip).
#pragma once
#include "fir_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// k_fir_r32: config 4's overlap-save (N = 1024, LE = 256, LOUT = 768) with the
// 1024-point transforms split 32 x 32 instead of 16 x 16 x 4, so each FFT
// crosses LDS ONCE (a 32 x 32 transpose) instead of twice.  The FFTs of
// k_fir_bulk_reg are LDS-bound (each exchange moves 8 KB through a ~80 B/clk
// write path per CU; four exchanges per pair): this halves the exchanges.
//
// A transform lives on 32 lanes (32 points per lane), so a wave runs two pairs
// at once, one per half.  Forward, for z[n] = a[n] + i b[n], n = 32 m1 + m2:
//   lane m2: DFT_32 over m1 (registers) -> k1, times W_1024^(m2 k1)
//   transpose through LDS (row k1, column m2; rows padded to 33: conflict-free)
//   lane k1: DFT_32 over m2 -> X[k1 + 32 k2] in register k2.
// The product with H (f < 512: H[f], else conj H[1024 - f]) keeps that
// layout, and the inverse runs the same two steps mirrored:
//   lane k1: IDFT_32 over k2 -> a, times conj W_1024^(k1 a)
//   transpose; lane a: IDFT_32 over k1 -> b:  y[a + 32 b] in register b,
// so the 768 outputs of a block (e = a + 32 b >= 256, b >= 8) leave as 24
// lane-contiguous dword stores per block.  Each lane keeps its 31 twiddles
// W_1024^(m r) come from an LDS table [r][m] (consecutive lanes, consecutive
// words) and the next pair's 64 samples are loaded during the current pair's
// transforms: two waves per SIMD (launch bounds 256, 2); exchange buffers
// 66 KB + H 4 KB + twiddles 8 KB per workgroup, two workgroups per CU.
// Edge pairs (span before sample 0 or past n) load through the prefix / zero
// rule and store predicated, in the same loop (a wave-uniform branch).
// Walk: each XCD group takes one contiguous eighth of the couples (xcd_walk), so
// neighbouring blocks' overlap comes from that XCD's L2 (a grid-wide front
// measured 0.2517 vs 0.2019 ms, profiles/r04_kbench_fir_walk.jsonl).
// PAIRED (the launcher's choice for 8 B aligned channels): bulk samples move as 8 B per lane -- a block's 1024 inputs as 16
// dwordx2 loads (rows 0..7 of block b are rows 24..31 of block a: 12 more), its
// 768 outputs as 12 dwordx2 stores -- each pair of dwords re-laid by one
// v_permlane16_swap (r32_pairswap): lane l of a half works on residue
// 2 (l & 15) + (l >> 4) instead of l, which only moves its forward-twiddle column
// and the rows the transposes use.  Needs 8 B aligned channels (x, y and
// their strides even).
// ------------------------------------------------------------------------
template <bool PAIRED>
__global__ void __launch_bounds__(256, 2)
k_fir_r32(const float2* Hg, const float* x, float* y, long long nch, long long x_stride, long long y_stride,
          long long ppc, const float2* tw1024, long long n, const float* prefix, long long lm1, long long qf,
          long long ql) {
    constexpr int N = 1024, LE = 256, LOUT = N - LE, F = 4;
    __shared__ __attribute__((aligned(16))) float2 xch[F * 2 * R32_BUF];
    __shared__ float2 lH[N / 2 + 1];
    __shared__ float2 ltw[32 * 32];   // [r][m] = W_1024^(m r) (row 0 unused)
    for (int i = threadIdx.x; i <= N / 2; i += 256) lH[i] = Hg[i];
    for (int i = threadIdx.x; i < 32 * 32; i += 256) ltw[i] = tw1024[((i & 31) * (i >> 5)) & (N - 1)];
    const int lt = threadIdx.x, slot = lt >> 6, lane = lt & 63, half = lane >> 5, m = lane & 31;
    float2* buf = xch + (2 * slot + half) * R32_BUF;
    // the lane's residue: input / output samples 32 r + mr in register r
    const int mr = PAIRED ? 2 * (m & 15) + (m >> 4) : m;
    const float2* atwf = ltw + mr;      // + 32 r: W_1024^(mr r), forward (lane = input residue)
    const float2* atw = ltw + m;        // + 32 r: W_1024^(m r), inverse (lane = bin residue)
    const float2* ahl = lH + m;         // + 32 k2: H[m + 32 k2], k2 < 16
    const float2* ahh = lH + 32 - m;    // + 32 (31 - k2): H[1024 - m - 32 k2]
    __syncthreads();
    const long long pairs = nch * ppc, couples = (pairs + 1) / 2;
    long long it, it_end, it_step;
    xcd_walk(couples, F, slot, &it, &it_end, &it_step);
    it = uni<64>(it);
    it_end = uni<64>(it_end);
    it_step = uni<64>(it_step);
    if (it < it_end) {
    // couple k: pairs 2k (lanes 0..31) and 2k+1 (lanes 32..63); a missing
    // second pair (odd total) computes pair 2k again and stores nothing.
    // Pair 2k = (channel c0, pair q0 of it), kept incrementally for the static
    // walk (one division per wave, not three per couple).
    long long c0 = 0, q0 = 0, dc = 0, dq = 0;
    auto seek = [&](long long k) {
        c0 = (2 * k) / ppc;
        q0 = 2 * k - c0 * ppc;
    };
    auto locate = [&](long long k, long long* c, long long* j, bool* valid, bool* edge_any) {
        const bool two = 2 * k + 1 < pairs;
        const bool wrap = q0 + 1 == ppc;
        const long long c1 = two ? c0 + (wrap ? 1 : 0) : c0, q1 = two ? (wrap ? 0 : q0 + 1) : q0;
        *valid = !half || two;
        *c = half ? c1 : c0;
        *j = 2 * (half ? q1 : q0);
        *edge_any = q0 < qf || q0 >= ql || q1 < qf || q1 >= ql;
    };
    auto advance = [&]() {   // (c0, q0) of couple k + it_step from those of k
        q0 += dq;
        c0 += dc;
        if (q0 >= ppc) {
            q0 -= ppc;
            ++c0;
        }
    };
    dc = (2 * it_step) / ppc;
    dq = 2 * it_step - dc * ppc;
    seek(it);
    float xa[32], xb[32];
    auto load_bulk = [&](long long c, long long j) {
        if constexpr (PAIRED) {
            // 8 B pairs (samples 64 i + 2m, +1), swapped into the residue layout at use
            const float2* a = reinterpret_cast<const float2*>(x + c * x_stride + j * LOUT - LE) + m;
            const float2* b = a + LOUT / 2;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float2 u = ld_nt(a + 32 * i);
                xa[2 * i] = u.x;
                xa[2 * i + 1] = u.y;
            }
#pragma unroll
            for (int i = 4; i < 16; ++i) {   // rows 0..7 of block b = rows 24..31 of block a
                const float2 u = b[32 * i];    // overlaps the next pair's block a: cached
                xb[2 * i] = u.x;
                xb[2 * i + 1] = u.y;
            }
        } else {
            const float* a = x + c * x_stride + j * LOUT - LE + m;
            const float* b = a + LOUT;
#pragma unroll
            for (int r = 0; r < 32; ++r) xa[r] = __builtin_nontemporal_load(a + 32 * r);
#pragma unroll
            for (int r = 0; r < 32; ++r) xb[r] = b[32 * r];   // overlaps the next pair's block a: cached
        }
    };
    // edge couples: staged through the (idle) exchange buffer with rolled loops
    // (fir_fetch<0> per sample), then read back -- no register
    // array is indexed by a loop variable, and nothing else is live here
    auto load_edge = [&](long long c, long long j) {
        const float* xs = x + c * x_stride;
        const float* pre = prefix ? prefix + c * lm1 : nullptr;
        float* sf = reinterpret_cast<float*>(buf);
        const long long s0 = j * LOUT - LE;
#pragma unroll 1
        for (int k = m; k < 2 * N; k += 32) sf[k] = fir_fetch<0>(xs, pre, s0 + (k < N ? k : k - N + LOUT), n, lm1, n);
        xsync<64>();
#pragma unroll
        for (int r = 0; r < 32; ++r) xa[r] = sf[mr + 32 * r];
#pragma unroll
        for (int r = 0; r < 32; ++r) xb[r] = sf[N + mr + 32 * r];
        xsync<64>();
    };
    long long c, j;
    bool valid, edge;
    locate(it, &c, &j, &valid, &edge);
    if (!edge) load_bulk(c, j);
    for (; it < it_end; it += it_step) {
        if (edge) {
            load_edge(c, j);   // at the top of its own iteration (a bulk couple was prefetched)
        } else if constexpr (PAIRED) {
#pragma unroll
            for (int i = 0; i < 16; ++i) r32_pairswap(xa[2 * i], xa[2 * i + 1]);
#pragma unroll
            for (int i = 4; i < 16; ++i) r32_pairswap(xb[2 * i], xb[2 * i + 1]);
        }
        float2 v[32];
        if constexpr (PAIRED) {
            // v[r] = (block a row r, block b row r); block b's rows 0..7 are block a's
            // rows 24..31 (edge couples too: the same sample indices)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const vf2_t A = {xa[2 * i], xa[2 * i + 1]};
                const vf2_t B = i < 4 ? vf2_t{xa[24 + 2 * i], xa[25 + 2 * i]} : vf2_t{xb[2 * i], xb[2 * i + 1]};
                v[2 * i] = upk(pk_pair<0>(A, B));
                v[2 * i + 1] = upk(pk_pair<1>(A, B));
            }
        } else {
#pragma unroll
            for (int r = 0; r < 32; ++r) v[r] = make_float2(xa[r], xb[r]);
        }
        const long long itn = it + it_step;
        long long cn = c, jn = j;
        bool validn = valid, edgen = edge;
        if (itn < it_end) {   // the next couple's loads, in flight across this one's transforms
            advance();
            locate(itn, &cn, &jn, &validn, &edgen);
            if (!edgen) load_bulk(cn, jn);
        }
        {
            // forward: DFT over m1, twiddle, transpose, DFT over m2 -> X[m + 32 k2] in v[k2]
            dft32<true>(v);
            r32_twiddle<true>(v, atwf);
            r32_transpose(v, buf, mr, m);
            dft32<true>(v);
            // times H: bin f = m + 32 k2 (H[f] for f < 512, conj H[1024 - f] above)
            {
                float2 h[16];
                lds_rd64x16<0, 256>(ahl, h);   // H[m + 32 k2], k2 < 16
#pragma unroll
                for (int k2 = 0; k2 < 16; ++k2) v[k2] = cmul(v[k2], h[k2]);
                lds_rd64x16<15 * 256, -256>(ahh, h);   // h[i] = H[1024 - m - 32 (16 + i)]
#pragma unroll
                for (int i = 0; i < 16; ++i) v[16 + i] = cmulc(v[16 + i], h[i]);
            }
            // inverse: IDFT over k2, conj twiddle, transpose, IDFT over k1 -> y[m + 32 b] in v[b]
            dft32<false>(v);
            r32_twiddle<false>(v, atw);
            r32_transpose(v, buf, m, mr);
            dft32<false>(v);
        }
        {
            float* ya = y + c * y_stride + j * LOUT - LE + mr;   // + 32 b: block j's output (b >= 8)
            if (!edge) {
                if constexpr (PAIRED) {
                    // rows b, b + 1 -> 8 B pairs: lane l < 16 stores samples 32 b + 2l, +1,
                    // lane l + 16 samples 32 (b + 1) + 2l, +1
                    float2 oa[12], ob[12];   // (row b, row b + 1) of block a / block b
#pragma unroll
                    for (int i = 0; i < 12; ++i) {
                        oa[i] = upk(pk_pair<0>(pk(v[8 + 2 * i]), pk(v[9 + 2 * i])));
                        ob[i] = upk(pk_pair<1>(pk(v[8 + 2 * i]), pk(v[9 + 2 * i])));
                        r32_pairswap(oa[i].x, oa[i].y);
                        r32_pairswap(ob[i].x, ob[i].y);
                    }
                    float2* yp = reinterpret_cast<float2*>(y + c * y_stride + j * LOUT - LE) + (m & 15) + 16 * (m >> 4);
                    if (valid) {
#pragma unroll
                        for (int i = 0; i < 12; ++i) st_nt(oa[i], yp + 16 * (8 + 2 * i));
#pragma unroll
                        for (int i = 0; i < 12; ++i) st_nt(ob[i], yp + LOUT / 2 + 16 * (8 + 2 * i));
                    }
                } else if (valid) {
#pragma unroll
                    for (int b = 8; b < 32; ++b) __builtin_nontemporal_store(v[b].x, ya + 32 * b);
#pragma unroll
                    for (int b = 8; b < 32; ++b) __builtin_nontemporal_store(v[b].y, ya + LOUT + 32 * b);
                }
            } else if (valid) {   // outputs past n are not stored
                const long long rem = n - (j * LOUT - LE + mr);
                const int rm = (int)(rem < (1 << 30) ? rem : (1 << 30));
#pragma unroll
                for (int b = 8; b < 32; ++b) {
                    if (32 * b < rm) ya[32 * b] = v[b].x;
                    if (32 * b + LOUT < rm) ya[LOUT + 32 * b] = v[b].y;
                }
            }
        }
        c = cn;
        j = jn;
        valid = validn;
        edge = edgen;
    }
    }
}

}  // namespace vvh
