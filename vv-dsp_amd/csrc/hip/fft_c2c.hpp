// fft_c2c.hpp -- k_c2c, the batched power-of-two C2C kernel for gfx950
// (launched from fft_c2c.hip).
//
// Power-of-two lengths use the persistent register/LDS Stockham kernels of
// fft_core.hpp: each slot (a wave, or the whole block for N >= 2048) loops over
// transforms with the NEXT transform's points prefetched into a second register
// set, reading one transform with lane-contiguous loads and writing it with
// lane-contiguous stores: one HBM read + one HBM write per transform
// (8 B/point each way for C2C).  Twiddle tables live in LDS, so vmcnt only
// waits on streamed data.
#pragma once
#include "fft_rules.hpp"

namespace vvh {

// The exchange reads are single ds_read_b32 into the complex register pairs
// (pass_exchange_ri RIV 1; the compiler's ds_read2 pairs and v_movs measured
// 0.1850 vs 0.1827 ms on the same buffers, profiles/r04_kbench_riv_ab.jsonl).
// (Two transforms per loop trip with alternating prefetch buffers, to drop the
// loop-carried copy, spilled at the 128 VGPRs of four waves per SIMD.)  A grid-
// wide interleaved front: per-XCD eighths measured 0.1992 vs 0.1836 ms
// (profiles/r04_kbench_c2c_walk.jsonl).
// N = 1024 exchanges through the half-size real/imaginary buffer
// (pass_exchange_ri): 26 KB of LDS per workgroup instead of 43 KB, so four
// workgroups (16 waves) fit per CU and keep more transforms' loads in flight.
template <int N, bool FWD, bool ONE = false>
__global__ void __launch_bounds__(Wg<N>::value, (N == 1024 || (ONE && N >= 16 && N <= 128)) ? 4 : 1)
k_c2c(const float2* in, float2* out, long long batch, long long in_dist, long long out_dist,
      const float2* gpass, const float2* gtab, float scale) {
    using G = Geo<N>;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    constexpr bool RI = N == 1024;
    constexpr int XF = RI ? ri_floats<N>() / 2 : G::LDS;   // float2 per transform
    // ONE with 16..128 points: each wave's 1024-point block staged through LDS
    constexpr bool SMALL = ONE && G::T < 16 && G::P == 16;
    constexpr int LDSX = G::NPASS > 1 ? F * XF : 1, LDSN = SMALL && F * G::LDS > LDSX ? F * G::LDS : LDSX;
    __shared__ __attribute__((aligned(16))) float2 lds[LDSN];
    __shared__ float2 ltab[TwLayout<N>::ENTRIES];
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + (G::NPASS > 1 ? slot * XF : 0);
    const TwTab<N> tw{ltab};
    const long long fend = batch;
    if constexpr (SMALL) {
        // small N (16..128): a wave's 64 / T transforms are 1024 consecutive points
        // (8 KB).  Lane-strided loads would touch 16..64 lines per instruction, so
        // the block moves as 16 B per lane, coalesced, and is re-laid through the
        // wave's LDS area (its slots' exchange buffers, padded 1 per 16) in both
        // directions.  The host takes this only for dense rows (dist == N).
        constexpr int WS = 64 / G::T;   // transforms per wave
        const int wv = lt >> 6, lane = lt & 63, sl = slot - wv * WS;
        const long long fw = (long long)blockIdx.x * F + (long long)wv * WS;   // the wave's first transform
        const long long nvl = fend - fw < WS ? fend - fw : WS;                   // its transforms in the batch
        const int nval = nvl > 0 ? (int)nvl * N : 0;                            // valid points of the block
        float2* wa = lds + wv * WS * G::LDS;                                    // the wave's LDS area
        stage_twiddles<N, WG>(ltab, gpass, gtab);
        __syncthreads();
        if (nval == 0) return;
        {
            vf4_t blk[WB_STEPS];
#pragma unroll
            for (int i = 0; i < WB_STEPS; ++i) blk[i] = wb_ld(in + fw * N + wb_ec(i, lane), wb_ec(i, lane) < nval);
#pragma unroll
            for (int i = 0; i < WB_STEPS; ++i) wb_put_c<G>(wa, wb_ec(i, lane), blk[i]);
        }
        xsync<64>();
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = wa[G::pad(sl * N + t + r * G::T)];
        xsync<64>();   // the FFT's exchanges reuse the area
        fft_regs<N, FWD, false, RI, TwTab<N>, false, false, 1>(v, t, my, tw);
        xsync<64>();
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            wa[G::pad(sl * N + out_pos<N>(t, q))] = c2c_out<FWD>(v[q], scale);
        }
        xsync<64>();
#pragma unroll
        for (int i = 0; i < WB_STEPS; ++i) {
            const int e = wb_ec(i, lane);
            if (e < nval) wb_st(wb_get_c<G>(wa, e), out + fw * N + e);
        }
        return;
    } else if constexpr (ONE) {
        // one transform per slot, no loop and no prefetch registers.  One-wave
        // transforms (N <= 1024) issue their loads before the block stages its
        // twiddles, so the load latency overlaps the staging: 1024 points 0.1815 ->
        // 0.1739 ms, 256 -1.8 %; for 2048 / 4096 (a transform over several waves)
        // that order measured +23 % / +2 %, so they load after the barrier
        // (profiles/r05_ab2_c2c_grid.jsonl)
        constexpr bool EARLY = G::T <= 64;
        const long long f = uni<G::T>((long long)blockIdx.x * F + slot);
        const bool act = f < fend;
        float2 v[G::P];
        if (EARLY && act) rows_load<N>(v, in + f * in_dist, t);
        stage_twiddles<N, WG>(ltab, gpass, gtab);
        __syncthreads();
        if (!act) return;
        if constexpr (!EARLY) rows_load<N>(v, in + f * in_dist, t);
        fft_regs<N, FWD, false, RI, TwTab<N>, false, false, 1>(v, t, my, tw);
        float2* dst = out + f * out_dist;
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            st_nt(c2c_out<FWD>(v[q], scale), dst + out_pos<N>(t, q));
        }
        return;
    }
    stage_twiddles<N, WG>(ltab, gpass, gtab);
    __syncthreads();
    const long long stride = (long long)gridDim.x * F;
    long long f = uni<G::T>((long long)blockIdx.x * F + slot);
    float2 nx[G::P];
    if (f < fend) rows_load<N>(nx, in + f * in_dist, t);
    for (; f < fend; f += stride) {
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = nx[r];
        const long long fn = f + stride;
        if (fn < fend) rows_load<N>(nx, in + fn * in_dist, t);
        fft_regs<N, FWD, false, RI, TwTab<N>, false, false, 1>(v, t, my, tw);
        float2* dst = out + f * out_dist;
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            st_nt(c2c_out<FWD>(v[q], scale), dst + out_pos<N>(t, q));
        }
    }
}

}  // namespace vvh
