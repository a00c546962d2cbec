// hilbert_fused.hpp -- single-pass Hilbert analytic signal for gfx950: one HBM
// read of the input rows and one write of the output rows, two rows per
// complex FFT, everything else in registers/LDS.
//
// Hilbert (src/spectral/hilbert.c:14-75): z = IFFT(m . FFT(x)) with the
// one-sided mask m = 1 at DC and N/2, 2 on 1..N/2-1, 0 above, and the
// backward transform scaled by 1/N (fft_kiss.c:45,70-73).  Two real rows a, b
// share one forward FFT of a + i b; since the mask is linear,
//   w = IFFT(m . FFT(a + i b)) = za + i zb,  za = a + i ha,  zb = b + i hb,
// so  Re w = a - hb  and  Im w = ha + b:  the two analytic signals are
//   za = (a, Im w - b),  zb = (b, a - Re w)
// with a and b kept in registers.  After the forward Stockham FFT thread t
// holds Z[t + T m], exactly the input set of the inverse FFT (register
// re-index, no LDS re-order), and after the inverse it holds w[t + T m], the
// same index set as its a[m], b[m].  Replaces R2C + mask + C2C (36 B/point of
// HBM traffic) with 12 B/point.
#pragma once
#include "fft_rules.hpp"
#include "pow2_launch.hpp"

namespace vvh {

template <int N>
__global__ void __launch_bounds__(Wg<N>::value)
k_hilbert_pair(const float* __restrict__ x, float2* __restrict__ z, long long batch, long long x_dist,
               long long z_dist, const float2* gpass, const float2* gtab) {
    using G = Geo<N>;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    constexpr int LDSN = G::NPASS > 1 ? F * G::LDS : 1;
    __shared__ float2 lds[LDSN];
    __shared__ float2 ltab[TwLayout<N>::ENTRIES];
    stage_twiddles<N, WG>(ltab, gpass, gtab);
    __syncthreads();
    const TwTab<N> tw{ltab};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + (G::NPASS > 1 ? slot * G::LDS : 0);
    const long long pairs = (batch + 1) / 2;
    const float inv = 1.0f / (float)N;
    for (long long p = uni<G::T>((long long)blockIdx.x * F + slot); p < pairs; p += (long long)gridDim.x * F) {
        const long long ra = 2 * p;
        const bool hb = ra + 1 < batch;
        const float* xa = x + ra * x_dist;
        const float* xb = hb ? xa + x_dist : xa;   // unconditional loads (no exec-masked branch)
        float a[G::P], b[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            a[r] = xa[t + r * G::T];
            b[r] = xb[t + r * G::T];
        }
#pragma unroll
        for (int r = 0; r < G::P; ++r) b[r] = hb ? b[r] : 0.0f;
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = make_float2(a[r], b[r]);
        fft_regs<N, true>(v, t, my, tw);
        float2 u[G::P];
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            const int m = q / G::RL + G::NPT * (q % G::RL);   // out_pos<N>(t, q) = t + T*m
            const int k = t + G::T * m;
            const float s = (k == 0 || 2 * k == N) ? 1.0f : (2 * k < N ? 2.0f : 0.0f);
            u[m] = cscale(v[q], s);
        }
        fft_regs<N, false>(u, t, my, tw);
        float2* za = z + ra * z_dist;
        float2* zb = za + z_dist;
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            const int m = q / G::RL + G::NPT * (q % G::RL);
            const int k = t + G::T * m;
            const float2 w = cscale(u[q], inv);
            st_nt(make_float2(a[m], w.y - b[m]), za + k);
            if (hb) st_nt(make_float2(b[m], a[m] - w.x), zb + k);
        }
    }
}

// Small N (16..128) with dense rows: k_hilbert_pair's arithmetic with each wave's
// 2 x 64 / T input rows (2048 floats) loaded as 16 B per lane and re-laid through
// LDS, and its complex outputs staged the same way (even rows, then odd rows) --
// lane-strided 4 / 8 B accesses touched 16..64 lines per instruction; a
// wave-uniform loop.
template <int N>
__global__ void __launch_bounds__(256, N >= 32 ? 3 : 4)
k_hilbert_small(const float* __restrict__ x, float2* __restrict__ z, long long batch, const float2* gpass,
                const float2* gtab) {
    using G = Geo<N>;
    static_assert(G::P == 16 && G::T <= 8, "16..128 points");
    constexpr int F = 256 / G::T, WS = 64 / G::T, WF = WB_FLOATS + WB_FLOATS / 16;   // floats per wave area
    constexpr int LDSN = (F * G::LDS > 4 * WF / 2) ? F * G::LDS : 4 * WF / 2;
    __shared__ __attribute__((aligned(16))) float2 lds[LDSN];
    __shared__ float2 ltab[TwLayout<N>::ENTRIES];
    stage_twiddles<N, 256>(ltab, gpass, gtab);
    __syncthreads();
    const TwTab<N> tw{ltab};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T, wv = lt >> 6, lane = lt & 63, sl = slot - wv * WS;
    float2* my = lds + (G::NPASS > 1 ? slot * G::LDS : 0);
    float* wa = reinterpret_cast<float*>(lds) + wv * WF;
    const long long pairs = (batch + 1) / 2;
    const float inv = 1.0f / (float)N;
    for (long long pw = (long long)blockIdx.x * F + (long long)wv * WS; pw < pairs; pw += (long long)gridDim.x * F) {
        const long long r0 = 2 * pw;
        const long long nr = batch - r0 < 2 * WS ? batch - r0 : 2 * WS;
        const int nval = (int)nr * N;
        {
            vf4_t blk[WB_STEPS];
#pragma unroll
            for (int i = 0; i < WB_STEPS; ++i) blk[i] = wb_ld(x + r0 * N + wb_ef(i, lane), wb_ef(i, lane) < nval);
#pragma unroll
            for (int i = 0; i < WB_STEPS; ++i) wb_put_f(wa, wb_ef(i, lane), blk[i]);
        }
        xsync<64>();
        float a[G::P], b[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            a[r] = wa[wb_padf(2 * sl * N + t + r * G::T)];
            b[r] = wa[wb_padf((2 * sl + 1) * N + t + r * G::T)];
        }
        xsync<64>();
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = make_float2(a[r], b[r]);
        fft_regs<N, true>(v, t, my, tw);
        float2 u[G::P];
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            const int m = q / G::RL + G::NPT * (q % G::RL);   // out_pos<N>(t, q) = t + T*m
            const int k = t + G::T * m;
            const float sc = (k == 0 || 2 * k == N) ? 1.0f : (2 * k < N ? 2.0f : 0.0f);
            u[m] = cscale(v[q], sc);
        }
        fft_regs<N, false>(u, t, my, tw);
        // outputs as k_hilbert_pair (row 2 sl: (a, w.y - b), row 2 sl + 1: (b, a - w.x)),
        // staged in two passes -- the wave's even rows, then its odd rows (WS rows x N
        // complex, padded 1 per 16 in the area) -- and stored as 16 B per lane, row
        // segments of N complex
        float2* wc = reinterpret_cast<float2*>(wa);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            xsync<64>();
#pragma unroll
            for (int q = 0; q < G::P; ++q) {
                const int m = q / G::RL + G::NPT * (q % G::RL);
                const int k = t + G::T * m;
                const float2 w = cscale(u[q], inv);
                wc[G::pad(sl * N + k)] = h == 0 ? make_float2(a[m], w.y - b[m]) : make_float2(b[m], a[m] - w.x);
            }
            xsync<64>();
#pragma unroll
            for (int i = 0; i < WB_STEPS; ++i) {
                // complex index among the WS rows (wb_ec written out: through it, N = 128 compiled to other code)
                const int e = i * WB_STEP_C + WB_LANE_C * lane;
                const int row = e / N, col = e - row * N;   // N >= 16: e, e + 1 in one row
                const long long gr = r0 + 2 * row + h;      // its row of the batch
                if (gr < batch) wb_st(wb_get_c<G>(wc, e), z + gr * N + col);
            }
        }
        xsync<64>();
    }
}

bool hilbert_fused_supported(long long n) { return n >= 2 && n <= 8192 && (n & (n - 1)) == 0; }

hipError_t launch_hilbert_fused(long long n, const float* x, float2* z, long long batch, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    const long long pairs = (batch + 1) / 2;
    // 16..128 points: the staged kernel (knob HIL_SMALL = 0 keeps k_hilbert_pair, A/B)
    if (n >= 16 && n <= 128 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)z & 15) == 0 && knob(KNOB_HIL_SMALL, 1) == 1)
        return pow2_dispatch<16, 128>(n, [&](auto nn) {
            constexpr int N = decltype(nn)::value;
            const Pow2Tables tb(N);
            if (!tb.ok()) return hipErrorOutOfMemory;
            hipLaunchKernelGGL((k_hilbert_small<N>), dim3(slot_grid(pairs, 256 / Geo<N>::T, 0, false)), dim3(256), 0, s,
                               x, z, batch, tb.pass, tb.tab);
            return hipGetLastError();
        });
    return pow2_dispatch<2, 8192>(n, [&](auto nn) {
        constexpr int N = decltype(nn)::value, WG = Wg<N>::value;
        const Pow2Tables tb(N);
        if (!tb.ok()) return hipErrorOutOfMemory;
        static std::atomic<int> capc;
        const int cap = cached_grid(capc, (const void*)k_hilbert_pair<N>, WG, 0, 1LL << 40);
        // knob ANA_TPW = 1: not persistent (A/B; Hilbert 1024 / 4096 +6 %, r05_ab2_analytic_mixed_grid)
        const int grid = slot_grid(pairs, Wg<N>::F, cap, knob(KNOB_ANA_TPW, 0) != 1);
        hipLaunchKernelGGL(k_hilbert_pair<N>, dim3(grid), dim3(WG), 0, s, x, z, batch, n, n, tb.pass, tb.tab);
        return hipGetLastError();
    });
}

}  // namespace vvh
