// fir_pair.hpp -- FFT-domain FIR (overlap-save) for gfx950, every block size:
// k_fir_pair (instantiated by fir_ols.hip).
//
// vv_dsp_fir_apply_fft (src/filter/fir.c:75-135) is "the first n samples of the
// linear convolution with zero initial state"; vv_dsp_fir_apply (:160-196) is
// the same convolution continued from a (taps-1)-sample history.  Both are
// computed here as overlap-save with blocks of N real samples and an
// effective history LE >= taps-1 (the filter read as zero-padded to LE+1 taps,
// which changes nothing; LE is a multiple of 4 and >= N/4 so that block starts
// are 16 B aligned and a pair's input span fits its LDS buffer):
//
//   block j of channel c covers input samples [j*Lout - LE, j*Lout + Lout)
//   (Lout = N - LE); samples before 0 come from `prefix` (history) or are 0;
//   outputs j*Lout + [0, Lout) are the block's circular-convolution samples
//   LE .. N-1.
//
// Two real blocks per complex FFT: z = a + i b (blocks j and j+1), then
// Y = FFT(z) * H with H = FFT(h)/N over all N bins, and y = IFFT(Y) holds
// a*h in its real part and b*h in its imaginary part (h is real, so the
// product keeps the two convolutions apart -- no split step).  After the
// forward Stockham FFT thread t holds Z[t + T*m] for m < P, which is exactly
// the input set of the inverse transform: the multiply by H re-indexes
// registers and no LDS re-order is needed between the two transforms.
//
// k_fir_pair<N, true>  (bulk, T >= 64): the pair's input span comes HBM -> LDS
//   by 16 B/lane LDS-DMA issued one pair ahead with a hand-counted vmcnt;
//   outputs are dword stores of which lanes below LE go to a write sink, so
//   every pair issues exactly 2P stores.
// k_fir_pair<N, false> (edges and small N): register loads with the prefix /
//   zero padding, predicated stores.
// HBM traffic: the signal read once (the LE overlap comes from L2/LDS), the
// output written once -- 8 B per sample.
#pragma once
#include "fir_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// samples s0 + t + r*T of one block (fir_fetch<0>: prefix before 0, zero past n)
template <int N>
__device__ __forceinline__ void fir_blk_load(float* xr, const float* xs, const float* pre, long long s0,
                                             long long n, long long lm1, int t) {
    using G = Geo<N>;
    if (s0 >= 0 && s0 + N <= n) {
        const float* b = xs + s0;
#pragma unroll
        for (int r = 0; r < G::P; ++r) xr[r] = b[t + r * G::T];
    } else {
#pragma unroll
        for (int r = 0; r < G::P; ++r) xr[r] = fir_fetch<0>(xs, pre, s0 + t + r * G::T, n, lm1, n);
    }
}

// Y = Z * H with the register re-index forward-output -> inverse-input
template <int N>
__device__ __forceinline__ void fir_multiply(const float2* v, float2* u, const float2* lH, int t) {
    using G = Geo<N>;
#pragma unroll
    for (int q = 0; q < G::P; ++q) {
        const int m = q / G::RL + G::NPT * (q % G::RL);   // out_pos<N>(t, q) = t + T*m
        u[m] = cmul(v[q], lH[t + G::T * m]);
    }
}

// Pairs of channel c handled by a launch: idx < qlo -> pair idx, else pair
// qhi + (idx - qlo); cnt = pairs per channel in this launch.
template <int N, bool BULK>
__global__ void __launch_bounds__(Wg<N>::value)
k_fir_pair(long long lm1, long long le, const float2* Hg, const float* x, float* y, long long n,
           long long nch, long long x_stride, long long y_stride, const float* prefix, long long cnt,
           long long qlo, long long qhi, const float2* gpass, const float2* gtab, float* sink, long long chunk) {
    using G = Geo<N>;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    constexpr int SPAN = BULK ? N + (3 * N) / 4 : 1;   // N + Lout, Lout <= 3N/4
    constexpr int NST = 2 * G::P;                      // stores per pair (bulk)
    static_assert(!BULK || G::T >= 64, "LDS-DMA spans need whole waves per transform");
    __shared__ float2 lds[F * G::LDS];
    __shared__ float2 ltab[TwLayout<N>::ENTRIES];
    __shared__ float2 lH[N];
    __shared__ float span_all[BULK ? F * SPAN : 1];
    stage_twiddles<N, WG>(ltab, gpass, gtab);
    for (int i = threadIdx.x; i < N; i += WG) lH[i] = Hg[i];
    __syncthreads();
    const TwTab<N> tw{ltab};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + slot * G::LDS;
    const long long lout = N - le;
    long long p, p_end, p_step;
    work_walk(nch * cnt, F, slot, chunk, &p, &p_end, &p_step);
    p = uni<G::T>(p);
    p_end = uni<G::T>(p_end);
    p_step = uni<G::T>(p_step);
    if (p >= p_end) return;   // uniform per transform (F == 1 whenever T > 64)
    // item -> (channel, first block of the pair)
    auto locate = [&](long long it, long long* cc, long long* jj) {
        *cc = it / cnt;
        const long long i = it - *cc * cnt;
        *jj = 2 * (i < qlo ? i : qhi + (i - qlo));
    };
    long long c, j;
    locate(p, &c, &j);
    if constexpr (BULK) {
        float* span = span_all + slot * SPAN;
        float* snk = sink + ((((long long)blockIdx.x * (WG / 64) + (lt >> 6)) * 64) % SINK_FLOATS) + (lt & 63);
        auto issue_span = [&](long long cc, long long jj) {
            const float* s0 = x + cc * x_stride + jj * lout - le;
            const int len = (int)(N + lout), lane = t & 63;
            for (int u = t >> 6; u * 256 < len; u += G::T / 64) {
                const int e = u * 256 + lane * 4;
                glds16(s0 + (e < len ? e : 0), span + u * 256);
            }
        };
        issue_span(c, j);
        vm_wait<0>();
        for (; p < p_end; p += p_step) {
            const bool more = p + p_step < p_end;
            long long cn = c, jn = j;
            if (more) locate(p + p_step, &cn, &jn);
            vm_wait<NST>();   // younger than this span's DMA: the previous pair's stores
            if constexpr (G::T > 64) lds_barrier();
            float2 v[G::P];
#pragma unroll
            for (int r = 0; r < G::P; ++r) v[r] = make_float2(span[t + r * G::T], span[lout + t + r * G::T]);
            lgkm_wait0();
            if constexpr (G::T > 64) lds_barrier();
            if (more) issue_span(cn, jn);
            fft_regs<N, true>(v, t, my, tw);
            float2 u[G::P];
            fir_multiply<N>(v, u, lH, t);
            fft_regs<N, false>(u, t, my, tw);
            float* ya = y + c * y_stride + j * lout - le;   // + e: block j output (e >= le)
#pragma unroll
            for (int q = 0; q < G::P; ++q) {
                const long long e = out_pos<N>(t, q);
                const bool ok = e >= le;
                st4_counted(ok ? ya + e : snk, u[q].x);
                st4_counted(ok ? ya + e + lout : snk, u[q].y);
            }
            c = cn;
            j = jn;
        }
    } else {
        float xa[G::P], xb[G::P];
        auto load_pair = [&](long long cc, long long jj) {
            const float* xs = x + cc * x_stride;
            const float* pre = prefix ? prefix + cc * lm1 : nullptr;
            fir_blk_load<N>(xa, xs, pre, jj * lout - le, n, lm1, t);
            fir_blk_load<N>(xb, xs, pre, (jj + 1) * lout - le, n, lm1, t);
        };
        load_pair(c, j);
        for (; p < p_end; p += p_step) {
            float2 v[G::P];
#pragma unroll
            for (int r = 0; r < G::P; ++r) v[r] = make_float2(xa[r], xb[r]);
            const bool more = p + p_step < p_end;
            long long cn = c, jn = j;
            if (more) {
                locate(p + p_step, &cn, &jn);
                load_pair(cn, jn);
            }
            fft_regs<N, true>(v, t, my, tw);
            float2 u[G::P];
            fir_multiply<N>(v, u, lH, t);
            fft_regs<N, false>(u, t, my, tw);
            float* ys = y + c * y_stride;
            const long long oa0 = j * lout - le;
#pragma unroll
            for (int q = 0; q < G::P; ++q) {
                const long long e = out_pos<N>(t, q);
                if (e >= le) {
                    const long long oa = oa0 + e, ob = oa + lout;
                    if (oa < n) ys[oa] = u[q].x;
                    if (ob < n) ys[ob] = u[q].y;
                }
            }
            c = cn;
            j = jn;
        }
    }
}

}  // namespace vvh
