// istft_kernels.hip -- STFT synthesis: overlap-add of inverse-transformed frames
// (k_ola), and the inverse FFT, window and overlap-add in one pass (k_istft).
#include "fft_core.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ISTFT accumulate for `count` frames placed at multiples of hop (stft.c:95-110
// applied frame after frame).  One thread per output sample sums its frames in
// frame order, so the f32 rounding matches sequential accumulation.
__global__ void k_ola(long long nfft, long long hop, const float2* tf, long long count,
                      const float* win, float* out_add, float* norm_add, long long len) {
    VVH_GRID_STRIDE(i, len) {
        long long f_hi = i / hop;
        if (f_hi > count - 1) f_hi = count - 1;
        long long f_lo = (i - nfft + 1 + hop - 1) / hop;
        if (i - nfft + 1 <= 0) f_lo = 0;
        float acc = out_add[i];
        float nacc = norm_add ? norm_add[i] : 0.0f;
        for (long long f = f_lo; f <= f_hi; ++f) {
            const long long e = i - f * hop;
            if (e < 0 || e >= nfft) continue;
            const float w = win[e];
            float c = tf[f * nfft + e].x * w, w2 = w * w;
            asm volatile("" : "+v"(c), "+v"(w2));   // products rounded before the adds (no FMA), as stft.c
            acc += c;
            nacc += w2;
        }
        out_add[i] = acc;
        if (norm_add) norm_add[i] = nacc;
    }
}

// ------------------------------------------------------------------------
// k_istft<N>: inverse FFT + window + overlap-add of `count` frames in one pass
// (stft.c:95-110 applied frame after frame), N = 1024, hop | N, K = N/hop <= 4.
// Only Re(IFFT(X)) is used, and Re(IFFT(X)) = IFFT of the Hermitian part
// (X[k] + conj X[N-k])/2, so two frames share one complex inverse FFT:
// Z = Ha + i Hb gives frame a's samples in Re z and frame b's in Im z.
// A workgroup (4 waves = 8 frames per step) owns the frames [fa, fb) and the
// output hop-blocks [fa, fb) (the last one also the K-1 tail blocks), computes
// K-1 frames before fa as halo, and finalises each block once all of its
// frames are in: out_add[i] + c_{b-K+1} + ... + c_b in frame order, products
// re*w and w*w rounded before they are added -- the f32 rounding of the
// sequential loop.  Blocks still open after a step (the K-1 newest) are
// carried in LDS.  The windowed real parts of a step's 8 frames sit in LDS; a
// wave's FFT exchange reuses its own 2 frames' area.
// Traffic: the spectrum read once (8 B per bin), out_add (and norm_add) read
// and written once -- against ~3x that for IFFT-to-scratch + a separate OLA.
// (Measured variants: one frame per wave with the next frame's spectrum
// prefetched in registers, and a compile-time hop with batched accumulator
// loads, both ran slower -- 0.59-0.65 vs 0.44 ms for 600 s at hop 256.)
// ------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(256, 3)
k_istft(const float2* __restrict__ spec, long long count, int hop, int K, const float* __restrict__ win,
        float* __restrict__ out_add, float* __restrict__ norm_add, long long run, const float2* gpass) {
    using G = Geo<N>;
    static_assert(G::T == 64 && ri_floats<N>() <= 2 * N, "one wave per transform; exchange fits two frames");
    constexpr int TWL = G::tw_off(G::NPASS - 1) > 0 ? G::tw_off(G::NPASS - 1) : 1;
    __shared__ __attribute__((aligned(16))) float stage[8 * N];
    __shared__ float carry[N], ncarry[N];
    __shared__ float lwin[N];
    __shared__ float2 ltab[TWL];
    const int tid = threadIdx.x, wv = tid >> 6, t = tid & 63;
    for (int i = tid; i < G::tw_off(G::NPASS - 1); i += 256) ltab[i] = gpass[i];
    for (int i = tid; i < N; i += 256) lwin[i] = win[i];
    TwLastReg<N> tw;
    tw.tab = ltab;
    tw.load(gpass, t);
    __syncthreads();
    const long long fa = (long long)blockIdx.x * run;
    const long long fb = fa + run < count ? fa + run : count;
    const long long bend = fb == count ? count + K - 1 : fb;   // blocks this workgroup writes: [fa, bend)
    const long long g0 = fa - (K - 1);
    const float sc = 0.5f / (float)N;   // Hermitian half and the backward 1/N, exact (powers of two)
    const int lh = 31 - __builtin_clz((unsigned)hop);   // hop is a power of two (istft_fused_supported)
    float* my = stage + 2 * wv * N;
    for (long long g = g0; g < fb; g += 8) {
        // ---- two frames per wave: Z = Ha + i Hb, inverse FFT, window -> stage
        const long long f0 = uni<64>(g + 2 * wv);   // wave-uniform: SGPR row bases, 32-bit lane offsets
        const bool va = f0 >= 0 && f0 < fb, vb = f0 + 1 >= 0 && f0 + 1 < fb;
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = make_float2(0.0f, 0.0f);
        if (va) {
            const float2* xa = spec + f0 * N;
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                const int k = t + 64 * r;
                const float2 A = xa[k], Am = xa[(N - k) & (N - 1)];
                v[r] = make_float2((A.x + Am.x) * sc, (A.y - Am.y) * sc);   // Ha
            }
        }
        if (vb) {
            const float2* xb = spec + (f0 + 1) * N;
#pragma unroll
            for (int r = 0; r < G::P; ++r) {
                const int k = t + 64 * r;
                const float2 B = xb[k], Bm = xb[(N - k) & (N - 1)];
                const float2 hb = make_float2((B.x + Bm.x) * sc, (B.y - Bm.y) * sc);
                v[r] = make_float2(v[r].x - hb.y, v[r].y + hb.x);   // + i Hb
            }
        }
        tw.opaque();
        fft_regs<N, false, false, true>(v, t, reinterpret_cast<float2*>(my), tw);
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            const int e = out_pos<N>(t, q);
            const float w = lwin[e];
            float ca = v[q].x * w, cb = v[q].y * w;
            asm volatile("" : "+v"(ca), "+v"(cb));   // re*w rounded before it is added
            my[e] = ca;
            my[N + e] = cb;
        }
        __syncthreads();
        // ---- combine: sum of block b's contributions of this step's frames, in frame order
        // ---- combine: sum of block b's contributions of this step's frames, in
        // frame order.  All per-sample index math is 32-bit and relative to the
        // step (block bb = b - g, frame r = f - g; hop is a power of two), with
        // the 64-bit bounds folded into uniform per-step limits.
        auto clampi = [](long long v) { return (int)(v < -(1LL << 30) ? -(1LL << 30) : (v > (1LL << 30) ? (1LL << 30) : v)); };
        const long long gh = g * hop;                           // sample index of block g
        const int rflo = g < 0 ? (int)(-g) : 0;                  // frames f >= 0
        const int rfhi = (int)(fb - 1 - g < 7 ? fb - 1 - g : 7);   // frames f < fb of this step
        const int bb_fa = clampi(fa - g), bb_bend = clampi(bend - g), bb_tot = clampi(count + K - 1 - g);
        auto combine = [&](int bb, int j, float acc, float nacc, float* acc_o, float* nacc_o) {
            int rlo = bb - K + 1;
            if (rlo < rflo) rlo = rflo;
            const int rhi = bb < rfhi ? bb : rfhi;
            for (int r = rlo; r <= rhi; ++r) {
                const int e = ((bb - r) << lh) + j;
                acc += stage[r * N + e];
                const float w = lwin[e];
                float w2 = w * w;
                asm volatile("" : "+v"(w2));   // no FMA: w*w rounded, then added (stft.c)
                nacc += w2;
            }
            *acc_o = acc;
            *nacc_o = nacc;
        };
        // Both phases read their out_add / norm_add words for eight samples per
        // thread before combining any (one memory latency per chunk instead of
        // one per sample: the loop body's load -> add -> store chain otherwise
        // serialises them).
        constexpr int CH = 8;
        for (int base = 0; base < 8 * hop; base += 256 * CH) {   // phase A: blocks [g, g+8) become final
            float a0[CH], n0[CH];
#pragma unroll
            for (int s = 0; s < CH; ++s) {
                const int idx = base + tid + 256 * s, bb = idx >> lh;
                const bool ok = idx < 8 * hop && bb >= bb_fa && bb < bb_bend && bb < bb_tot;
                const bool fresh = g == g0 || bb >= K - 1;
                a0[s] = ok ? (fresh ? out_add[gh + idx] : carry[idx]) : 0.0f;
                n0[s] = ok && norm_add ? (fresh ? norm_add[gh + idx] : ncarry[idx]) : 0.0f;
            }
#pragma unroll
            for (int s = 0; s < CH; ++s) {
                const int idx = base + tid + 256 * s, bb = idx >> lh, j = idx & (hop - 1);   // idx = bb * hop + j
                if (idx >= 8 * hop || bb < bb_fa || bb >= bb_bend || bb >= bb_tot) continue;
                float acc, nacc;
                combine(bb, j, a0[s], n0[s], &acc, &nacc);
                out_add[gh + idx] = acc;
                if (norm_add) norm_add[gh + idx] = nacc;
            }
        }
        __syncthreads();   // phase A's carry reads before phase B's carry writes
        const bool last = g + 8 >= fb;
        const long long gh8 = gh + 8LL * hop;
        for (int base = 0; base < (K - 1) * hop; base += 256 * CH) {   // phase B: blocks [g+8, g+8+K-1), fresh
            float a0[CH], n0[CH];
#pragma unroll
            for (int s = 0; s < CH; ++s) {
                const int idx = base + tid + 256 * s, bb = 8 + (idx >> lh);
                const bool ok = idx < (K - 1) * hop && bb < bb_tot;
                a0[s] = ok ? out_add[gh8 + idx] : 0.0f;
                n0[s] = ok && norm_add ? norm_add[gh8 + idx] : 0.0f;
            }
#pragma unroll
            for (int s = 0; s < CH; ++s) {
                const int idx = base + tid + 256 * s, bb = 8 + (idx >> lh), j = idx & (hop - 1);
                if (idx >= (K - 1) * hop || bb >= bb_tot) continue;
                float acc, nacc;
                combine(bb, j, a0[s], n0[s], &acc, &nacc);
                if (last) {
                    if (bb >= bb_fa && bb < bb_bend) {
                        out_add[gh8 + idx] = acc;
                        if (norm_add) norm_add[gh8 + idx] = nacc;
                    }
                } else {
                    carry[idx] = acc;   // = (b - (g+8)) * hop + j: next step's base
                    ncarry[idx] = nacc;
                }
            }
        }
        __syncthreads();   // stage and carry are reused by the next step
    }
}

bool istft_fused_supported(long long nfft, long long hop) {
    return nfft == 1024 && hop >= 256 && nfft % hop == 0 && (hop & (hop - 1)) == 0;   // K = nfft/hop <= 4
}

hipError_t launch_istft_fused(long long nfft, long long hop, const float2* spec, long long count,
                              const float* win, float* out_add, float* norm_add, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (!istft_fused_supported(nfft, hop)) return hipErrorInvalidValue;
    constexpr int N = 1024;
    const float2* pN = pass_twiddles(N);
    if (!pN) return hipErrorOutOfMemory;
    const int K = (int)(N / hop);
    // owned frames per workgroup: run + K - 1 computed frames = whole steps of 8
    long long run = 64 - (K - 1);
    if (count < 8 * run) run = 8 - (K - 1);   // small jobs: more workgroups
    const long long grid = (count + run - 1) / run;
hipLaunchKernelGGL((k_istft<N>), dim3((unsigned)grid), dim3(256), 0, s, spec, count, (int)hop, K, win, out_add,
                       norm_add, run, pN);
    return hipGetLastError();
}

hipError_t launch_ola(long long nfft, long long hop, const float2* time_frames, long long count,
                      const float* win, float* out_add, float* norm_add, hipStream_t s) {
    const long long len = (count - 1) * hop + nfft;
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ola, dim3(stride_blocks(len)), dim3(256), 0, s, nfft, hop, time_frames, count, win,
                       out_add, norm_add, len);
    return hipGetLastError();
}

}  // namespace vvh
