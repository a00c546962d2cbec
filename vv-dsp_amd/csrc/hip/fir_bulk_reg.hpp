// fir_bulk_reg.hpp -- k_fir_bulk_reg: overlap-save at N = 1024 with 16 x 16 x 4
// transforms and register loads (instantiated by fir_1024.hip; knob FIR_R32 = 0).
#pragma once
#include "fir_common.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

// ------------------------------------------------------------------------
// k_fir_bulk_reg<N>: the bulk pairs (le == N/4) with the pair's two blocks
// loaded straight into registers (coalesced dword loads, the LE overlap re-read
// from L1/L2) instead of round 2's LDS span (k_fir_bulk, now in
// scripts/stftlab.hip only).  Without the 28 KB of spans a workgroup needs
// 24 KB of LDS, so four workgroups fit per CU (16 waves instead of 12): the
// kernel is latency-bound on its LDS exchanges (scripts/kbench.py firlab*).
// The next pair's loads are issued after the inverse FFT, ahead of this
// pair's stores (issued during the FFT they would need 32 more VGPRs than the
// four waves per SIMD allow).  All global accesses are compiler-visible.
// ------------------------------------------------------------------------
// DYN: the dynamic band walk of k_stft_pair VAR 4 (persistent grid, each
// wave's next pair from a per-(XCD group, slot) counter in `ctrs`, the last wave
// of each counter stream resets it); otherwise the static XCD walk.
template <int N, bool DYN = false>
__global__ void __launch_bounds__(256, 4)
k_fir_bulk_reg(const float2* Hg, const float* x, float* y, long long nch, long long x_stride, long long y_stride,
               long long cnt, long long q0, const float2* gpass, long long n, const float* prefix, long long lm1,
               long long qf, long long ql, unsigned* ctrs) {
    using G = Geo<N>;
    static_assert(G::T == 64 && N == 1024 && !TwLayout<N>::SPLIT, "one wave per transform (T = N/16), pass-major twiddles");
    constexpr int F = 4, RL = G::RL;
    constexpr int LE = N / 4, LOUT = N - LE;   // taps <= N/4 + 1
    constexpr int TWL = G::tw_off(G::NPASS - 1) > 0 ? G::tw_off(G::NPASS - 1) : 1;
    constexpr int XW = ri_floats<N>();   // the FFT exchanges as real / imaginary halves (b32)
    __shared__ __attribute__((aligned(16))) float xch[F * XW];
    __shared__ float2 ltab[TWL];
    __shared__ float2 lH[N / 2 + 1];
    for (int i = threadIdx.x; i < G::tw_off(G::NPASS - 1); i += 256) ltab[i] = gpass[i];
    for (int i = threadIdx.x; i <= N / 2; i += 256) lH[i] = Hg[i];
    const int lt = threadIdx.x, slot = lt >> 6, t = lt & 63;
    TwLastReg<N> tw;
    tw.tab = ltab;
    tw.load(gpass, t);
    __syncthreads();
    float2* my = reinterpret_cast<float2*>(xch + slot * XW);
    long long p, p_end, p_step;
    // DYN: counter value k of stream s (= XCD group, slot) is pair
    // (k / 64) * 8 F 64 + s * 64 + k % 64: the chip sweeps one moving band
    const int stream = __builtin_amdgcn_readfirstlane((int)(blockIdx.x & 7) * F + slot);
    unsigned* const ctr = DYN ? ctrs + 32 * stream : nullptr;
    auto band_pair = [&](unsigned k) -> long long {
        return (long long)(k >> 6) * (8 * F * 64) + (long long)stream * 64 + (long long)(k & 63);
    };
    unsigned rk = 0;   // lane 0: the counter value of the pair after p
    if constexpr (DYN) {
        unsigned r0 = 0;
        if (t == 0) r0 = atomicAdd(ctr, 1u);
        p = band_pair(__builtin_amdgcn_readfirstlane(r0));
        p_end = nch * cnt;
        p_step = 0;
        if (p < p_end && t == 0) rk = atomicAdd(ctr, 1u);
    } else {
        xcd_walk(nch * cnt, F, slot, &p, &p_end, &p_step);
        p = uni<64>(p);
        p_end = uni<64>(p_end);
        p_step = uni<64>(p_step);
        if (p >= p_end) return;
    }
    auto locate = [&](long long it, long long* cc, long long* jj) {
        *cc = it / cnt;
        *jj = 2 * (q0 + (it - *cc * cnt));
    };
    long long c = 0, j = 0;
    if (p < p_end) locate(p, &c, &j);
    float xa[G::P], xb[G::P];
    auto load_a = [&](long long cc, long long jj) {
        const float* a = x + cc * x_stride + jj * LOUT - LE;   // wave-uniform block base
#pragma unroll
        for (int r = 0; r < G::P; ++r) xa[r] = __builtin_nontemporal_load(a + t + 64 * r);
    };
    auto load_b = [&](long long cc, long long jj) {
        const float* b = x + cc * x_stride + jj * LOUT - LE + LOUT;
#pragma unroll
        for (int r = 0; r < G::P; ++r) xb[r] = b[t + 64 * r];   // overlaps the next pair's block a: cached
    };
    // Edge pairs (pair index < qf: the span starts before sample 0; >= ql: it
    // reaches past n) take bounds-checked loads (history prefix or zeros before
    // 0, zeros past n) and predicated stores in the same launch -- a wave-
    // uniform branch, so the bulk pairs pay two scalar compares.
    // An edge pair is loaded at the top of its own iteration (nothing else live
    // then); a bulk pair is prefetched during the previous pair's stores.
    auto is_edge = [&](long long jj) { return (jj >> 1) < qf || (jj >> 1) >= ql; };
    if (p < p_end && !is_edge(j)) {
        load_a(c, j);
        load_b(c, j);
    }
    for (; p < p_end; p += p_step) {
        if constexpr (DYN) p_step = band_pair(__builtin_amdgcn_readfirstlane(rk)) - p;
        const bool more = p + p_step < p_end;
        long long cn = c, jn = j;
        if (more) locate(p + p_step, &cn, &jn);
        if (is_edge(j)) {
            // staged through the (idle) exchange buffer with a rolled loop, so the
            // bounds checks need no per-register address state
            const float* xs = x + c * x_stride;
            const float* pre = prefix ? prefix + c * lm1 : nullptr;
            float* sf = reinterpret_cast<float*>(my);
            auto stage = [&](long long s0, float* dst) {
#pragma unroll 1
                for (int k = t; k < N; k += 64) sf[k] = fir_fetch<0>(xs, pre, s0 + k, n, lm1, n);
                xsync<64>();
#pragma unroll
                for (int r = 0; r < G::P; ++r) dst[r] = sf[t + 64 * r];
                xsync<64>();
            };
            stage(j * LOUT - LE, xa);
            stage((j + 1) * LOUT - LE, xb);
        }
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = make_float2(xa[r], xb[r]);
        tw.opaque();
        fft_regs<N, true, false, true, TwLastReg<N>, false, false>(v, t, my, tw);
        float2 u[G::P];
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            const int m = q / RL + G::NPT * (q % RL);   // out_pos<N>(t, q) = t + 64*m
            if (m < G::P / 2) u[m] = cmul(v[q], lH[t + 64 * m]);
            else u[m] = cmul(v[q], cconj(lH[N - t - 64 * m]));
        }
        tw.opaque();
        fft_regs<N, false, false, true, TwLastReg<N>, false, false>(u, t, my, tw);
        if (more && !is_edge(jn)) {   // ahead of this pair's stores: in flight across them
            load_a(cn, jn);
            load_b(cn, jn);
        }
        if constexpr (DYN) {
            if (more && t == 0) rk = atomicAdd(ctr, 1u);   // -> the pair after cn/jn
        }
        float* ya = y + c * y_stride + j * LOUT - LE;   // + e: block j output (e >= LE)
        if (is_edge(j)) {   // outputs past n are not stored
            long long rem = n - (j * LOUT - LE + t);   // this lane's outputs below n: e < rem
            const int rm = (int)(rem < (1 << 30) ? rem : (1 << 30));
#pragma unroll
            for (int q = 0; q < G::P; ++q) {
                const int m = q / RL + G::NPT * (q % RL);
                if (q % RL != 0) {
                    if (64 * m < rm) ya[t + 64 * m] = u[q].x;
                    if (64 * m + LOUT < rm) ya[LOUT + t + 64 * m] = u[q].y;
                }
            }
            c = cn;
            j = jn;
            continue;
        }
#pragma unroll
        for (int q = 0; q < G::P; ++q) {
            if (q % RL != 0) {   // e = t + 64 m >= LE exactly for these registers
                const int m = q / RL + G::NPT * (q % RL);
                __builtin_nontemporal_store(u[q].x, ya + t + 64 * m);
                __builtin_nontemporal_store(u[q].y, ya + LOUT + t + 64 * m);
            }
        }
        c = cn;
        j = jn;
    }
    if constexpr (DYN) {   // the XCD group's last wave out resets its counters for the next launch
        if (t == 0) {
            const unsigned nw = (unsigned)((gridDim.x - (blockIdx.x & 7) + 7) / 8);
            if (atomicAdd(ctr + 16, 1u) == nw - 1) {
                atomicExch(ctr, 0u);
                atomicExch(ctr + 16, 0u);
            }
        }
    }
}

}  // namespace vvh
