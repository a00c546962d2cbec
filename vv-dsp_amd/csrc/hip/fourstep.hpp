// fourstep.hpp -- the two kernels of the two-pass four-step FFT (launchers:
// fourstep_fft.hip).  n = N1*N2, 64 <= N1 <= N2 <= 1024, and
//   X[k1 + N1*k2] = sum_n2 W_N2^(n2 k2) * W_n^(n2 k1) * sum_n1 x[n1 N2 + n2] W_N1^(n1 k1)
// in TWO HBM passes, no transposes:
//   columns: a workgroup owns G = 16 adjacent columns n2 of [N1][N2]; lane l
//            works on column l % G, so every load x[n1][n2..n2+15] and every
//            store Y[k1][n2..n2+15] is a 128-B line.  N1-pt FFT down each
//            column, times W_n^(n2 k1), stored in place of the column.
//   rows:    a workgroup owns G = 16 adjacent rows k1; loads are row-contiguous
//            (lanes along the row); the last Stockham exchange re-maps the
//            threads so lanes run across the G rows, and the stores
//            X[k1..k1+15 + N1*k2] are 128-B lines again.
#pragma once
#include "fft_core.hpp"
#include "fourstep_chain.hpp"

namespace vvh {

// One asm statement, not fft_core.hpp's lgkm_wait0() and lds_barrier(): the compiler
// schedules address arithmetic between those two, which changes every kernel here.
__device__ __forceinline__ void wg_bar() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// G transforms of length N per workgroup; LDS region per transform of S
// elements (floats when RI, float2 otherwise).  S is odd, so the same offset in
// the G regions falls in G different banks (lanes of one instruction work on
// different transforms in the interleaved mapping).
template <int N, int G, bool RI>
struct FsGeo {
    using Ge = Geo<N>;
    static constexpr int T = Ge::T;
    static constexpr int THREADS = G * T;
    static constexpr int S = Ge::LDS | 1;
    static constexpr int LDS_BYTES = G * S * (RI ? 4 : 8);
    static_assert(THREADS <= 1024 && Ge::NPASS >= 2, "two-pass four-step geometry");
};

// Stockham exchange after pass p; the writer is thread wt of transform wj, the
// reader thread rt of transform rj (a re-map of the workgroup when they differ).
template <int N, int p, int S, bool RI>
__device__ __forceinline__ void fs_exchange(float2* v, void* lds, int wj, int wt, int rj, int rt) {
    using Ge = Geo<N>;
    constexpr int R = Ge::radix(p), Ns = Ge::ns(p), R2 = Ge::radix(p + 1), T = Ge::T;
    if constexpr (RI) {
        float* W = reinterpret_cast<float*>(lds) + wj * S;
        const float* Rd = reinterpret_cast<const float*>(lds) + rj * S;
        float nx[Ge::P];
#pragma unroll
        for (int i = 0; i < Ge::P / R; ++i) {
            const int b = wt + T * i, base = (b / Ns) * Ns * R + (b % Ns);
#pragma unroll
            for (int r = 0; r < R; ++r) W[Ge::pad(base + r * Ns)] = v[i * R + r].x;
        }
        wg_bar();
#pragma unroll
        for (int i = 0; i < Ge::P / R2; ++i) {
            const int b = rt + T * i;
#pragma unroll
            for (int r = 0; r < R2; ++r) nx[i * R2 + r] = Rd[Ge::pad(b + r * (N / R2))];
        }
        wg_bar();
#pragma unroll
        for (int i = 0; i < Ge::P / R; ++i) {
            const int b = wt + T * i, base = (b / Ns) * Ns * R + (b % Ns);
#pragma unroll
            for (int r = 0; r < R; ++r) W[Ge::pad(base + r * Ns)] = v[i * R + r].y;
        }
        wg_bar();
#pragma unroll
        for (int i = 0; i < Ge::P / R2; ++i) {
            const int b = rt + T * i;
#pragma unroll
            for (int r = 0; r < R2; ++r) v[i * R2 + r] = make_float2(nx[i * R2 + r], Rd[Ge::pad(b + r * (N / R2))]);
        }
        wg_bar();
    } else {
        float2* W = reinterpret_cast<float2*>(lds) + wj * S;
        const float2* Rd = reinterpret_cast<const float2*>(lds) + rj * S;
#pragma unroll
        for (int i = 0; i < Ge::P / R; ++i) {
            const int b = wt + T * i, base = (b / Ns) * Ns * R + (b % Ns);
#pragma unroll
            for (int r = 0; r < R; ++r) W[Ge::pad(base + r * Ns)] = v[i * R + r];
        }
        wg_bar();
#pragma unroll
        for (int i = 0; i < Ge::P / R2; ++i) {
            const int b = rt + T * i;
#pragma unroll
            for (int r = 0; r < R2; ++r) v[i * R2 + r] = Rd[Ge::pad(b + r * (N / R2))];
        }
        wg_bar();
    }
}

// Pass chain; with REMAP the last pass runs in mapping (j2, t2), all others in (j1, t1).
template <int N, bool FWD, int p, int S, bool RI, bool REMAP>
struct FsChain {
    __device__ __forceinline__ static void run(float2* v, void* lds, const TwTab<N>& tw, int j1, int t1, int j2,
                                               int t2) {
        constexpr int NP = Geo<N>::NPASS;
        constexpr bool last = p == NP - 1;
        pass_compute<N, FWD, p, false>(v, (REMAP && last) ? t2 : t1, tw);
        if constexpr (!last) {
            if constexpr (REMAP && p + 1 == NP - 1) fs_exchange<N, p, S, RI>(v, lds, j1, t1, j2, t2);
            else fs_exchange<N, p, S, RI>(v, lds, j1, t1, j1, t1);
            FsChain<N, FWD, p + 1, S, RI, REMAP>::run(v, lds, tw, j1, t1, j2, t2);
        }
    }
};

// Columns pass: Y[b][k1][n2] = W_n^(+-n2 k1) * FFT_N1(x[b][.][n2])[k1]
template <int N1, int G, bool RI, bool FWD>
__global__ void __launch_bounds__(G * Geo<N1>::T)
k_fs_cols(const float2* __restrict__ in, float2* __restrict__ out, int N2, int cpb, const float2* gpass,
          const float2* gtab, const float2* __restrict__ split, int lo_bits, FsHooks hk) {
    using Ge = Geo<N1>;
    using F = FsGeo<N1, G, RI>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[F::LDS_BYTES];
    __shared__ float2 ltab[TwLayout<N1>::ENTRIES];
    // two-level W_n table (lo[2^lo_bits] ++ hi[n >> lo_bits], n <= 2^20) in LDS
    __shared__ float2 lsplit[2048];
    stage_twiddles<N1, F::THREADS>(ltab, gpass, gtab);
    const long long n = (long long)N1 * N2;
    {
        const int nsplit = (1 << lo_bits) + (int)(n >> lo_bits);
        for (int i = threadIdx.x; i < nsplit; i += F::THREADS) lsplit[i] = split[i];
    }
    const long long b = blockIdx.x / cpb;
    const int col = (blockIdx.x % cpb) * G + (int)(threadIdx.x % G), t = threadIdx.x / G;
    float2 v[Ge::P];
    if (hk.pre_chirp) {
        const long long base = (hk.b0 + b) * hk.in_dist;
#pragma unroll
        for (int r = 0; r < Ge::P; ++r) {
            const long long m = (long long)(t + r * Ge::T) * N2 + col;
            float2 x = make_float2(0.0f, 0.0f);
            if (m < hk.nsig) {
                x = hk.real_in ? make_float2(reinterpret_cast<const float*>(hk.raw)[base + m], 0.0f)
                               : reinterpret_cast<const float2*>(hk.raw)[base + m];
                x = cmul(x, hk.pre_chirp[m]);
            }
            v[r] = x;
        }
    } else {
        const float2* src = in + b * n + col;
#pragma unroll
        for (int r = 0; r < Ge::P; ++r) v[r] = ld_nt(src + (long long)(t + r * Ge::T) * N2);
    }
    __syncthreads();
    const int j = threadIdx.x % G;
    FsChain<N1, FWD, 0, F::S, RI, false>::run(v, lds, TwTab<N1>{ltab}, j, t, j, t);
    const unsigned mask = (1u << lo_bits) - 1u;
    const float2* hi = lsplit + (1u << lo_bits);
    float2* dst = out + b * n + col;
#pragma unroll
    for (int q = 0; q < Ge::P; ++q) {
        const int k1 = out_pos<N1>(t, q);
        const unsigned k = (unsigned)col * (unsigned)k1;   // < n <= 2^20
        float2 w = cmul(lsplit[k & mask], hi[k >> lo_bits]);
        if (!FWD) w = cconj(w);
        st_nt(cmul(v[q], w), dst + (long long)k1 * N2);
    }
}

// Rows pass: X[b][k1 + N1 k2] = scale * FFT_N2(Y[b][k1][.])[k2], times mulv[k1 + N1 k2]
// when mulv is given (Bluestein's pointwise product with the chirp spectrum,
// the same n-vector for every transform of the batch)
template <int N2, int G, bool RI, bool FWD>
__global__ void __launch_bounds__(G * Geo<N2>::T)
k_fs_rows(const float2* __restrict__ in, float2* __restrict__ out, int N1, int rpb, const float2* gpass,
          const float2* gtab, float scale, FsHooks hk) {
    using Ge = Geo<N2>;
    using F = FsGeo<N2, G, RI>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[F::LDS_BYTES];
    __shared__ float2 ltab[TwLayout<N2>::ENTRIES];
    stage_twiddles<N2, F::THREADS>(ltab, gpass, gtab);
    const long long n = (long long)N1 * N2;
    const long long b = blockIdx.x / rpb;
    const int r0 = (blockIdx.x % rpb) * G;
    const int j1 = threadIdx.x / Ge::T, t1 = threadIdx.x % Ge::T;   // lanes along a row
    const int j2 = threadIdx.x % G, t2 = threadIdx.x / G;           // lanes across rows
    const float2* src = in + b * n + (long long)(r0 + j1) * N2 + t1;
    float2 v[Ge::P];
#pragma unroll
    for (int r = 0; r < Ge::P; ++r) v[r] = ld_nt(src + r * Ge::T);
    __syncthreads();
    FsChain<N2, FWD, 0, F::S, RI, true>::run(v, lds, TwTab<N2>{ltab}, j1, t1, j2, t2);
    float2* dst = out + b * n + r0 + j2;
#pragma unroll
    for (int q = 0; q < Ge::P; ++q) {
        const int k2 = out_pos<N2>(t2, q);
        float2 x = FWD ? v[q] : cscale(v[q], scale);
        const long long k = r0 + j2 + (long long)k2 * N1;
        if (hk.mulv) x = cmul(x, hk.mulv[k]);
        if (hk.post_chirp) {
            if (k < hk.nout) hk.post_out[(hk.b0 + b) * hk.out_dist + k] = cscale(cmul(x, hk.post_chirp[k]), hk.post_scale);
        } else {
            st_nt(x, dst + (long long)k2 * N1);
        }
    }
}

}  // namespace vvh
