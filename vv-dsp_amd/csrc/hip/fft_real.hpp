// fft_real.hpp -- the fused power-of-two R2C / C2R kernels for gfx950 (real
// length 2M <= 16384; launched from fft_real.hip).
//
// R2C of real length 2M runs an M-point complex FFT on z[m] = x[2m] + i x[2m+1]
// and the split step X[k] = Fe + W_{2M}^k (-i Fo) with Z[k] and Z[M-k] held in
// the same thread (mirror-paired last pass); C2R runs the inverse split step
// and an M-point inverse FFT.  Real transforms move 4 B/point.
#pragma once
#include "fft_rules.hpp"

namespace vvh {

template <int M>
__global__ void __launch_bounds__(Wg<M>::value)
k_r2c(const float* in, float2* out, long long batch, long long in_dist, long long out_dist,
      const float2* gpass, const float2* gtabM, const float2* gtab2M) {
    using G = Geo<M>;
    constexpr bool PAIR = G::CAN_PAIR;
    constexpr int WG = Wg<M>::value, F = Wg<M>::F;
    __shared__ float2 lds[F * G::LDS];
    __shared__ float2 ltab[TwLayout<M>::ENTRIES];
    __shared__ float2 lpost[PostLayout<M>::ENTRIES];
    stage_twiddles<M, WG>(ltab, gpass, gtabM);
    stage_post<M, WG>(lpost, gtab2M);
    __syncthreads();
    const TwTab<M> tw{ltab};
    const PostTab<M> pw{lpost};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + slot * G::LDS;
    long long stride = (long long)gridDim.x * F;
    long long f = uni<G::T>((long long)blockIdx.x * F + slot);
    long long fend = batch;
    float2 nx[G::P];
    if (f < fend) {
        const float2* src = reinterpret_cast<const float2*>(in + f * in_dist);
        rows_load<M>(nx, src, t);
    }
    for (; f < fend; f += stride) {
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = nx[r];
        const long long fn = f + stride;
        if (fn < fend) {
            const float2* src = reinterpret_cast<const float2*>(in + fn * in_dist);
            rows_load<M>(nx, src, t);
        }
        fft_regs<M, true, PAIR>(v, t, my, tw);
        float2* dst = out + f * out_dist;
        if constexpr (PAIR) {
#pragma unroll
            for (int q = 0; q < G::P; ++q) {
                const int k = out_pos<M, true>(t, q);
                const float2 A = v[q];
                if (k == 0) {
                    *(dst) = split_fwd_dc(A.x, A.y);
                    *(dst + M) = split_fwd_nyq(A.x, A.y);
                } else {
                    *(dst + k) = split_fwd(A, cconj(mirror_of<M, true>(v, t, q)), pw(k));
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < G::P; ++q) my[G::pad(out_pos<M>(t, q))] = v[q];
            xsync<G::T>();
#pragma unroll
            for (int q = 0; q < G::P; ++q) {
                const int k = t + G::T * q;
                const float2 A = my[G::pad(k)];
                if (k == 0) {
                    *(dst) = split_fwd_dc(A.x, A.y);
                    *(dst + M) = split_fwd_nyq(A.x, A.y);
                } else {
                    *(dst + k) = split_fwd(A, cconj(my[G::pad(M - k)]), pw(k));
                }
            }
            xsync<G::T>();
        }
    }
}

template <int M>
__global__ void __launch_bounds__(Wg<M>::value)
k_c2r(const float2* in, float* out, long long batch, long long in_dist, long long out_dist,
      const float2* gpass, const float2* gtabM, const float2* gtab2M, float scale) {
    using G = Geo<M>;
    constexpr int WG = Wg<M>::value, F = Wg<M>::F;
    __shared__ float2 lds[F * G::LDS];
    __shared__ float2 ltab[TwLayout<M>::ENTRIES];
    __shared__ float2 lpost[PostLayout<M>::ENTRIES];
    stage_twiddles<M, WG>(ltab, gpass, gtabM);
    stage_post<M, WG>(lpost, gtab2M);
    __syncthreads();
    const TwTab<M> tw{ltab};
    const PostTab<M> pw{lpost};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T;
    float2* my = lds + slot * G::LDS;
    const long long stride = (long long)gridDim.x * F;
    long long f = uni<G::T>((long long)blockIdx.x * F + slot);
    float2 nx[G::P];
    float2 nxm = make_float2(0.0f, 0.0f);
    if (f < batch) {
        const float2* src = in + f * in_dist;
#pragma unroll
        for (int r = 0; r < G::P; ++r) nx[r] = ld_nt(src + t + r * G::T);   // (rows_load: other code at M = 4, 8, 16)
        nxm = src[M];
    }
    for (; f < batch; f += stride) {
        float2 xm = nxm;
#pragma unroll
        for (int r = 0; r < G::P; ++r) my[G::pad(t + r * G::T)] = nx[r];
        const long long fn = f + stride;
        if (fn < batch) {
            const float2* src = in + fn * in_dist;
#pragma unroll
            for (int r = 0; r < G::P; ++r) nx[r] = ld_nt(src + t + r * G::T);
            nxm = src[M];
        }
        xsync<G::T>();
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            const int k = t + r * G::T;
            float2 A = my[G::pad(k)];
            float2 B;
            if (k == 0) {   // imag of DC and Nyquist ignored (the fft_kiss.c:158-171 result)
                A = split_inv_edge(A);
                B = split_inv_edge(xm);
            } else {
                B = my[G::pad(M - k)];
            }
            v[r] = split_inv(A, B, pw(k));
        }
        xsync<G::T>();
        fft_regs<M, false>(v, t, my, tw);
        float2* dst = reinterpret_cast<float2*>(out + f * out_dist);
#pragma unroll
        for (int q = 0; q < G::P; ++q) st_nt(cscale(v[q], scale), dst + out_pos<M>(t, q));
    }
}

// R2C of 32..128 real points (M = 16..64) with dense rows: the mirror of
// k_c2r_small -- each wave's 64 / T rows (1024 float2) loaded as 16 B per lane
// through its LDS area (padded 1 per 16), the FFT's bins back through the area
// for the split step's mirror, and the M + 1 bins per row staged and stored as
// 8 B per lane, coalesced.  A wave-uniform loop.
template <int M>
__global__ void __launch_bounds__(256, 4)
k_r2c_small(const float* __restrict__ in, float2* __restrict__ out, long long batch, const float2* gpass,
            const float2* gtabM, const float2* gtab2M) {
    using G = Geo<M>;
    static_assert(G::P == 16 && G::T <= 4, "M = 16..64");
    constexpr int F = 256 / G::T, WS = 64 / G::T, WA = WS * G::LDS;   // float2 per wave area
    static_assert(WS * (M + 1) <= WA && WB_CPX + WB_CPX / 16 <= WA, "the wave area holds the rows and the bins");
    __shared__ __attribute__((aligned(16))) float2 lds[F * G::LDS];
    __shared__ float2 ltab[TwLayout<M>::ENTRIES];
    __shared__ float2 lpost[PostLayout<M>::ENTRIES];
    stage_twiddles<M, 256>(ltab, gpass, gtabM);
    stage_post<M, 256>(lpost, gtab2M);
    __syncthreads();
    const TwTab<M> tw{ltab};
    const PostTab<M> pw{lpost};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T, wv = lt >> 6, lane = lt & 63, sl = slot - wv * WS;
    float2* my = lds + slot * G::LDS;
    float2* wa = lds + wv * WA;
    for (long long fw = (long long)blockIdx.x * F + (long long)wv * WS; fw < batch; fw += (long long)gridDim.x * F) {
        const long long nr = batch - fw < WS ? batch - fw : WS;
        const int nin = (int)nr * M, nout = (int)nr * (M + 1);   // valid input / output float2
#pragma unroll
        for (int i = 0; i < WB_STEPS; ++i) {   // (wb_ec, wb_ld, wb_put_c written out: through them, other code)
            const int e = i * WB_STEP_C + WB_LANE_C * lane;
            const vf4_t q = e < nin ? __builtin_nontemporal_load(reinterpret_cast<const vf4_t*>(in + 2 * (fw * M + e)))
                                    : vf4_t{0.0f, 0.0f, 0.0f, 0.0f};
            wa[G::pad(e)] = make_float2(q[0], q[1]);
            wa[G::pad(e + 1)] = make_float2(q[2], q[3]);
        }
        xsync<64>();
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) v[r] = wa[G::pad(sl * M + t + r * G::T)];
        xsync<64>();   // the FFT's exchanges reuse the area
        fft_regs<M, true>(v, t, my, tw);
        xsync<64>();
#pragma unroll
        for (int q = 0; q < G::P; ++q) wa[G::pad(sl * M + out_pos<M>(t, q))] = v[q];
        xsync<64>();
        float2 o[G::P];
        float2 onyq = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            const int k = t + r * G::T;
            const float2 A = wa[G::pad(sl * M + k)];
            if (k == 0) {
                o[r] = split_fwd_dc(A.x, A.y);
                onyq = split_fwd_nyq(A.x, A.y);
            } else {
                o[r] = split_fwd(A, cconj(wa[G::pad(sl * M + M - k)]), pw(k));
            }
        }
        xsync<64>();
#pragma unroll
        for (int r = 0; r < G::P; ++r) wa[sl * (M + 1) + t + r * G::T] = o[r];
        if (t == 0) wa[sl * (M + 1) + M] = onyq;
        xsync<64>();
#pragma unroll
        for (int i = 0; i * 64 < WS * (M + 1); ++i) {
            const int e = i * 64 + lane;
            if (e < nout) st_nt(wa[e], out + fw * (M + 1) + e);
        }
        xsync<64>();
    }
}

// C2R of 32..128 real points (M = 16..64) with dense rows: k_c2r's arithmetic,
// each wave's 64 / T rows of M + 1 complex values loaded as 8 B per lane
// (coalesced) into its LDS area and read from there by the split step, and its
// real outputs (64 / T rows x 2M floats = 1024 float2) staged back (padded 1 per
// 16) and stored as 16 B per lane.  A wave-uniform loop.
template <int M>
__global__ void __launch_bounds__(256, 4)
k_c2r_small(const float2* __restrict__ in, float* __restrict__ out, long long batch, const float2* gpass,
            const float2* gtabM, const float2* gtab2M, float scale) {
    using G = Geo<M>;
    static_assert(G::P == 16 && G::T <= 4, "M = 16..64");
    constexpr int F = 256 / G::T, WS = 64 / G::T, WA = WS * G::LDS;   // float2 per wave area
    static_assert(WS * (M + 1) <= WA && WB_CPX + WB_CPX / 16 <= WA, "the wave area holds the rows and the outputs");
    __shared__ __attribute__((aligned(16))) float2 lds[F * G::LDS];
    __shared__ float2 ltab[TwLayout<M>::ENTRIES];
    __shared__ float2 lpost[PostLayout<M>::ENTRIES];
    stage_twiddles<M, 256>(ltab, gpass, gtabM);
    stage_post<M, 256>(lpost, gtab2M);
    __syncthreads();
    const TwTab<M> tw{ltab};
    const PostTab<M> pw{lpost};
    const int lt = threadIdx.x, slot = lt / G::T, t = lt % G::T, wv = lt >> 6, lane = lt & 63, sl = slot - wv * WS;
    float2* my = lds + slot * G::LDS;
    float2* wa = lds + wv * WA;
    for (long long fw = (long long)blockIdx.x * F + (long long)wv * WS; fw < batch; fw += (long long)gridDim.x * F) {
        const long long nr = batch - fw < WS ? batch - fw : WS;
        const int nin = (int)nr * (M + 1), nout = (int)nr * M;   // valid input / output float2
#pragma unroll
        for (int i = 0; i * 64 < WS * (M + 1); ++i) {
            const int e = i * 64 + lane;
            if (e < WS * (M + 1)) wa[e] = e < nin ? in[fw * (M + 1) + e] : make_float2(0.0f, 0.0f);
        }
        xsync<64>();
        const float2* row = wa + sl * (M + 1);
        float2 v[G::P];
#pragma unroll
        for (int r = 0; r < G::P; ++r) {
            const int k = t + r * G::T;
            float2 A = row[k], B;
            if (k == 0) {   // imag of DC and Nyquist ignored (the fft_kiss.c:158-171 result)
                A = split_inv_edge(A);
                B = split_inv_edge(row[M]);
            } else {
                B = row[M - k];
            }
            v[r] = split_inv(A, B, pw(k));
        }
        xsync<64>();   // the FFT's exchanges reuse the area
        fft_regs<M, false>(v, t, my, tw);
        xsync<64>();
#pragma unroll
        for (int q = 0; q < G::P; ++q) wa[G::pad(sl * M + out_pos<M>(t, q))] = cscale(v[q], scale);
        xsync<64>();
#pragma unroll
        for (int i = 0; i < WB_STEPS; ++i) {   // (wb_ec, wb_get_c, wb_st written out: through them, other code)
            const int e = i * WB_STEP_C + WB_LANE_C * lane;   // float2 index among the wave's outputs
            if (e < nout) {
                const float2 c0 = wa[G::pad(e)], c1 = wa[G::pad(e + 1)];
                __builtin_nontemporal_store(vf4_t{c0.x, c0.y, c1.x, c1.y},
                                            reinterpret_cast<vf4_t*>(out + 2 * (fw * M + e)));
            }
        }
        xsync<64>();
    }
}

}  // namespace vvh
