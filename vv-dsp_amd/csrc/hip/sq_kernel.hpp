// sq_kernel.hpp -- transforms of n = N1 * N2 (both <= 32) in registers: the
// speech lengths 400 = 20 x 20, 480 = 20 x 24, 960 = 30 x 32.  The plan kernel
// (mixed_plan.hip) runs a runtime radix plan through LDS with a barrier per pass
// and is bound by that (400-point STFT: 0.31 of the HBM roofline); here a
// transform (a row, or a frame pair as MixIO's MODE 1-3) is owned by
// max(N1, N2) lanes of one wave and takes two register passes with one LDS
// exchange:
//   pass 1, lane m2 < N2:  N1-point DFT of x[m1 N2 + m2] over m1, times W_n^(m2 k1)
//   pass 2, lane k1 < N1:  N2-point DFT over m2 -> X[k1 + N1 k2]
// The N-point DFTs are composed at compile time (R = A x B, constant
// twiddles), the W_n factors come from the n-entry table in LDS.  Results go
// back to LDS in natural order and the wave writes its pairs' rows as one
// contiguous run (rows a and b of consecutive pairs are adjacent).
//
// Included by the units that instantiate the kernel: sq_stft.hip (MODE 1, 2, 3)
// and sq_rows.hip (MODE 0, 5).
#pragma once
#include "mixed_common.hpp"

namespace vvh {

constexpr double cx_pi = 3.14159265358979323846264338327950288;
// cos / sin(2 pi j / R) in double at compile time (Taylor series on [-pi, pi])
constexpr double cx_cos2pi(int j, int R) {
    j %= R;
    double x = 2.0 * cx_pi * (double)j / (double)R;
    if (2 * j > R) x -= 2.0 * cx_pi;
    double term = 1.0, sum = 1.0;
    for (int i = 1; i < 24; ++i) {
        term *= -x * x / ((2.0 * i - 1.0) * (2.0 * i));
        sum += term;
    }
    return sum;
}
constexpr double cx_sin2pi(int j, int R) {
    j %= R;
    double x = 2.0 * cx_pi * (double)j / (double)R;
    if (2 * j > R) x -= 2.0 * cx_pi;
    double term = x, sum = x;
    for (int i = 1; i < 24; ++i) {
        term *= -x * x / ((2.0 * i) * (2.0 * i + 1.0));
        sum += term;
    }
    return sum;
}

// v * W_R^J (forward, W_R = exp(-2 pi i / R)); quarter and half turns exact
template <int J, int R>
__device__ __forceinline__ float2 twk(float2 v) {
    constexpr int m = J % R;
    if constexpr (m == 0) {
        return v;
    } else if constexpr (2 * m == R) {
        return upk(-pk(v));
    } else if constexpr (4 * m == R) {
        return cmul_mi(v);
    } else if constexpr (4 * m == 3 * R) {
        return cmul_pi(v);
    } else {
        constexpr float c = (float)cx_cos2pi(m, R), s = (float)-cx_sin2pi(m, R);
        return cmul(v, make_float2(c, s));
    }
}

template <int R>
struct RegFac {   // R = A * B for the composite DFT (A = 1: a base case)
    static constexpr bool BASE = R == 1 || R == 2 || R == 3 || R == 4 || R == 5 || R == 7 || R == 8 || R == 16;
    static constexpr int A = BASE ? 1 : R % 8 == 0 ? 8 : R % 4 == 0 ? 4 : R % 2 == 0 ? 2 : R % 3 == 0 ? 3 : R % 5 == 0 ? 5 : 7;
    static constexpr int B = BASE ? R : R / A;
};

// forward DFT of length R on registers, natural order in and out
template <int R>
__device__ __forceinline__ void reg_dft(float2* v) {
    if constexpr (RegFac<R>::BASE) {
        if constexpr (R == 1) {
        } else if constexpr (R == 2 || R == 4 || R == 8 || R == 16) {
            Dft<R, true>::run(v);
        } else {
            odd_dft<R>(v);
        }
    } else {
        constexpr int A = RegFac<R>::A, B = RegFac<R>::B;
        float2 y[A][B];
        static_for<0, B>([&](auto m2c) {
            constexpr int m2 = decltype(m2c)::value;
            float2 col[A];
#pragma unroll
            for (int m1 = 0; m1 < A; ++m1) col[m1] = v[m1 * B + m2];
            reg_dft<A>(col);
            static_for<0, A>([&](auto k1c) {
                constexpr int k1 = decltype(k1c)::value;
                y[k1][m2] = twk<k1 * m2, R>(col[k1]);
            });
        });
#pragma unroll
        for (int k1 = 0; k1 < A; ++k1) {
            reg_dft<B>(y[k1]);
#pragma unroll
            for (int k2 = 0; k2 < B; ++k2) v[k1 + A * k2] = y[k1][k2];
        }
    }
}

// The kernel and its launcher are private to the unit that instantiates them
namespace {

template <int N1, int N2, int MODE = 0>
struct Sq {
    static constexpr int N = N1 * N2;
    static constexpr int TT = N1 > N2 ? N1 : N2;   // lanes per transform
    static constexpr int TPW = 64 / TT;            // transforms per wave
    static constexpr int P2 = N2 + 1;              // padded pass-1 row (k1 rows of N2)
    // float2 per transform, even: 16 B aligned transform buffers (the staged row flush reads float4s)
    static constexpr int LT = ((N1 * P2 > N ? N1 * P2 : N) + 1) / 2 * 2;
    // + the W_n table and the window (MODE 5: W_2n^k, k <= n, for the split step)
    static constexpr int LDS = 4 * TPW * LT + N + (MODE == 5 ? N + 1 : N / 2);
    // workgroups per CU the LDS allows, at most 3 (<= 168 VGPRs), or 4 when
    // both factors are <= 20 (the transform's registers then fit 128 VGPRs
    // without spills: 320 = 16 x 20 measured 3.4 % faster at 4 than at 3; 480 =
    // 20 x 24 spills at 128 and measured 21 % slower, profiles/r03_kbench_sq_lb4.jsonl).
    // Latency-bound, so occupancy matters.
    static constexpr int FIT = (160 * 1024) / (8 * LDS);
    static constexpr int CAP = (N1 <= 20 && N2 <= 20) ? 4 : 3;
    static constexpr int LB = FIT < CAP ? (FIT < 1 ? 1 : FIT) : CAP;
    // magnitude rows (MODE 1) are staged in LDS and flushed as one contiguous
    // run per pair: 16 B/lane when the row length is a multiple of 4 floats
    // (and the output 16 B aligned), 4 B/lane otherwise
    // (not for magnitude rows of 600 = 20 x 30 / 640 = 20 x 32: at 3 waves per
    // SIMD the held magnitudes make the 30/32-point pass spill, 1.16-1.34x
    // slower, profiles/r03_ab_sq_stage_pow.jsonl -- those keep the symmetric emit)
    static constexpr bool STG = MODE == 3 || (MODE == 1 && !(LB == 3 && (N1 > 24 || N2 > 24)));
    static constexpr bool ST16 = STG && MODE == 1 && N % 4 == 0;
};

// MODE 0 c2c rows (`pairs` = rows), MODE 5 real rows of 2n (even/odd pairs
// + split step, as k_fft_mixed); STFT frame pairs: MODE 1 |X| rows, 2 complex
// rows, 3 |X|^2 for bins 0..n/2 (as k_fft_mixed).  A wave reads its rows whole
// before it writes them, so in == out is safe.
template <int N1, int N2, int MODE>
__global__ void __launch_bounds__(256, (Sq<N1, N2, MODE>::LB)) k_stft_sq(MixIO io, long long pairs, const float2* __restrict__ gtab) {
    using S = Sq<N1, N2, MODE>;
    constexpr int n = S::N, TT = S::TT, TPW = S::TPW, P2 = S::P2, LT = S::LT;
    constexpr int W = MODE == 3 ? n / 2 + 1 : n;   // bins per row
    __shared__ __attribute__((aligned(16))) float2 sm[S::LDS];
    float2* const tab = sm + 4 * TPW * LT;
    float* const lwin = reinterpret_cast<float*>(tab + n);
    float2* const ltw = tab + n;   // MODE 5 (in the window's place)
    // pass 1's twiddles W_n^(k1 t) stored [k1][t] (t < N2): for one k1 the lanes
    // read consecutive entries (tab[k1 t] had k1-strided, bank-conflicting reads)
    for (int i = threadIdx.x; i < n; i += 256) {
        const int k1 = i / N2, tt = i - k1 * N2;
        tab[i] = gtab[k1 * tt];
        if constexpr (MODE != 0 && MODE != 5) lwin[i] = io.win[i];
    }
    if constexpr (MODE == 5) {   // the split step's W_2n^k from LDS, not a dependent global load per bin
        for (int i = threadIdx.x; i <= n; i += 256) ltw[i] = io.twn[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = lane / TT, t = lane - slot * TT;
    const bool lane_ok = slot < TPW;
    float2* const wbuf = sm + wave * TPW * LT;
    float2* const L = wbuf + (lane_ok ? slot : 0) * LT;
    __syncthreads();
    const long long step = (long long)gridDim.x * 4 * TPW;
    for (long long g = ((long long)blockIdx.x * 4 + wave) * TPW; g < pairs; g += step) {
        // pass 1: lane t < N2 of slot `slot` on row / pair q
        if (const long long q = g + slot; lane_ok && q < pairs && t < N2) {
            float2 v[N1];
            if constexpr (MODE == 0) {   // complex row q (the inverse by conjugation)
                const float2* x = reinterpret_cast<const float2*>(io.in) + q * io.in_dist + t;
#pragma unroll
                for (int m1 = 0; m1 < N1; ++m1) {
                    const float2 a = x[m1 * N2];
                    v[m1] = make_float2(a.x, a.y * io.isign);
                }
            } else if constexpr (MODE == 5) {   // real row q of length 2n: z[m] = x[2m] + i x[2m+1]
                const float* x = reinterpret_cast<const float*>(io.in) + q * io.in_dist + 2 * t;
#pragma unroll
                for (int m1 = 0; m1 < N1; ++m1) v[m1] = make_float2(x[2 * m1 * N2], x[2 * m1 * N2 + 1]);
            } else {
                // frame pair q: frame_pair()'s rule written out (through the descriptor
                // pass 1 compiled to other code at every length, slower at 960)
                const long long c = q / io.ppc, fra = 2 * (q - c * io.ppc);
                const long long st = fra * io.hop;
                const float* ra = reinterpret_cast<const float*>(io.in) + c * io.ch_stride + st;
                const float* rb = ra + io.hop;
                const long long lima = io.sig_n - st;
                const long long limb = fra + 1 < io.frames ? lima - io.hop : 0;
                if (limb >= n) {   // both frames inside the signal: base + immediate loads
                    const float* pa = ra + t;
                    const float* pb = rb + t;
#pragma unroll
                    for (int m1 = 0; m1 < N1; ++m1) {
                        const float w = lwin[m1 * N2 + t];
                        v[m1] = make_float2(pa[m1 * N2] * w, pb[m1 * N2] * w);
                    }
                } else {
#pragma unroll
                    for (int m1 = 0; m1 < N1; ++m1) v[m1] = pair_load(ra, rb, lima, limb, m1 * N2 + t, io.win, lwin);
                }
            }
            reg_dft<N1>(v);
#pragma unroll
            for (int k1 = 0; k1 < N1; ++k1) L[k1 * P2 + t] = k1 == 0 ? v[0] : cmul(v[k1], tab[k1 * N2 + t]);
        }
        xsync<64>();
        // pass 2: lane t < N1 on row k1 = t
        if (lane_ok && g + slot < pairs && t < N1) {
            float2 u[N2];
#pragma unroll
            for (int m2 = 0; m2 < N2; ++m2) u[m2] = L[t * P2 + m2];
            reg_dft<N2>(u);
#pragma unroll
            for (int k2 = 0; k2 < N2; ++k2) L[t + N1 * k2] = u[k2];
        }
        xsync<64>();
        // the wave's rows (rows a and b of each of its pairs), the whole wave on each
        const float sx = io.scale, sy = io.scale * io.isign;   // MODE 0
#pragma unroll
        for (int s = 0; s < TPW; ++s) {
            const long long q = g + s;
            if (q >= pairs) break;   // wave-uniform
            const float2* const Z = wbuf + s * LT;
            if constexpr (MODE == 0 || MODE == 5) {   // row q: scaled c2c bins, or the split step
                float2* const y = io.out + q * io.out_dist;
                for (int e = lane; e < io.nout; e += 64)
                    y[e] = MODE == 0 ? c2c_bin(Z[e], sx, sy) : r2c_split_bin(Z, e, n, ltw, io.scale);
            } else if constexpr (S::STG) {
                // Magnitude (and power) rows staged in the transform's own (now consumed) LDS
                // buffer and written as 16 B/lane stores of the pair's 2W-float run
                // (4 B/lane plain stores for power rows and rows not a multiple of 4 floats):
                // |X| of bins e and n - e of both rows from one read of Z[e], Z[n-e]
                // (conjugate symmetry), held in registers until every read is done.
                // 12-18 % faster than the 4 B/lane stores of the symmetric emit below
                // at 400 / 480 / 720 / 900 / 960 (profiles/r03_kbench_sq_stage.jsonl,
                // r03_ab_sq_stage_all.jsonl).
                constexpr int IT = (n / 2 + 1 + 63) / 64;
                float* const X = reinterpret_cast<float*>(wbuf + s * LT);
                float ma[IT], mb[IT];
#pragma unroll
                for (int i = 0; i < IT; ++i) {
                    const int e = lane + 64 * i;
                    const int ec = 2 * e <= n ? e : 0;
                    // pair_split() and row_value() written out (through them the magnitude
                    // rows' kernels compiled to other code)
                    const float2 z = Z[ec], m = Z[ec == 0 ? 0 : n - ec];
                    const float h = 0.5f;
                    const float2 xa = make_float2((z.x + m.x) * h, (z.y - m.y) * h);
                    const float2 xb = make_float2((z.y + m.y) * h, (m.x - z.x) * h);
                    ma[i] = __builtin_fmaf(xa.x, xa.x, xa.y * xa.y);
                    mb[i] = __builtin_fmaf(xb.x, xb.x, xb.y * xb.y);
                    if constexpr (MODE == 1) {
                        ma[i] = __builtin_amdgcn_sqrtf(ma[i]);
                        mb[i] = __builtin_amdgcn_sqrtf(mb[i]);
                    }
                }
                xsync<64>();   // every read of Z before the rows overwrite it
#pragma unroll
                for (int i = 0; i < IT; ++i) {
                    const int e = lane + 64 * i;
                    if (2 * e <= n) {
                        X[e] = ma[i];
                        X[W + e] = mb[i];
                        if (MODE == 1 && e != 0 && 2 * e != n) {   // power rows (MODE 3) end at bin n/2
                            X[n - e] = ma[i];
                            X[W + n - e] = mb[i];
                        }
                    }
                }
                xsync<64>();
                const long long c = q / io.ppc, fra = 2 * (q - c * io.ppc);   // as frame_pair()
                const int lim = fra + 1 < io.frames ? 2 * W : W;   // floats of the run (row b may not exist)
                float* const fo = reinterpret_cast<float*>(io.out) + c * io.out_ch_stride + fra * W;
                if (S::ST16 && io.a16) {
                    const vf4_t* const X4 = reinterpret_cast<const vf4_t*>(X);
#pragma unroll
                    for (int o = lane; o < (2 * W) / 4; o += 64)
                        if (4 * o < lim) __builtin_nontemporal_store(X4[o], reinterpret_cast<vf4_t*>(fo) + o);
                } else {   // plain stores: runs that are not whole lines merge in L2
                    for (int o = lane; o < lim; o += 64) fo[o] = X[o];
                }
            } else if constexpr (n < 900) {
                // Magnitude / complex rows of real frames from their conjugate symmetry:
                // bins e and n - e of both rows from one read of Z[e], Z[n - e] and one
                // split/magnitude (|X[n-e]| = |X[e]|, X[n-e] = conj X[e], bit-identical
                // to computing bin n - e on its own): 12-18 % faster than emitting each
                // row bin by bin (480-point rows 6.00 -> 4.92 ms for 32 ch x 10 min at
                // 48 kHz, profiles/r03_kbench_sq_sym.jsonl)
                static_assert(MODE == 2 || (MODE == 1 && (n == 600 || n == 640)),
                              "symmetric emit: complex rows below 900, and the magnitude rows that are not staged");
                const FramePair p = frame_pair(io, q, W);
                RowValue<MODE>* const o = reinterpret_cast<RowValue<MODE>*>(io.out) + p.out;
                for (int e = lane; 2 * e <= n; e += 64) {
                    float2 xa, xb;
                    pair_split(Z[e], Z[e == 0 ? 0 : n - e], &xa, &xb);
                    const bool mir = e != 0 && 2 * e != n;
                    const auto va = row_value<MODE>(xa), vb = row_value<MODE>(xb);
                    o[e] = va;
                    if (mir) o[n - e] = row_mirror(va);
                    if (p.has_b) {
                        o[W + e] = vb;
                        if (mir) o[W + n - e] = row_mirror(vb);
                    }
                }
            } else {
                // bin e of both rows from one read of Z[e] and Z[n - e], bin by bin (2 %
                // faster than the symmetric emit at n >= 900: 960-pt 5.83 -> 4.57 ms;
                // 400 / 480 measured 1.3-1.4x slower that way, profiles/r02_ab_sq_emit.jsonl)
                static_assert(MODE == 2 && n >= 900, "per-bin emit: complex rows of 900 and 960 (power and magnitude rows are staged)");
                const FramePair p = frame_pair(io, q, W);
                float2* const o = io.out + p.out;
#pragma unroll 4
                for (int e = lane; e < W; e += 64) {
                    float2 xa, xb;
                    pair_split(Z[e], Z[e == 0 ? 0 : n - e], &xa, &xb);
                    o[e] = xa;
                    if (p.has_b) o[W + e] = xb;
                }
            }
        }
        xsync<64>();   // the next group's pass 1 overwrites the buffers
    }
}

template <int N1, int N2, int MODE>
hipError_t run_stft_sq(const MixIO& io, long long pairs, hipStream_t s) {
    const float2* tab = twiddle_table(N1 * N2);
    if (!tab) return hipErrorOutOfMemory;
    constexpr int TPW = Sq<N1, N2, MODE>::TPW;
    // batched C2C (MODE 0) and R2C (MODE 5) rows: a non-persistent grid, each
    // wave's transforms once -- -4..-11 % (C2C 320..960) and -7..-14 % (R2C 400 /
    // 480 / 960) on the same buffers, bit-identical; the STFT modes measured 6-10 %
    // slower that way and stay persistent (profiles/r05_ab2_analytic_mixed_grid.jsonl).
    // Knob MIX_TPW = 0 / 1 forces the persistent / non-persistent grid (A/B)
    const bool once = knob(KNOB_MIX_TPW, (MODE == 0 || MODE == 5) ? 1 : 0) == 1;
    const int grid = mixed_grid(once, (const void*)k_stft_sq<N1, N2, MODE>, 0, (pairs + 4 * TPW - 1) / (4 * TPW));
    hipLaunchKernelGGL((k_stft_sq<N1, N2, MODE>), dim3(grid), dim3(256), 0, s, io, pairs, tab);
    return hipGetLastError();
}

// Lengths the register kernel takes (n, N1, N2; N1, N2 <= 32): speech and
// audio frames of 20 / 25 / 30 / 60 ms at 16, 32, 44.1 and 48 kHz
#define VVH_SQ_LENGTHS(X) \
    X(320, 16, 20) X(400, 20, 20) X(441, 21, 21) X(480, 20, 24) X(600, 20, 30) X(640, 20, 32) \
    X(720, 24, 30) X(800, 25, 32) X(900, 30, 30) X(960, 30, 32)
// half lengths of the real (R2C) rows: the list plus 200 and 240 (R2C at 400 / 480)
#define VVH_SQ_HALF_ONLY(X) X(200, 10, 20) X(240, 12, 20)

// f(integral_constant N1, N2) for length n of the list (HALF: or of the half
// lengths); false when n is not in it or knob STFT_SQ = 0 (the plan kernel, A/B)
template <bool HALF, class F>
bool sq_dispatch(long long n, F&& f) {
    if (knob(KNOB_STFT_SQ, 1) == 0) return false;
#define VVH_SQ_CASE(L, A, B) \
    case L: f(std::integral_constant<int, A>{}, std::integral_constant<int, B>{}); return true;
    switch (n) {
        VVH_SQ_LENGTHS(VVH_SQ_CASE)
        default: break;
    }
    if constexpr (HALF) {
        switch (n) {
            VVH_SQ_HALF_ONLY(VVH_SQ_CASE)
            default: break;
        }
    }
#undef VVH_SQ_CASE
    return false;
}

}  // namespace

}  // namespace vvh
