// mixed_plan.hip -- the LDS Stockham kernel for 7-smooth lengths that are not
// powers of two (n = 2^a 3^b 5^c 7^d, 6 <= n <= 4096): one transform per T
// threads runs the passes of its length's plan (mixed_plan.hpp) in LDS.  Rows of
// every MixIO mode; the inverse is conj(FFT(conj x)), then the caller's scale.
//
// Loads and stores are lane-contiguous (coalesced); a transform is read whole
// into LDS before any of it is written, so in == out is safe.
#include "mixed_plan.hpp"

namespace vvh {

#ifndef VVH_MIX_LB
#define VVH_MIX_LB 1
#endif

namespace {

// One transform's points in and out (MixIO's modes)
template <int MODE>
struct Row {
    const float2* cin;      // MODE 0
    const float* ra;        // MODE 4 / 5: the real row
    FramePair p;            // MODE 1 / 2 / 3
    const float* win;
    RowValue<MODE> *oa, *ob;   // the transform's row (rows a and b of a frame pair)

    __device__ __forceinline__ void open(const MixIO& io, long long f, int n) {
        if constexpr (MODE == 0) {
            cin = reinterpret_cast<const float2*>(io.in) + f * io.in_dist;
            oa = io.out + f * io.out_dist;
        } else if constexpr (MODE == 4 || MODE == 5) {
            ra = reinterpret_cast<const float*>(io.in) + f * io.in_dist;
            oa = io.out + f * io.out_dist;
        } else {
            const long long w = MODE == 3 ? n / 2 + 1 : n;
            p = frame_pair(io, f, w);
            win = io.win;
            oa = reinterpret_cast<RowValue<MODE>*>(io.out) + p.out;
            ob = oa + w;
        }
    }
    __device__ __forceinline__ float2 load(const MixIO& io, int e) const {
        if constexpr (MODE == 0) {   // the inverse conjugates (a sign, no branch)
            const float2 x = cin[e];
            return make_float2(x.x, x.y * io.isign);
        } else if constexpr (MODE == 4) {
            return make_float2(ra[e], 0.0f);
        } else if constexpr (MODE == 5) {   // z[m] = x[2m] + i x[2m+1]
            return make_float2(ra[2 * e], ra[2 * e + 1]);
        } else {
            return pair_load(p.ra, p.rb, p.lima, p.limb, e, win, win);
        }
    }
    // all outputs of the transform in buf (natural order), lane-contiguous
    template <int T>
    __device__ __forceinline__ void emit(const MixIO& io, const float2* buf, int t, int n) const {
        if constexpr (MODE == 0 || MODE == 4) {
            const float sx = io.scale, sy = io.scale * io.isign;
            for (int e = t; e < io.nout; e += T) oa[e] = c2c_bin(buf[e], sx, sy, MODE == 4 && 2 * e == n);
        } else if constexpr (MODE == 5) {
            for (int e = t; e < io.nout; e += T) oa[e] = r2c_split_bin(buf, e, n, io.twn, io.scale);
        } else {
            const int lim = MODE == 3 ? n / 2 + 1 : n;
            for (int e = t; e < lim; e += T) {
                float2 xa, xb;
                pair_split(buf[e], buf[e == 0 ? 0 : n - e], &xa, &xb);
                oa[e] = row_value<MODE>(xa);
                if (p.has_b) ob[e] = row_value<MODE>(xb);
            }
        }
    }
};

// Copy a transform in (a plain strided loop measured 1.3x faster than loading
// all of a thread's points first: 400-point rows 0.26 vs 0.35 ms per GiB).
template <int T, int MODE>
__device__ __forceinline__ void mload(float2* buf, int t, int n, const MixIO& io, const Row<MODE>& row, bool act) {
    if (act)
        for (int e = t; e < n; e += T) buf[e] = row.load(io, e);
    xsync<T>();
}

template <int T, int MODE>
__global__ void __launch_bounds__(256, VVH_MIX_LB)
k_fft_mixed(MixedPlan pl, MixIO io, long long batch, const float2* __restrict__ gtab) {
    constexpr int F = 256 / T;
    extern __shared__ float2 sm[];
    const int n = pl.n;
    float2* tab = sm;
    const int lt = threadIdx.x, slot = lt / T, t = lt % T;
    float2* buf = sm + n + slot * n;
    for (int i = lt; i < n; i += 256) tab[i] = gtab[i];
    __syncthreads();
    const long long stride = (long long)gridDim.x * F;
    for (long long f0 = (long long)blockIdx.x * F; f0 < batch; f0 += stride) {
        const long long f = f0 + slot;
        const bool act = f < batch;
        Row<MODE> row;
        if (act) row.open(io, f, n);
        mload<T, MODE>(buf, t, n, io, row, act);
        VVH_MIX_RUN_PASSES(T, buf, tab, t, n, pl, act)
        if (act) row.template emit<T>(io, buf, t, n);
        xsync<T>();   // the next transform's loads overwrite buf
    }
}

template <int MODE>
hipError_t run_mixed_mode(const MixedPlan& pl, const MixIO& io, long long batch, hipStream_t s) {
    const float2* tab = twiddle_table(pl.n);
    if (!tab) return hipErrorOutOfMemory;
    return with_mixed_threads(pl.n, [&](auto tc) {
        constexpr int T = decltype(tc)::value, F = 256 / T;
        const size_t lds = sizeof(float2) * (size_t)pl.n * (1 + F);
        // knob MIX_TPW = 1: a non-persistent grid (A/B; 1000-4000-point C2C measured
        // 8-22 % slower that way, profiles/r05_ab2_analytic_mixed_grid.jsonl)
        const int grid = mixed_grid(knob(KNOB_MIX_TPW, 0) == 1, (const void*)k_fft_mixed<T, MODE>, lds, (batch + F - 1) / F);
        hipLaunchKernelGGL((k_fft_mixed<T, MODE>), dim3(grid), dim3(256), lds, s, pl, io, batch, tab);
        return hipGetLastError();
    });
}

}  // namespace

hipError_t run_mixed(int mode, const MixedPlan& pl, const MixIO& io, long long batch, hipStream_t s) {
    switch (mode) {
        case 0: return run_mixed_mode<0>(pl, io, batch, s);
        case 1: return run_mixed_mode<1>(pl, io, batch, s);
        case 2: return run_mixed_mode<2>(pl, io, batch, s);
        case 3: return run_mixed_mode<3>(pl, io, batch, s);
        case 4: return run_mixed_mode<4>(pl, io, batch, s);
        default: return run_mixed_mode<5>(pl, io, batch, s);
    }
}

}  // namespace vvh
