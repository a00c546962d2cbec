// pitch_kernels.hip -- per-frame fundamental frequency by YIN (de Cheveigne &
// Kawahara 2002, steps 2-5) for gfx950, over rows or over the frames of a
// signal.  include/vv_dsp/features/pitch.h states the definition; this file
// states how it is computed.
//
// One wave per row.  The row (of a FrameSrc: a frame is read through
// frame_sample, frame_src.hpp, as k_fetch_frames reads it) goes to the wave's
// own piece of LDS once, as f64 where four rows of f64 fit 64 KiB (the
// conversion is exact, so both storages give the same bits) and as f32 beyond.
// No workgroup barrier is needed: a wave reads only what it wrote.
//
// Difference function.  Lane l owns T adjacent lags t0 = base + T l .. t0 + T - 1
// and walks j = 0 .. W - 1 in runs of R = PITCH_RUN: a run loads x[j .. j + R) (the
// same address in every lane, 16 bytes per read) and the window
// x[j + t0 .. j + t0 + R + T - 1), R + R + T - 1 values for R T terms, each term
// one f64 subtract and one f64 FMA.  T is odd, so the 64 windows start
// T elements apart on distinct banks.  Every lag has one accumulator that takes
// its W terms in ascending j: the sum depends on (n, tau_max) alone, not on T,
// the storage, the batch, the stride, the requested outputs or the entry point.
// Lags past tau_max shift down to the last T lags (duplicate work, same bits).
//
// CMND and decision.  d(tau) goes to LDS; blocks of 64 lags take an inclusive
// wave scan (shuffle-up, 1 2 4 .. 32) on top of the carry of the blocks before,
// d'(tau) = d(tau) tau / c(tau) overwrites d(tau) and is the exported curve.  The
// threshold search is a ballot per block of 64 lags, the descent a ballot of the
// lanes whose right neighbour is not smaller, the unvoiced minimum a per-lane
// strictly-smaller scan in ascending tau and an xor butterfly on (value, lag)
// that prefers the lower lag at equal values.
#include "frame_src.hpp"
#include "wave_sync.hpp"

#include <climits>
#include <cmath>

namespace vvh {

namespace {

constexpr int PITCH_RUN = 8;                     // R: consecutive j per load group
constexpr size_t PITCH_LDS_SMALL = 64u << 10;    // dynamic LDS a launch gets without asking

struct PitchAt {
    long long plane, cmnd;   // where the row's values go in the planes / in cmnd
};
using PitchRow = FrameRow<PitchAt>;

__device__ __forceinline__ PitchRow pitch_row(const FrameSrc& s, const PitchOut& o, long long row) {
    return frame_row(
        s, row, [&] { return PitchAt{row, row * o.cmnd_row_stride}; },
        [&](unsigned ch, unsigned f) {
            return PitchAt{ch * o.ch_stride + f, ch * o.cmnd_ch_stride + f * o.cmnd_row_stride};
        });
}

// The run x[j .. j + R): j is a multiple of R and the row 16-byte aligned, so it
// is read 16 bytes at a time (ds_read_b128; the window's start is only aligned
// to its element and is left to the compiler, which pairs its reads).
template <class S>
__device__ __forceinline__ void pitch_load_run(const S* __restrict__ p, double (&a)[PITCH_RUN]) {
    constexpr int V = 16 / (int)sizeof(S);
    typedef S vec __attribute__((ext_vector_type(V)));
    const vec* q = reinterpret_cast<const vec*>(__builtin_assume_aligned(p, 16));
#pragma unroll
    for (int r = 0; r < PITCH_RUN / V; ++r) {
        const vec v = q[r];
#pragma unroll
        for (int e = 0; e < V; ++e) a[r * V + e] = (double)v[e];
    }
}

// d(tau), tau <= tau_max, of the row xs[0, W + tau_max) into d
template <int T, class S>
__device__ __forceinline__ void pitch_difference(const S* __restrict__ xs, double* __restrict__ d, int tau_max, int W,
                                                 int lane) {
#pragma clang fp contract(off)
    constexpr int R = PITCH_RUN;
    const int last = tau_max - (T - 1);   // >= 0: the launcher takes T = 3 for tau_max < 192, and tau_max >= 3
    for (int base = 0; base <= tau_max; base += 64 * T) {
        const int t0 = base + T * lane < last ? base + T * lane : last;
        const S* xw = xs + t0;
        double acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = 0.0;
        int j = 0;
#pragma unroll 1
        for (; j + R <= W; j += R) {
            double a[R], w[R + T - 1];
            pitch_load_run<S>(xs + j, a);
#pragma unroll
            for (int k = 0; k < R + T - 1; ++k) w[k] = (double)xw[j + k];
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const double df = a[r] - w[r + t];
                    acc[t] = __builtin_fma(df, df, acc[t]);
                }
            }
        }
        for (; j < W; ++j) {
            const double a = (double)xs[j];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const double df = a - (double)xw[j + t];
                acc[t] = __builtin_fma(df, df, acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) d[t0 + t] = acc[t];
    }
}

// d -> d' in place (and into cmnd when wanted); returns c(tau_max) in every lane
__device__ __forceinline__ double pitch_cmnd(double* __restrict__ d, int tau_max, float* __restrict__ cmnd, int lane) {
#pragma clang fp contract(off)
    double carry = 0.0;
    for (int b = 0; b <= tau_max; b += 64) {
        const int tau = b + lane;
        const bool act = tau <= tau_max;
        const double dv = act ? d[tau] : 0.0;
        double v = tau == 0 ? 0.0 : dv;   // c starts at k = 1
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const double u = __shfl_up(v, m);
            if (lane >= m) v += u;
        }
        const double c = carry + v;
        const double q = (tau == 0 || c == 0.0) ? 1.0 : dv * (double)tau / c;
        if (act) {
            d[tau] = q;
            if (cmnd) cmnd[tau] = (float)q;
        }
        carry = __shfl(c, 63);   // lanes past tau_max added 0
    }
    return carry;
}

struct PitchResult {
    float f0, ap;
    unsigned lag;
};

// the decision on d' (LDS), the same in every lane
__device__ __forceinline__ PitchResult pitch_decide(const double* __restrict__ q, const PitchCfg& cfg, int lane) {
#pragma clang fp contract(off)
    const int tau_min = cfg.tau_min, tau_max = cfg.tau_max;
    int tau = -1;
    for (int b = tau_min; b <= tau_max && tau < 0; b += 64) {
        const int t = b + lane;
        const bool hit = t <= tau_max && q[t] < cfg.threshold;
        const unsigned long long m = __ballot(hit);
        if (m) tau = b + __builtin_ctzll(m);
    }
    if (tau >= 0) {
        for (;;) {   // walk right while the next value is smaller
            const int t = tau + lane;
            const bool down = t + 1 <= tau_max && q[t + 1] < q[t];
            const unsigned long long stop = __ballot(!down);
            if (stop) {
                tau += __builtin_ctzll(stop);
                break;
            }
            tau += 64;
        }
        const double b = q[tau];
        double off = 0.0;
        if (tau - 1 >= 1 && tau + 1 <= tau_max) {
            const double a = q[tau - 1], c = q[tau + 1];
            const double den = (a - 2.0 * b) + c;
            if (a >= b && c >= b && den > 0.0) off = (a - c) / (2.0 * den);
        }
        return {(float)(cfg.sample_rate / ((double)tau + off)), (float)b, (unsigned)tau};
    }
    double bv = INFINITY;
    int bi = INT_MAX;
    for (int t = tau_min + lane; t <= tau_max; t += 64) {
        const double v = q[t];
        if (v < bv) {
            bv = v;
            bi = t;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (ov < bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    return {0.0f, (float)bv, (unsigned)bi};
}

template <int T, class S, bool INSIDE>
__device__ __forceinline__ void pitch_wave_row(const FrameSrc& src, const PitchRow& rw, const PitchCfg& cfg,
                                               const PitchOut& out, S* xs, double* d, int lane) {
    const int n = (int)src.len;
    for (int i = lane; i < n; i += 64) xs[i] = (S)frame_sample<INSIDE>(src, rw, i);
    wave_sync();
    pitch_difference<T, S>(xs, d, cfg.tau_max, cfg.W, lane);
    wave_sync();
    const double total = pitch_cmnd(d, cfg.tau_max, out.cmnd ? out.cmnd + rw.at.cmnd : nullptr, lane);
    wave_sync();
    PitchResult r = {0.0f, NAN, 0u};   // a non-finite sample: c(tau_max) holds every one of them
    if (isfinite(total)) r = pitch_decide(d, cfg, lane);
    if (lane == 0) {
        if (out.f0) out.f0[rw.at.plane] = r.f0;
        if (out.aperiodicity) out.aperiodicity[rw.at.plane] = r.ap;
        if (out.lag) out.lag[rw.at.plane] = r.lag;
    }
}

// one wave per row, wpb rows per workgroup; row_bytes of LDS per wave: the row, then d
template <int T, class S>
__global__ void __launch_bounds__(256) k_pitch(FrameSrc src, PitchCfg cfg, PitchOut out, int wpb, int x_bytes,
                                               int row_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pitch_lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * wpb + wave;
    if (row >= src.rows) return;
    unsigned char* mine = pitch_lds + (size_t)wave * row_bytes;
    S* xs = reinterpret_cast<S*>(mine);
    double* d = reinterpret_cast<double*>(mine + x_bytes);
    const PitchRow rw = pitch_row(src, out, row);
    if (rw.inside) pitch_wave_row<T, S, true>(src, rw, cfg, out, xs, d, lane);
    else pitch_wave_row<T, S, false>(src, rw, cfg, out, xs, d, lane);
}

template <int T, class S>
hipError_t pitch_launch(const FrameSrc& src, const PitchCfg& cfg, const PitchOut& out, hipStream_t s) {
    const size_t x_bytes = ((size_t)src.len * sizeof(S) + 15) / 16 * 16;
    const size_t row_bytes = x_bytes + ((size_t)(cfg.tau_max + 1) * sizeof(double) + 15) / 16 * 16;
    size_t wpb = PITCH_LDS_SMALL / row_bytes;
    wpb = wpb > 4 ? 4 : wpb < 1 ? 1 : wpb;
    const size_t lds = wpb * row_bytes;
    auto kern = k_pitch<T, S>;
    if (lds > PITCH_LDS_SMALL) {   // one long row: up to 64 KiB of samples and 64 KiB of lags
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)PITCH_LDS_MAX);
        if (e != hipSuccess) return e;
    }
    const long long blocks = (src.rows + (long long)wpb - 1) / (long long)wpb;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3((unsigned)(64 * wpb)), lds, s, src, cfg, out, (int)wpb,
                       (int)x_bytes, (int)row_bytes);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pitch(const FrameSrc& src, const PitchCfg& cfg, const PitchOut& out, bool f32_rows, hipStream_t s) {
    if (src.rows <= 0 || !out.any()) return hipSuccess;
    if (src.len <= 0 || src.len > PITCH_MAX_FRAME || src.rows >= (1LL << 31) || src.frames <= 0 || cfg.tau_min < 2 ||
        cfg.tau_min >= cfg.tau_max || cfg.tau_max > PITCH_MAX_LAG || cfg.W < 1 ||
        (long long)cfg.W + cfg.tau_max != src.len)
        return hipErrorInvalidValue;
    // lags per lane: the fewer lane-lags a row's passes take, the better; 3 for short ranges
    const int lags = cfg.tau_max + 1;
    const bool five = lags > 192 && (lags + 319) / 320 * 5 <= (lags + 191) / 192 * 3;
    // f64 samples where four rows fit the small LDS
    const bool f64 = !f32_rows && ((size_t)src.len + (size_t)lags) * sizeof(double) + 32 <= PITCH_LDS_SMALL / 4;
    if (five) return f64 ? pitch_launch<5, double>(src, cfg, out, s) : pitch_launch<5, float>(src, cfg, out, s);
    return f64 ? pitch_launch<3, double>(src, cfg, out, s) : pitch_launch<3, float>(src, cfg, out, s);
}

}  // namespace vvh
