// shape_kernels.hip -- per-frame spectral shape descriptors of power rows for
// gfx950: energy, centroid, spread, skewness, kurtosis, flatness, roll-off, flux,
// crest and peak bin.  include/vv_dsp/features/spectral_shape.h states the
// definitions; this file states how they are computed.
//
// One wave per run of consecutive rows of one group, up to four waves per
// workgroup.  A row is loaded once, 16 bytes per lane and load where the base and
// the pitch allow it and 4 bytes otherwise, turned into weights (sqrtf with
// `magnitude`; a negative weight becomes a NaN) and written to the wave's own
// piece of LDS -- the same floats on both paths.  No workgroup barrier is
// needed: a wave reads only what it wrote.
//
// Ownership.  With t the smallest odd number >= K / 64, lane l owns bins
// [l t, l t + t): t is odd, so the 64 lanes read LDS t floats apart on distinct
// banks.  Up to t = 9 (K <= 576) a lane copies its bins to registers and every
// pass runs from them; beyond, the passes read LDS.  Both give the same bits:
// the passes are one piece of code over either storage.
//
// Sums.  A lane adds its bins of the band in ascending k in f64, the 64 lanes
// combine by an xor butterfly (32, 16, .. 1): the order depends on (K, k_min,
// k_max) alone.  Pass 1: S0, S1 = sum k w, the sum and the product of w' =
// max(w, floor), the squared difference to the previous row and the running
// maximum, a (value, index) pair seeded with (w[k_min], k_min) in every lane
// (stats_kernels.hip's rule).  Pass 2, about c = S1 / S0: m2, m3, m4.
//
// Flatness.  The product of the w' is an f64 mantissa in [0.5, 1) and an integer
// exponent (frexp), renormalised after every multiply, the butterfly's included;
// one log and one exp per row.
//
// Roll-off.  An inclusive scan (shuffle-up 1, 2, .. 32) of the lanes' S0 parts
// gives every lane the sum below its bins; the lane adds its bins to it one by
// one and notes the first k at which the sum reaches T = rolloff S0; a ballot
// picks the lowest such lane.  The running sum never decreases inside a lane, so
// that is the smallest k with C_k >= T; no lane: k_max.
//
// Flux.  A wave keeps the previous row of its run (registers or a second piece of
// LDS); the row before the run is read once, so a row is fetched 1 + 1 / run
// times.  Kernels without flux walk the same runs of SHAPE_RUN rows: a wave's
// set-up (its run's place among the groups, a 64-bit division) is paid once per
// run (one-row waves were slower in a one-off A/B: DESIGN.md section 4,
// "Spectral shape").
//
// The kernel is specialised on the storage and on what is wanted: the second
// pass (spread, skewness, kurtosis), flatness, roll-off and flux each drop out
// of a kernel whose mask lacks them.
#include "vvhip_internal.hpp"
#include "wave_sync.hpp"

#include <cmath>
#include <cstdint>

namespace vvh {

namespace {

constexpr int SHAPE_RUN = 8;                     // rows of a run
constexpr int SHAPE_REG_T = 9;                   // bins per lane up to which they sit in registers
constexpr size_t SHAPE_LDS_SMALL = 64u << 10;    // dynamic LDS a launch gets without asking

struct ShapeExt {     // the running maximum
    float v;
    unsigned i;
};

__device__ __forceinline__ ShapeExt shape_max(ShapeExt a, ShapeExt b) {
    const bool take = b.v > a.v || (b.v == a.v && b.i < a.i);
    return {take ? b.v : a.v, take ? b.i : a.i};
}

__device__ __forceinline__ float shape_weight(float p, int magnitude) {
    const float w = magnitude ? sqrtf(p) : p;
    return w < 0.0f ? NAN : w;
}

// m 2^e <- (m 2^e) (m2 2^e2), m back in [0.5, 1): the product of two mantissas lies
// in [0.25, 1), so the renormalisation is at most one exact doubling (what frexp
// would return, without its two instructions); a NaN or an infinity stays
__device__ __forceinline__ void shape_flat_mul(double& m, int& e, double m2, int e2) {
    const double p = m * m2;
    const bool small = p < 0.5;
    m = small ? p + p : p;
    e += e2 - (small ? 1 : 0);
}

// the row at src -> its weights at dst (LDS, 16-byte aligned)
template <bool VEC>
__device__ __forceinline__ void shape_stage(const float* __restrict__ src, float* __restrict__ dst, int K,
                                            int magnitude, int lane) {
    int done = 0;
    if (VEC) {
        const int n4 = K >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int i = lane; i < n4; i += 64) {
            float4 v = s4[i];
            v.x = shape_weight(v.x, magnitude);
            v.y = shape_weight(v.y, magnitude);
            v.z = shape_weight(v.z, magnitude);
            v.w = shape_weight(v.w, magnitude);
            d4[i] = v;
        }
        done = n4 << 2;
    }
    for (int i = done + lane; i < K; i += 64) dst[i] = shape_weight(src[i], magnitude);
}

struct ShapeArgs {
    const float* rows;
    long long nrows, pitch, rpg, runs_per_group, nruns;
    int run_len, wpb, row_floats, vec;
};

// fn(k, i) for the lane's bins k = a + i of the band [lo, hi), in ascending k
template <bool REG, class F>
__device__ __forceinline__ void shape_bins(int a, int lo, int hi, F&& fn) {
    if (REG) {
#pragma unroll
        for (int i = 0; i < SHAPE_REG_T; ++i) {
            const int k = a + i;
            if (k >= lo && k < hi) fn(k, i);
        }
    } else {
        for (int k = lo; k < hi; ++k) fn(k, 0);
    }
}

// At least four waves per SIMD (128 registers): left alone, the variants with most
// outputs take up to 160 and run three; capped, four of the 32 variants spill 8 to
// 44 bytes per lane (the compiler's kernel-resource-usage remarks print each variant's registers and scratch)
// and all ten outputs were still faster in a one-off A/B (DESIGN.md section 4,
// "Spectral shape").
template <bool REG, bool MOM, bool FLAT, bool ROLL, bool FLUX>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) k_shape(ShapeArgs A, ShapeCfg cfg, ShapeOut out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float shape_lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long run = (long long)blockIdx.x * A.wpb + wave;
    if (run >= A.nruns) return;
    const long long g = run / A.runs_per_group;
    const long long f0 = (run - g * A.runs_per_group) * A.run_len;
    long long f1 = f0 + A.run_len < A.rpg ? f0 + A.run_len : A.rpg;
    if (g * A.rpg + f1 > A.nrows) f1 = A.nrows - g * A.rpg;   // the last group may be short
    if (f0 >= f1) return;

    constexpr int BUFS = (!REG && FLUX) ? 2 : 1;
    float* cur = shape_lds + (size_t)wave * BUFS * A.row_floats;
    float* prev = cur + (BUFS - 1) * A.row_floats;   // LDS storage with flux: the other buffer
    const int K = cfg.K, T = ((K + 63) >> 6) | 1;
    const int a = lane * T;
    const int lo = a > cfg.k_min ? a : cfg.k_min;
    const int hi = a + T < cfg.k_max + 1 ? a + T : cfg.k_max + 1;
    const double B = (double)(cfg.k_max - cfg.k_min + 1);

    float w[SHAPE_REG_T], pw[SHAPE_REG_T];   // REG: the lane's bins of the row and of the row before
#pragma unroll
    for (int i = 0; i < SHAPE_REG_T; ++i) w[i] = pw[i] = 0.0f;

    auto stage = [&](long long f, float* dst) {
        const float* src = A.rows + (g * A.rpg + f) * A.pitch;
        if (A.vec) shape_stage<true>(src, dst, K, cfg.magnitude, lane);
        else shape_stage<false>(src, dst, K, cfg.magnitude, lane);
        wave_sync();
    };
    auto to_regs = [&](const float* buf, float (&r)[SHAPE_REG_T]) {
#pragma unroll
        for (int i = 0; i < SHAPE_REG_T; ++i) r[i] = (i < T && a + i < K) ? buf[a + i] : 0.0f;
    };

    if (FLUX && f0 > 0) {   // the row before the run, read once
        stage(f0 - 1, prev);
        if (REG) {
            to_regs(prev, pw);
            wave_sync();
        }
    }

    for (long long f = f0; f < f1; ++f) {
        stage(f, cur);
        if (REG) to_regs(cur, w);
        auto wv = [&](int k, int i) { return REG ? w[i] : cur[k]; };
        auto pv = [&](int k, int i) { return REG ? pw[i] : prev[k]; };

        // pass 1
        double s0 = 0.0, s1 = 0.0, sf = 0.0, fl = 0.0, fm = 1.0;
        int fe = 0;
        const float seed = cur[cfg.k_min];
        ShapeExt mx = {seed, (unsigned)cfg.k_min};
        const bool first = f == 0;
        shape_bins<REG>(a, lo, hi, [&](int k, int i) {
            const float x = wv(k, i);
            const double d = (double)x;
            s0 += d;
            s1 = __builtin_fma((double)k, d, s1);   // k w is exact: the fused form adds the same term
            if (x > mx.v) mx = {x, (unsigned)k};
            if (FLAT) {
                const float xf = x < cfg.floor ? cfg.floor : x;
                const double df = (double)xf;
                sf += df;
                int ex;
                const double mt = frexp(df, &ex);
                shape_flat_mul(fm, fe, mt, ex);
            }
            if (FLUX) {
                const double df = d - (double)pv(k, i);
                fl = __builtin_fma(df, df, fl);
            }
        });
        const double part0 = s0;
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            s0 += __shfl_xor(s0, m);
            s1 += __shfl_xor(s1, m);
            const ShapeExt o = {__shfl_xor(mx.v, m), __shfl_xor(mx.i, m)};
            mx = shape_max(mx, o);
            if (FLAT) {
                sf += __shfl_xor(sf, m);
                const double om = __shfl_xor(fm, m);
                const int oe = __shfl_xor(fe, m);
                shape_flat_mul(fm, fe, om, oe);
            }
            if (FLUX) fl += __shfl_xor(fl, m);
        }
        const double c = s1 / s0;

        // pass 2, about c
        double m2 = 0.0, m3 = 0.0, m4 = 0.0;
        if (MOM && s0 != 0.0) {
            shape_bins<REG>(a, lo, hi, [&](int k, int i) {
                const double x = (double)wv(k, i);
                const double d = (double)k - c;
                const double d2 = d * d;
                m2 = __builtin_fma(d2, x, m2);
                m3 = __builtin_fma(d2 * d, x, m3);
                m4 = __builtin_fma(d2 * d2, x, m4);
            });
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                m2 += __shfl_xor(m2, m);
                m3 += __shfl_xor(m3, m);
                m4 += __shfl_xor(m4, m);
            }
        }

        // roll-off
        int kr = cfg.k_max;
        if (ROLL) {
            double v = part0;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const double u = __shfl_up(v, m);
                if (lane >= m) v += u;
            }
            double below = __shfl_up(v, 1);
            if (lane == 0) below = 0.0;
            const double thr = cfg.rolloff * s0;
            int hit = -1;
            shape_bins<REG>(a, lo, hi, [&](int k, int i) {
                below += (double)wv(k, i);
                if (hit < 0 && below >= thr) hit = k;
            });
            const unsigned long long any = __ballot(hit >= 0);
            if (any) kr = __shfl(hit, (int)__builtin_ctzll(any));
        }

        if (lane == 0) {
            const long long at = g * out.group_stride + f;
            auto fo = [&](int k) { return static_cast<float*>(out.p[k]) + at; };
            const bool none = s0 == 0.0;
            const double hz = cfg.sample_rate, nf = cfg.n_fft;
            if (out.p[SHAPE_ENERGY]) *fo(SHAPE_ENERGY) = (float)s0;
            if (out.p[SHAPE_CENTROID]) *fo(SHAPE_CENTROID) = none ? 0.0f : (float)(c * hz / nf);
            if (MOM) {
                const double var = m2 / s0;
                const double sd = sqrt(var);
                const bool flat = none || m2 == 0.0;
                if (out.p[SHAPE_SPREAD]) *fo(SHAPE_SPREAD) = none ? 0.0f : (float)(sd * hz / nf);
                if (out.p[SHAPE_SKEW]) *fo(SHAPE_SKEW) = flat ? 0.0f : (float)((m3 / s0) / (var * sd));
                if (out.p[SHAPE_KURT]) *fo(SHAPE_KURT) = flat ? 0.0f : (float)((m4 / s0) / (var * var));
            }
            if (FLAT && out.p[SHAPE_FLATNESS]) {
                const double lg = (log(fm) + (double)fe * 0.69314718055994530942) / B;
                *fo(SHAPE_FLATNESS) = (float)(exp(lg) / (sf / B));
            }
            if (ROLL && out.p[SHAPE_ROLLOFF]) *fo(SHAPE_ROLLOFF) = (float)((double)kr * hz / nf);
            if (FLUX && out.p[SHAPE_FLUX]) *fo(SHAPE_FLUX) = first ? 0.0f : (float)sqrt(fl);
            if (out.p[SHAPE_CREST]) *fo(SHAPE_CREST) = none ? 0.0f : (float)((double)mx.v / (s0 / B));
            if (out.p[SHAPE_PEAK]) static_cast<unsigned*>(out.p[SHAPE_PEAK])[at] = mx.i;
        }

        wave_sync();   // the passes' LDS reads stay above the next row's writes
        if (FLUX) {
            if (REG) {
#pragma unroll
                for (int i = 0; i < SHAPE_REG_T; ++i) pw[i] = w[i];
            } else {
                float* t = cur;
                cur = prev;
                prev = t;
            }
        }
    }
}

template <bool REG, bool MOM, bool FLAT, bool ROLL, bool FLUX>
hipError_t shape_go(ShapeArgs A, const ShapeCfg& cfg, const ShapeOut& out, hipStream_t s) {
    const size_t bufs = (!REG && FLUX) ? 2 : 1;
    const size_t wave_bytes = bufs * (size_t)A.row_floats * sizeof(float);
    size_t wpb = SHAPE_LDS_SMALL / wave_bytes;
    wpb = wpb > 4 ? 4 : wpb < 1 ? 1 : wpb;
    const size_t lds = wpb * wave_bytes;
    auto kern = k_shape<REG, MOM, FLAT, ROLL, FLUX>;
    if (lds > SHAPE_LDS_SMALL) {   // the longest rows with flux: two buffers of 8196 floats
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    A.wpb = (int)wpb;
    const long long blocks = (A.nruns + (long long)wpb - 1) / (long long)wpb;
    if (blocks >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3((unsigned)(64 * wpb)), lds, s, A, cfg, out);
    return hipGetLastError();
}

template <bool... Bs>
hipError_t shape_pick(const bool* want, const ShapeArgs& A, const ShapeCfg& cfg, const ShapeOut& out, hipStream_t s) {
    if constexpr (sizeof...(Bs) == 5) return shape_go<Bs...>(A, cfg, out, s);
    else
        return want[sizeof...(Bs)] ? shape_pick<Bs..., true>(want, A, cfg, out, s)
                                   : shape_pick<Bs..., false>(want, A, cfg, out, s);
}

}  // namespace

bool shape_rows_vec16(const float* rows_ptr, long long row_pitch) {
    return (reinterpret_cast<uintptr_t>(rows_ptr) & 15) == 0 && (row_pitch & 3) == 0;
}

hipError_t launch_shape(const float* rows_ptr, long long rows, long long row_pitch, long long rows_per_group,
                        const ShapeCfg& cfg, const ShapeOut& out, bool dword, hipStream_t s) {
    const unsigned mask = out.mask();
    if (rows <= 0 || mask == 0) return hipSuccess;
    if (cfg.K < 2 || cfg.K > SHAPE_MAX_BINS || row_pitch < cfg.K || cfg.k_min < 0 || cfg.k_min > cfg.k_max ||
        cfg.k_max >= cfg.K || rows_per_group <= 0 || rows >= (1LL << 31))
        return hipErrorInvalidValue;
    const int T = ((cfg.K + 63) >> 6) | 1;
    const bool want[5] = {
        T <= SHAPE_REG_T,
        (mask & (1u << SHAPE_SPREAD | 1u << SHAPE_SKEW | 1u << SHAPE_KURT)) != 0,
        (mask & 1u << SHAPE_FLATNESS) != 0,
        (mask & 1u << SHAPE_ROLLOFF) != 0,
        (mask & 1u << SHAPE_FLUX) != 0,
    };
    ShapeArgs A;
    A.rows = rows_ptr;
    A.nrows = rows;
    A.pitch = row_pitch;
    A.rpg = rows_per_group < rows ? rows_per_group : rows;
    A.run_len = SHAPE_RUN;
    A.runs_per_group = (A.rpg + A.run_len - 1) / A.run_len;
    A.nruns = (rows + A.rpg - 1) / A.rpg * A.runs_per_group;
    A.wpb = 0;
    A.row_floats = (cfg.K + 3) & ~3;
    A.vec = !dword && shape_rows_vec16(rows_ptr, row_pitch);
    return shape_pick<>(want, A, cfg, out, s);
}

}  // namespace vvh
