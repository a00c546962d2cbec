// interp_kernels.hip -- batched linear and cubic interpolation at arbitrary
// fractional positions (reference src/resample/interpolate.c:4-64 per output).
//
//   k_interp<METHOD, UNIFORM, ROWS, G>: a workgroup takes a run of INTERP_RUN
//       consecutive outputs of one row (of ROWS rows that share their positions),
//       lane = output, IP_OPT outputs per thread a workgroup stride apart, so
//       neighbouring lanes read neighbouring positions and write neighbouring
//       outputs.  The two or four neighbours are read straight from global memory:
//       on a monotone curve they lie in the cache lines the wave is reading anyway,
//       on arbitrary positions the gather is element-granular and lives on L2 and
//       the Infinity Cache.  No LDS.
//       The position decides everything but the samples: the end clamps, floorf,
//       the fraction and the weights are computed once per output (interp_tap) and
//       applied to each of the ROWS rows (interp_value).  A thread takes its
//       outputs G at a time with no branch between their loads.
//   Values are the reference's bit for bit: pos <= 0 -> x[0], pos >= (float)(n - 1)
//   -> x[n - 1] (so -Inf / +Inf clamp), the cubic returns x[0] when n < 2 whatever
//   the position, neighbour indices clamped, every product and sum rounded
//   separately (interp_rule.hpp).  A NaN position, which the reference leaves
//   undefined, gives that NaN.
#include "vvhip_internal.hpp"
#include "interp_rule.hpp"

namespace vvh {

namespace {

constexpr int IP_BLOCK = 256;
constexpr int IP_OPT = INTERP_RUN / IP_BLOCK;   // outputs per thread

// What the position of one output decides, for every row it is applied to: which
// of the three cases the output is, the neighbour indices and the weights.  No
// branches: the indices are clamped into the row in every case, so each load is in
// bounds, the rule is evaluated on whatever they fetch, and the case selects the
// result -- the rule's value inside, the sample at i1 at an end clamp (never a
// weighted sum: 0 * Inf would not give the sample), the position itself for a NaN.
template <int METHOD>
struct Tap {
    bool inside, nan;
    unsigned i0, i1, i2, i3;   // i1 = floor(pos) inside (<= n - 2), 0 or n - 1 at a clamp; the others clamped around it
    float t;                   // linear: the fraction
    CubicBasis h;              // cubic: the basis at the fraction
};

template <int METHOD>
__device__ inline Tap<METHOD> interp_tap(float pos, int n, float max_index) {
    Tap<METHOD> tap;
    const bool by_pos = METHOD == INTERP_LINEAR || n >= 2;   // the cubic's n < 2 rule comes before the position
    const bool lo = pos <= 0.0f, hi = pos >= max_index, num = pos == pos;
    tap.nan = by_pos && !num;
    tap.inside = by_pos && num && !lo && !hi;
    const float p = tap.inside ? pos : 0.0f;   // 0 < p < (float)(n - 1): finite, floor(p) <= n - 2
    const int i = (int)floorf(p);              // n < 2^31: one conversion each way, exact
    const float t = p - (float)i;
    const int i1 = tap.inside ? i : (hi && !lo ? n - 1 : 0);
    tap.i1 = (unsigned)i1;
    tap.i0 = (unsigned)(i1 == 0 ? 0 : i1 - 1);
    tap.i2 = (unsigned)(i1 < n - 1 ? i1 + 1 : n - 1);   // compared this way round: no sum beyond n - 1 < 2^31
    tap.i3 = (unsigned)(i1 < n - 2 ? i1 + 2 : n - 1);
    if (METHOD == INTERP_CUBIC) tap.h = interp_cubic_basis(t);
    tap.t = t;
    return tap;
}

template <int METHOD>
__device__ inline float interp_value(const float* __restrict__ x, const Tap<METHOD>& tap, float pos) {
    const float p1 = x[tap.i1], p2 = x[tap.i2];
    const float y = METHOD == INTERP_LINEAR ? interp_linear_rule(tap.t, p1, p2)
                                            : interp_cubic_rule(tap.h, x[tap.i0], p1, p2, x[tap.i3]);
    return tap.inside ? y : (tap.nan ? pos : p1);
}

// (float)(start + (double)k * step): the empty asm keeps the f64 product out of a
// fused multiply-add with the sum (hipcc contracts __dmul_rn / __dadd_rn as well)
__device__ inline float uniform_position(double start, double step, long long k) {
    double p = (double)k * step;
    asm volatile("" : "+v"(p));
    return (float)(start + p);
}

// UNIFORM 0: positions read from pos (rows pos_stride floats apart, 0: shared);
// 1: position k = (float)(start + (double)k * step).  ROWS > 1 needs shared positions.
template <int METHOD, int UNIFORM, int ROWS, int G>
__global__ void __launch_bounds__(IP_BLOCK)
k_interp(const float* __restrict__ x, long long n, long long batch, long long x_stride,
         const float* __restrict__ pos, long long pos_stride, double start, double step, long long m,
         float* __restrict__ out, long long out_stride, unsigned blocks_per_row) {
    const long long r0 = (long long)(blockIdx.x / blocks_per_row) * ROWS;
    const long long k0 = (long long)(blockIdx.x % blocks_per_row) * INTERP_RUN + threadIdx.x;
    const float* prow = UNIFORM ? nullptr : pos + r0 * pos_stride;
    const int ni = (int)n;                      // n < 2^31
    const float max_index = (float)(ni - 1);   // rounded to nearest, as the reference's (float)(n - 1)
    // A thread's IP_OPT outputs go G at a time with no branch between their loads: G
    // positions, then G x 2 (or 4) samples per row, are in flight together.  An
    // output past the row's end computes the row's last output again and stores nothing.
#pragma unroll
    for (int j0 = 0; j0 < IP_OPT; j0 += G) {
        if (k0 + (long long)j0 * IP_BLOCK >= m) break;
        float p[G];
        Tap<METHOD> tap[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const long long k = k0 + (long long)(j0 + g) * IP_BLOCK;
            const long long kk = k < m ? k : m - 1;
            p[g] = UNIFORM ? uniform_position(start, step, kk) : prow[kk];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) tap[g] = interp_tap<METHOD>(p[g], ni, max_index);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const long long row = r0 + r;
            if (ROWS > 1 && row >= batch) break;
            const float* xr = x + row * x_stride;
            float* yr = out + row * out_stride;
            float y[G];
#pragma unroll
            for (int g = 0; g < G; ++g) y[g] = interp_value<METHOD>(xr, tap[g], p[g]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const long long k = k0 + (long long)(j0 + g) * IP_BLOCK;
                if (k < m) yr[k] = y[g];
            }
        }
    }
}

template <int METHOD, int UNIFORM, int ROWS, int G>
hipError_t launch_one(const InterpArgs& a, hipStream_t s) {
    const long long bpr = (a.m + INTERP_RUN - 1) / INTERP_RUN;
    const long long groups = (a.batch + ROWS - 1) / ROWS;
    if (bpr * groups > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_interp<METHOD, UNIFORM, ROWS, G>), dim3((unsigned)(bpr * groups)), dim3(IP_BLOCK), 0, s, a.x, a.n,
                       a.batch, a.x_stride, a.pos, a.pos_stride, a.start, a.step, a.m, a.out, a.out_stride, (unsigned)bpr);
    return hipGetLastError();
}

// G by measurement on 32 rows x 9.6 M samples: read positions
// want loads in flight -- 4 outputs at a time, 2 for the cubic over 8 rows, whose
// weights and indices otherwise push the registers below 4 waves per SIMD; computed
// positions are instruction-bound and gain nothing from it.
constexpr int interp_group(int method, int uniform, int rows) {
    return uniform ? 1 : (method == INTERP_CUBIC && rows > 1 ? 2 : 4);
}

template <int METHOD>
hipError_t launch_method(const InterpArgs& a, int rows, hipStream_t s) {
    if (!a.pos) return rows == 1 ? launch_one<METHOD, 1, 1, interp_group(METHOD, 1, 1)>(a, s) : hipErrorInvalidValue;
    if (rows == 1) return launch_one<METHOD, 0, 1, interp_group(METHOD, 0, 1)>(a, s);
    if (rows == INTERP_SHARED_ROWS && a.pos_stride == 0)
        return launch_one<METHOD, 0, INTERP_SHARED_ROWS, interp_group(METHOD, 0, INTERP_SHARED_ROWS)>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_interp(const InterpArgs& a, int method, int rows, hipStream_t s) {
    if (a.n < 1 || a.n >= (1LL << 31) || a.m < 1 || a.batch < 1) return hipErrorInvalidValue;
    if (method == INTERP_LINEAR) return launch_method<INTERP_LINEAR>(a, rows, s);
    if (method == INTERP_CUBIC) return launch_method<INTERP_CUBIC>(a, rows, s);
    return hipErrorInvalidValue;
}

}  // namespace vvh
