// resample_kernels.hip -- fixed-ratio resampling of batched rows
// (reference src/resample/resampler.c:65-119, src/resample/interpolate.c:4-21).
//
//   k_resample_linear : the reference's linear path, bit-identical: the position
//       (float)((double)k / ratio), the end cases, floorf, and (1 - t) a + t b
//       with both products and the sum rounded separately (interp_rule.hpp).
//   k_resample_table  : the windowed-sinc path through a polyphase table.  The
//       ratio is rational, so the fractional position of output k is one of
//       P = num / gcd values and the reference's per-output sin / cos weights
//       collapse into P + 1 rows (csrc/host/resampler.c builds them).  The centre
//       is the reference's own (int)floor((double)k / ratio): where k den / num is
//       an integer that f64 quotient can land one ulp below it, and the reference
//       then centres one sample lower with a fraction of 1 - eps.  Table row P is
//       that filter at fraction 1; the kernel evaluates those few outputs (944 of
//       217,686 at 160/147) with the reference's own f64 loop instead, because
//       with 4 taps and cutoff 1 their value hangs on eps (see rs_exact's caller).
//       A workgroup takes a run of consecutive outputs of one row: the table and
//       the run's contiguous input span go to LDS once (clamped indices only in
//       the runs at a row's two ends), then lane = output.
//   k_resample_generic: any ratio; every output evaluates the reference's weights
//       itself in f64 and normalises by their sum (tables too large for LDS).
#include "vvhip_internal.hpp"
#include "interp_rule.hpp"

#include <algorithm>
#include <cmath>

namespace vvh {

namespace {

constexpr double kPiD = 3.141592653589793238462643383279502884;   // VV_DSP_PI_D
constexpr int RS_BLOCK = 256;
constexpr int RS_SPAN_MAX = 16384;   // floats of input one workgroup stages (64 KB)

// a workgroup takes RS_LIN_OPT x RS_BLOCK consecutive outputs of one row (one
// output per thread made 3.6 M workgroups of the 16 -> 48 kHz job: dispatch-bound)
constexpr int RS_LIN_OPT = 8;

__global__ void __launch_bounds__(RS_BLOCK)
k_resample_linear(const float* __restrict__ in, long long in_n, long long in_stride, float* __restrict__ out,
                  long long out_n, long long out_stride, double ratio, long long blocks_per_row) {
    const long long c = blockIdx.x / blocks_per_row;
    const long long k0 = (blockIdx.x % blocks_per_row) * (RS_BLOCK * RS_LIN_OPT) + threadIdx.x;
    const float* x = in + c * in_stride;
    float* yrow = out + c * out_stride;
    const float max_index = (float)(unsigned long long)(in_n - 1);
#pragma unroll
    for (int j = 0; j < RS_LIN_OPT; ++j) {
        const long long k = k0 + (long long)j * RS_BLOCK;
        if (k >= out_n) break;
        const float pos = (float)((double)k / ratio);
        float y;
        if (pos <= 0.0f) {
            y = x[0];
        } else if (pos >= max_index) {
            y = x[in_n - 1];
        } else {
            const long long i = (long long)floorf(pos);
            const float t = pos - (float)(unsigned long long)i;
            const float a = x[i];
            const float b = x[i + 1 < in_n ? i + 1 : in_n - 1];
            y = interp_linear_rule(t, a, b);
        }
        yrow[k] = y;
    }
}

__device__ inline float rs_sinc(double v) {   // resampler.c:54-58, rounded to f32 as there
    if (v == 0.0) return 1.0f;
    const double pix = kPiD * v;
    return (float)(sin(pix) / pix);
}

// one output by the reference's own loop (resampler.c:95-118): f64 weights from
// the exact in_pos, f64 sums, normalised by the weights' sum
__device__ inline float rs_exact(const float* __restrict__ x, long long in_n, long long k, double ratio,
                                 double cutoff, int taps) {
    const int half = taps / 2;
    const double in_pos = (double)k / ratio;
    const long long center = (long long)floor(in_pos);
    double acc = 0.0, wsum = 0.0;
    for (int m = 0; m < taps; ++m) {
        long long idx = center + m - half;
        const double t = (double)idx - in_pos;
        const double s = (double)rs_sinc(t * cutoff);
        const double w = 0.5 - 0.5 * cos((2.0 * kPiD * (double)m) / (double)(taps - 1));
        const double weight = s * w;
        idx = idx < 0 ? 0 : (idx >= in_n ? in_n - 1 : idx);
        acc += (double)x[idx] * weight;
        wsum += weight;
    }
    if (wsum != 0.0) acc /= wsum;
    return (float)acc;
}

// Dynamic LDS: Ws [phases][S] (S = resample_row_stride(taps): 16 B rows whose
// quarter stride is odd, so the 16 lanes of a ds_read_b128 group, on 16 rows that
// differ mod 16, read 16 distinct 4-bank blocks), then xs [span_cap].
// TAPS: the tap count when compiled in (full unroll), 0: `taps` (even, >= 4).
template <int TAPS>
__global__ void __launch_bounds__(RS_BLOCK)
k_resample_table(const float* __restrict__ in, long long in_n, long long in_stride, float* __restrict__ out,
                 long long out_n, long long out_stride, double ratio, double cutoff, int P, int taps,
                 const float* __restrict__ W, int run, long long runs_per_row, int span_cap) {
    extern __shared__ float4 rs_lds[];
    const int T = TAPS ? TAPS : taps;
    const int S = resample_row_stride(T);
    float* Ws = reinterpret_cast<float*>(rs_lds);
    float* xs = Ws + (size_t)(P + 1) * S;
    const long long c = blockIdx.x / runs_per_row;
    const long long k0 = (blockIdx.x % runs_per_row) * run;
    const int kn = (int)(out_n - k0 < run ? out_n - k0 : run);
    const int half = T / 2;
    const float* x = in + c * in_stride;

    const long long c_first = (long long)floor((double)k0 / ratio);
    const long long c_last = (long long)floor((double)(k0 + kn - 1) / ratio);
    const long long base = c_first - half;
    const int span = (int)(c_last - c_first) + T;
    if (span > span_cap) return;   // cannot happen: the launcher sizes span_cap for `run`

    {   // the table, already padded to S on the device: 16 B copies
        const float4* W4 = reinterpret_cast<const float4*>(W);
        const int n4 = (P + 1) * (S / 4);
        for (int i = threadIdx.x; i < n4; i += RS_BLOCK) rs_lds[i] = W4[i];
    }
    if (base >= 0 && base + span <= in_n) {   // interior run: no clamping
        const float* xb = x + base;
        for (int j = threadIdx.x; j < span; j += RS_BLOCK) xs[j] = xb[j];
    } else {
        for (int j = threadIdx.x; j < span; j += RS_BLOCK) {
            long long idx = base + j;
            idx = idx < 0 ? 0 : (idx >= in_n ? in_n - 1 : idx);
            xs[j] = x[idx];
        }
    }
    __syncthreads();

    float* y = out + c * out_stride + k0;
    for (int o = threadIdx.x; o < kn; o += RS_BLOCK) {
        const double in_pos = (double)(k0 + o) / ratio;
        const double cf = floor(in_pos);
        int row = (int)rint((in_pos - cf) * (double)P);   // 0 .. P
        row = row < 0 ? 0 : (row > P ? P : row);
        if (row == P) {
            // the quotient fell below an integer (fraction 1 - eps): the reference's own
            // evaluation.  With 4 taps and cutoff 1 the Hann window zeroes the one tap whose
            // sinc does not vanish there, and the result hangs on eps -- no table row holds that.
            y[o] = rs_exact(x, in_n, k0 + o, ratio, cutoff, T);
            continue;
        }
        const float* xw = xs + ((long long)cf - c_first);
        const float* w = Ws + (size_t)row * S;
        float acc = 0.0f;
        const int t4 = T & ~3;
#pragma unroll
        for (int m = 0; m < t4; m += 4) {
            const float4 wv = *reinterpret_cast<const float4*>(w + m);
            acc = fmaf(xw[m], wv.x, acc);
            acc = fmaf(xw[m + 1], wv.y, acc);
            acc = fmaf(xw[m + 2], wv.z, acc);
            acc = fmaf(xw[m + 3], wv.w, acc);
        }
        for (int m = t4; m < T; ++m) acc = fmaf(xw[m], w[m], acc);
        y[o] = acc;
    }
}

__global__ void __launch_bounds__(RS_BLOCK)
k_resample_generic(const float* __restrict__ in, long long in_n, long long in_stride, float* __restrict__ out,
                   long long out_n, long long out_stride, double ratio, double cutoff, int taps,
                   long long blocks_per_row) {
    const long long c = blockIdx.x / blocks_per_row;
    const long long k = (blockIdx.x % blocks_per_row) * RS_BLOCK + threadIdx.x;
    if (k >= out_n) return;
    out[c * out_stride + k] = rs_exact(in + c * in_stride, in_n, k, ratio, cutoff, taps);
}

// input floats a run of `run` outputs can span: its centres differ by at most
// ceil((run - 1) / ratio) + 1 (each f64 quotient is within an ulp of its value)
long long span_need(int run, int taps, double ratio) {
    return (long long)std::ceil((double)(run - 1) / ratio) + 2 + taps;
}

}  // namespace

int resample_run(long long phases, int taps, double ratio) {
    if (phases < 2 || taps < 4 || (taps & 1) || !(ratio > 0.0)) return 0;
    const size_t table = (size_t)phases * resample_row_stride(taps) * sizeof(float);
    if (table > RESAMPLE_TABLE_BYTES) return 0;
    long long cap = (long long)((RESAMPLE_LDS_BYTES - table) / sizeof(float));
    if (cap > RS_SPAN_MAX) cap = RS_SPAN_MAX;
    const double fit = std::floor((double)(cap - taps - 3) * ratio) + 1.0;   // span_need(fit) <= cap
    int run = fit > (double)RESAMPLE_RUN ? RESAMPLE_RUN : (int)fit;
    while (run > 1 && span_need(run, taps, ratio) > cap) --run;
    return run >= 64 ? run : 0;   // a strongly decimating ratio leaves too short a run: generic kernel
}

hipError_t launch_resample_linear(const float* in, long long in_n, long long nch, long long in_stride, float* out,
                                  long long out_n, long long out_stride, double ratio, hipStream_t s) {
    const long long per = (long long)RS_BLOCK * RS_LIN_OPT;
    const long long bpr = (out_n + per - 1) / per;
    if (bpr * nch > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resample_linear, dim3((unsigned)(bpr * nch)), dim3(RS_BLOCK), 0, s, in, in_n, in_stride, out,
                       out_n, out_stride, ratio, bpr);
    return hipGetLastError();
}

hipError_t launch_resample_table(const float* in, long long in_n, long long nch, long long in_stride, float* out,
                                 long long out_n, long long out_stride, double ratio, double cutoff, long long phases,
                                 int taps, const float* W, hipStream_t s) {
    const int run = resample_run(phases, taps, ratio);
    if (run == 0) return hipErrorInvalidValue;
    const long long rpr = (out_n + run - 1) / run;
    if (rpr * nch > 0x7fffffffLL) return hipErrorInvalidValue;
    const long long cap = span_need(run, taps, ratio);
    const size_t lds = ((size_t)phases * resample_row_stride(taps) + (size_t)cap) * sizeof(float);
    auto kern = taps == 32 ? k_resample_table<32> : k_resample_table<0>;
    if (lds > (48u << 10)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)RESAMPLE_LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(rpr * nch)), dim3(RS_BLOCK), lds, s, in, in_n, in_stride, out, out_n,
                       out_stride, ratio, cutoff, (int)(phases - 1), taps, W, run, rpr, (int)cap);
    return hipGetLastError();
}

hipError_t launch_resample_generic(const float* in, long long in_n, long long nch, long long in_stride, float* out,
                                   long long out_n, long long out_stride, double ratio, double cutoff, int taps,
                                   hipStream_t s) {
    const long long bpr = (out_n + RS_BLOCK - 1) / RS_BLOCK;
    if (bpr * nch > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resample_generic, dim3((unsigned)(bpr * nch)), dim3(RS_BLOCK), 0, s, in, in_n, in_stride, out,
                       out_n, out_stride, ratio, cutoff, taps, bpr);
    return hipGetLastError();
}

}  // namespace vvh
