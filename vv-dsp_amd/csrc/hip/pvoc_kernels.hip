// pvoc_kernels.hip -- the phase vocoder of include/vv_dsp/spectral/phase_vocoder.h:
// output row j of a channel is the analysis rows floor(p_j) and floor(p_j) + 1
// blended in magnitude, at the phase of row 0 plus the sum of the rows' phase
// steps so far.  Every value is f64 (atan2, sqrt, sincos) rounded to float once.
//
// Lanes run across (channel, bin) pairs, bin fastest, so a wave reads 64
// consecutive bins of one analysis row and writes 64 consecutive bins (and their
// 64 mirror bins) of one output row.  Time is cut into segments of PVOC_SEGMENT
// output rows, one wave per (segment, 64 pairs):
//   k_pvoc_rows<false>  walks a segment and stores the sum of its phase steps
//                       (every segment but the last, whose total nothing reads);
//   k_pvoc_scan         one lane per pair: the totals become the segments' bases
//                       in ascending order, and the phase of row 0 is stored;
//   k_pvoc_rows<true>   walks the segment again from its base and writes the rows.
// Knob PVOC_PLANE = 1 (for timing the alternative; the same bits): k_pvoc_theta
// first stores every analysis bin's phase in an f64 plane, and the walks read it
// instead of calling atan2 (the first walk then reads no input row at all).
// A walk keeps the last two analysis rows it used (index, phase, magnitude) in
// registers: positions that advance by less than a row reuse them, so a walk
// takes one atan2 per analysis row it touches, not two per output row.  The
// positions are the same for every lane, so the reuse tests are uniform.
#include "vvhip_internal.hpp"

#include <cmath>

namespace vvh {

namespace {

constexpr int PV_BLOCK = 64;

// p_j of the header, clamped into [0, T], a NaN to 0.  The empty asm keeps the
// product out of a fused multiply-add with the sum.
__device__ inline double pvoc_position(const PvocArgs& a, long long j) {
    double p;
    if (a.pos) {
        p = (double)a.pos[j];
    } else {
        double q = (double)j * a.step;
        asm volatile("" : "+v"(q));
        p = a.start + q;
    }
    if (!(p >= 0.0)) p = 0.0;
    if (p > (double)a.T) p = (double)a.T;
    return p;
}

struct PvRow {
    long long t;
    double th, mag;
};

// phase and magnitude of bin `in[t * n_fft]`; a row t >= T is zero.  PLANE: the
// phase is read from th[t * K], where k_pvoc_theta stored this function's value.
template <bool MAG, bool PLANE>
__device__ inline PvRow pvoc_row(const float2* __restrict__ in, const double* __restrict__ th, long long t,
                                 const PvocArgs& a) {
#pragma clang fp contract(off)
    PvRow r;
    r.t = t;
    r.th = 0.0;
    r.mag = 0.0;
    if (t >= a.T) return r;
    if (PLANE) r.th = th[t * (a.n_fft / 2 + 1)];
    if (MAG || !PLANE) {
        const float2 v = in[t * a.n_fft];
        const double re = (double)v.x, im = (double)v.y;
        if (MAG) r.mag = sqrt(re * re + im * im);
        if (!PLANE && !(v.x == 0.0f && v.y == 0.0f)) r.th = atan2(im, re);
        // a non-finite bin is NaN in phase and in magnitude (atan2 of an infinity is
        // finite, and an infinite magnitude would give infinities, not NaN)
        if (!(fabsf(v.x) < INFINITY && fabsf(v.y) < INFINITY)) {
            if (!PLANE) r.th = (double)NAN;
            if (MAG) r.mag = (double)NAN;
        }
    }
    return r;
}

// the lane's (channel, bin) pair; false past the last pair
__device__ inline bool pvoc_pair(const PvocArgs& a, unsigned block, long long* ch, int* k) {
    const int K = (int)(a.n_fft / 2 + 1);
    const long long g = (long long)block * PV_BLOCK + threadIdx.x;
    if (g >= a.nch * K) return false;
    *ch = g / K;
    *k = (int)(g - *ch * K);
    return true;
}

template <bool OUT, bool PLANE>
__global__ void __launch_bounds__(PV_BLOCK) k_pvoc_rows(PvocArgs a, unsigned pair_blocks) {
#pragma clang fp contract(off)
    const long long seg = blockIdx.x / pair_blocks;
    long long ch;
    int k;
    if (!pvoc_pair(a, blockIdx.x % pair_blocks, &ch, &k)) return;
    const int K = (int)(a.n_fft / 2 + 1);
    const long long nseg = pvoc_segments(a.m);
    const float2* __restrict__ in = a.in + ch * a.in_ch_stride + k;
    const double* __restrict__ th = PLANE ? a.plane + ch * a.T * K + k : nullptr;
    double* __restrict__ w = a.work + ch * (nseg + 1) * K;
    const long long j0 = seg * PVOC_SEGMENT;
    const long long j1 = j0 + PVOC_SEGMENT < a.m ? j0 + PVOC_SEGMENT : a.m;

    double base = 0.0, th_first = 0.0;
    if (OUT) {
        base = w[seg * K + k];
        th_first = w[nseg * K + k];
    }
    const bool mirror = k > 0 && 2 * (long long)k < a.n_fft;
    float2* __restrict__ out = a.out + ch * a.out_ch_stride;

    PvRow c0{-1, 0.0, 0.0}, c1{-1, 0.0, 0.0};
    double part = 0.0;
    for (long long j = j0; j < j1; ++j) {
        const double p = pvoc_position(a, j);
        const double fl = floor(p);
        const long long t0 = (long long)fl;
        PvRow r0, r1;
        if (t0 == c0.t) r0 = c0;
        else if (t0 == c1.t) r0 = c1;
        else r0 = pvoc_row<OUT, PLANE>(in, th, t0, a);
        if (t0 + 1 == c1.t) r1 = c1;
        else if (t0 + 1 == c0.t) r1 = c0;
        else r1 = pvoc_row<OUT, PLANE>(in, th, t0 + 1, a);
        c0 = r0;
        c1 = r1;
        if (OUT) {
            const double al = p - fl;
            const double mj = (1.0 - al) * r0.mag + al * r1.mag;
            const double phi = th_first + (base + part);
            double sn, cs;
            sincos(phi, &sn, &cs);
            float2 v;
            v.x = (float)(mj * cs);
            v.y = (float)(mj * sn);
            if (mj == 0.0 && phi == phi) v.x = v.y = 0.0f;
            float2* row = out + j * a.n_fft;
            row[k] = v;
            if (mirror) {
                v.y = -v.y;
                row[a.n_fft - k] = v;
            }
        }
        part += r1.th - r0.th;
    }
    if (!OUT) w[seg * K + k] = part;
}

// One lane per pair: totals -> bases (an exclusive scan in ascending order from
// 0.0; the last segment's total is never formed), then the phase of row 0.
__global__ void __launch_bounds__(PV_BLOCK) k_pvoc_scan(PvocArgs a) {
#pragma clang fp contract(off)
    long long ch;
    int k;
    if (!pvoc_pair(a, blockIdx.x, &ch, &k)) return;
    const int K = (int)(a.n_fft / 2 + 1);
    const long long nseg = pvoc_segments(a.m);
    double* __restrict__ w = a.work + ch * (nseg + 1) * K + k;
    double base = 0.0;
    long long s = 0;
    constexpr int U = 8;   // the loads of a run are independent of the sums
    for (; s + U < nseg; s += U) {
        double t[U];
#pragma unroll
        for (int i = 0; i < U; ++i) t[i] = w[(s + i) * K];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            w[(s + i) * K] = base;
            base += t[i];
        }
    }
    for (; s < nseg; ++s) {
        const double t = s + 1 < nseg ? w[s * K] : 0.0;
        w[s * K] = base;
        base += t;
    }
    const double p = pvoc_position(a, 0);
    w[nseg * K] = pvoc_row<false, false>(a.in + ch * a.in_ch_stride + k, nullptr, (long long)floor(p), a).th;
}

// The phase plane [nch][T][K] (knob PVOC_PLANE): one wave per (analysis row, 64 pairs).
__global__ void __launch_bounds__(PV_BLOCK) k_pvoc_theta(PvocArgs a, double* __restrict__ plane, unsigned pair_blocks) {
    const long long t = blockIdx.x / pair_blocks;
    long long ch;
    int k;
    if (!pvoc_pair(a, blockIdx.x % pair_blocks, &ch, &k)) return;
    const int K = (int)(a.n_fft / 2 + 1);
    plane[(ch * a.T + t) * K + k] = pvoc_row<false, false>(a.in + ch * a.in_ch_stride + k, nullptr, t, a).th;
}

__global__ void __launch_bounds__(256) k_pvoc_normalize(float* __restrict__ y, long long y_stride,
                                                        const float* __restrict__ norm, long long len) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    float* yc = y + (long long)blockIdx.y * y_stride;
    const float nv = norm[(long long)blockIdx.y * len + i];
    yc[i] = nv > PVOC_NORM_FLOOR ? yc[i] / nv : 0.0f;
}

}  // namespace

bool pvoc_supported(long long T, long long n_fft, long long nch, long long m) {
    const long long lim = 1ll << 31;
    if (n_fft > PVOC_MAX_FFT || T >= lim || m >= lim || nch >= lim) return false;
    const long long pairs = nch * (n_fft / 2 + 1);
    if (pairs >= lim) return false;
    const long long pair_blocks = (pairs + PV_BLOCK - 1) / PV_BLOCK;
    return pair_blocks * pvoc_segments(m) < lim;
}

bool pvoc_plane_supported(long long T, long long n_fft, long long nch) {
    const long long pair_blocks = (nch * (n_fft / 2 + 1) + PV_BLOCK - 1) / PV_BLOCK;
    return T > 0 && pair_blocks * T < (1ll << 31);
}

template <bool PLANE>
static hipError_t pvoc_launches(const PvocArgs& a, unsigned pair_blocks, hipStream_t s) {
    const long long nseg = pvoc_segments(a.m);
    if (PLANE)
        hipLaunchKernelGGL(k_pvoc_theta, dim3((unsigned)(pair_blocks * a.T)), dim3(PV_BLOCK), 0, s, a,
                           const_cast<double*>(a.plane), pair_blocks);
    if (nseg > 1)
        hipLaunchKernelGGL((k_pvoc_rows<false, PLANE>), dim3((unsigned)(pair_blocks * (nseg - 1))), dim3(PV_BLOCK), 0, s,
                           a, pair_blocks);
    hipLaunchKernelGGL(k_pvoc_scan, dim3(pair_blocks), dim3(PV_BLOCK), 0, s, a);
    hipLaunchKernelGGL((k_pvoc_rows<true, PLANE>), dim3((unsigned)(pair_blocks * nseg)), dim3(PV_BLOCK), 0, s, a,
                       pair_blocks);
    return hipGetLastError();
}

hipError_t launch_pvoc(const PvocArgs& a, hipStream_t s) {
    const long long pairs = a.nch * (a.n_fft / 2 + 1);
    const unsigned pair_blocks = (unsigned)((pairs + PV_BLOCK - 1) / PV_BLOCK);
    return a.plane ? pvoc_launches<true>(a, pair_blocks, s) : pvoc_launches<false>(a, pair_blocks, s);
}

hipError_t launch_pvoc_normalize(float* y, long long y_stride, const float* norm, long long len, long long nch,
                                 hipStream_t s) {
    for (long long c = 0; c < nch; c += 65535) {
        const unsigned g = (unsigned)(nch - c < 65535 ? nch - c : 65535);
        hipLaunchKernelGGL(k_pvoc_normalize, dim3((unsigned)((len + 255) / 256), g), dim3(256), 0, s,
                           y + c * y_stride, y_stride, norm + c * len, len);
    }
    return hipGetLastError();
}

}  // namespace vvh
