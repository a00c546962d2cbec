// lsf_kernels.hip -- LPC rows <-> line spectral frequencies and reflection
// coefficients for gfx950, as include/vv_dsp/envelope/lsf.h defines them: every
// value an IEEE f64 operation in the header's order, nothing fused.
//
// k_lpc_to_lsf: one wave per row, four rows per workgroup.
//   Step-down: lane i holds c[i]; step m broadcasts k = c[m] and fetches c[m-i]
//   by one cross-lane read each, so the recursion is p dependent steps, not p^2/2.
//   Scan: lane 0 folds the row into the two Chebyshev series (2 x (p/2 + 1)
//   values, in LDS, read back as broadcasts).  The 257 grid points are spread over
//   the lanes, four points a lane plus the last; a ballot per 64 points gives the
//   sign classes and the brackets are bit arithmetic on the ballots.  Then one
//   lane per root: lanes 0..M1-1 bisect f1's brackets, lanes 32..32+M2-1 f2's,
//   32 Clenshaw evaluations each.  The interlace test is one cross-lane read.
// k_lsf_to_lpc: one wave per row, lane i holds entry i of F1 and F2; a factor
//   is two cross-lane reads (entries i-1, i-2) and three operations.  Lane k
//   evaluates the header's polynomial cosine of lsf[k] once.
// The grid is a table of the code object, built at compile time by the header's
// recurrence (constant evaluation is IEEE f64, one rounding per operation).
#include "vvhip_internal.hpp"
#include "wave_sync.hpp"
#include "../../../include/vv_dsp/envelope/lsf.h"

#pragma clang fp contract(off)

namespace vvh {

namespace {

constexpr int G = VV_DSP_LSF_GRID;
constexpr int HALF = LSF_MAX_ORDER / 2 + 2;   // entries of one Chebyshev series, rounded up

struct LsfGrid {
    double x[G + 1];
};
constexpr LsfGrid lsf_make_grid() {
    LsfGrid g{};
    g.x[0] = 1.0;
    g.x[1] = VV_DSP_LSF_CG;
    for (int i = 2; i < G; ++i) g.x[i] = (2.0 * VV_DSP_LSF_CG) * g.x[i - 1] - g.x[i - 2];
    g.x[G] = -1.0;
    return g;
}
__device__ const LsfGrid LSF_GRID = lsf_make_grid();

// the header's cosine: C[i] = (-1)^i / (2i+1)! by its recurrence, at compile time
struct LsfCosC {
    double c[VV_DSP_LSF_COS_TERMS];
};
constexpr LsfCosC lsf_make_cos() {
    LsfCosC t{};
    t.c[0] = 1.0;
    for (int i = 1; i < VV_DSP_LSF_COS_TERMS; ++i) t.c[i] = -t.c[i - 1] / (double)((2 * i) * (2 * i + 1));
    return t;
}
__device__ const LsfCosC LSF_COS = lsf_make_cos();

__device__ __forceinline__ double lsf_cos(double w) {
    const double t = (w - VV_DSP_LSF_PIO2_HI) - VV_DSP_LSF_PIO2_LO;
    const double s = t * t;
    double q = LSF_COS.c[VV_DSP_LSF_COS_TERMS - 1];
#pragma unroll
    for (int i = VV_DSP_LSF_COS_TERMS - 2; i >= 0; --i) q = q * s + LSF_COS.c[i];
    return -(t * q);
}

__device__ __forceinline__ float qnanf() { return __uint_as_float(0x7FC00000u); }

// Clenshaw of the series c[0..M] (LDS) at x
__device__ __forceinline__ double clenshaw(const double* c, int M, double x) {
    const double x2 = 2.0 * x;
    double b1 = 0.0, b2 = 0.0;
    for (int n = M; n >= 1; --n) {
        const double b = (x2 * b1 - b2) + c[n];
        b2 = b1;
        b1 = b;
    }
    return (x * b1 - b2) + c[0];
}

// the cell of the k-th bracket (k below the number of set bits of br)
__device__ __forceinline__ int kth_cell(const unsigned long long (&br)[4], int k) {
    int cell = 0;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        int before = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < j) before += __popcll(br[t]);
        if (k >= before && k < before + __popcll(br[j])) {
            unsigned long long w = br[j];
            for (int t = k - before; t > 0; --t) w &= w - 1;
            cell = 64 * j + (int)__builtin_ctzll(w);
        }
    }
    return cell;
}

// the brackets of one series over the grid: br = cells whose end points differ in
// sign class; returns their number
__device__ __forceinline__ int scan_series(const double* c, int M, int lane, unsigned long long (&br)[4]) {
    unsigned long long neg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) neg[j] = __ballot(clenshaw(c, M, LSF_GRID.x[64 * j + lane]) < 0.0);
    const unsigned long long last = clenshaw(c, M, LSF_GRID.x[G]) < 0.0 ? 1ull : 0ull;   // the same in every lane
    int count = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long next = j < 3 ? (neg[j < 3 ? j + 1 : 3] & 1ull) : last;
        br[j] = neg[j] ^ ((neg[j] >> 1) | (next << 63));
        count += __popcll(br[j]);
    }
    return count;
}

__global__ void __launch_bounds__(256)
k_lpc_to_lsf(const float* __restrict__ a, int p, long long rows, long long a_pitch, float* __restrict__ lsf,
             float* __restrict__ rc, int* __restrict__ flags) {
    __shared__ double sh[4][LSF_MAX_ORDER + 2 + 2 * HALF];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wv;
    if (row >= rows) return;   // the whole wave
    const float* ar = a + row * a_pitch;
    const double ai = (lane >= 1 && lane <= p) ? (double)ar[lane] : 0.0;

    bool stable = true;
    if (rc || flags) {
        double c = ai;
        float r = qnanf();
        for (int m = p; m >= 1; --m) {
            const double k = __shfl(c, m);
            const double cm = __shfl(c, (m - lane) & 63);
            if (lane == m - 1) r = k != k ? qnanf() : (float)k;
            if (!(fabs(k) < 1.0)) {
                stable = false;
                break;
            }
            const double den = 1.0 - k * k;
            if (lane >= 1 && lane < m) c = (c - k * cm) / den;
        }
        if (rc && lane < p) rc[row * p + lane] = r;
    }
    if (!lsf && !flags) return;

    double* ad = sh[wv];          // a as doubles, a[0] = 1, a[p+1] = 0
    double* c1 = ad + LSF_MAX_ORDER + 2;
    double* c2 = c1 + HALF;
    if (lane <= p + 1) ad[lane] = lane == 0 ? 1.0 : ai;   // ai is 0 at p + 1
    wave_sync();
    const int M1 = (p + 1) / 2, M2 = p / 2;
    if (lane == 0) {
        if ((p & 1) == 0) {
            double f1 = 0.0, f2 = 0.0;
            for (int k = 0; k <= M1; ++k) {
                const double P = ad[k] + ad[p + 1 - k], Q = ad[k] - ad[p + 1 - k];
                f1 = k ? P - f1 : P;
                f2 = k ? Q + f2 : Q;
                c1[M1 - k] = k == M1 ? f1 : 2.0 * f1;
                c2[M2 - k] = k == M2 ? f2 : 2.0 * f2;
            }
        } else {
            for (int k = 0; k <= M1; ++k) {
                const double f1 = ad[k] + ad[p + 1 - k];
                c1[M1 - k] = k == M1 ? f1 : 2.0 * f1;
            }
            double g1 = 0.0, g2 = 0.0;   // f2[k-1], f2[k-2]
            for (int k = 0; k <= M2; ++k) {
                const double Q = ad[k] - ad[p + 1 - k];
                const double f2 = k >= 2 ? Q + g2 : Q;
                g2 = g1;
                g1 = f2;
                c2[M2 - k] = k == M2 ? f2 : 2.0 * f2;
            }
        }
    }
    wave_sync();

    unsigned long long br1[4], br2[4];
    const int n1 = scan_series(c1, M1, lane, br1);
    const int n2 = scan_series(c2, M2, lane, br2);
    bool complete = n1 == M1 && n2 == M2;
    const int which = lane >> 5, k = lane & 31;
    const bool slot = k < (which ? M2 : M1);
    double root = 0.0;
    if (complete) {   // the whole wave
        if (slot) {
            const double* c = which ? c2 : c1;
            const int M = which ? M2 : M1;
            const int cell = which ? kth_cell(br2, k) : kth_cell(br1, k);
            double lo = LSF_GRID.x[cell], hi = LSF_GRID.x[cell + 1];
            const bool nlo = clenshaw(c, M, lo) < 0.0;
            for (int it = 0; it < VV_DSP_LSF_BISECTIONS; ++it) {
                const double mid = 0.5 * (lo + hi);
                if ((clenshaw(c, M, mid) < 0.0) == nlo) lo = mid;
                else hi = mid;
            }
            root = 0.5 * (lo + hi);
        }
        const double other = __shfl(root, which ? ((k + 1) & 31) : 32 + k);
        const bool check = which ? (k < M2 && k + 1 < M1) : k < M2;
        complete = __ballot(check && !(root > other)) == 0ull;
    }
    if (lsf && slot) lsf[row * p + 2 * k + which] = complete ? (float)acos(root) : qnanf();
    if (flags && lane == 0) flags[row] = (stable ? VV_DSP_LSF_STABLE : 0) | (complete ? VV_DSP_LSF_COMPLETE : 0);
}

__global__ void __launch_bounds__(256)
k_lsf_to_lpc(const float* __restrict__ lsf, int p, long long rows, float* __restrict__ a, long long a_pitch) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;   // the whole wave
    const double mine = lane < p ? lsf_cos((double)lsf[row * p + lane]) : 0.0;
    double F1 = lane == 0 ? 1.0 : 0.0, F2 = F1;
    for (int k = 0; k < p; ++k) {
        const double tc = 2.0 * __shfl(mine, k);
        const double F = (k & 1) ? F2 : F1;
        double o1 = __shfl_up(F, 1), o2 = __shfl_up(F, 2);
        if (lane < 1) o1 = 0.0;
        if (lane < 2) o2 = 0.0;
        const double nf = (F - tc * o1) + o2;
        if (k & 1) F2 = nf;
        else F1 = nf;
    }
    double p1 = __shfl_up(F1, 1), q1 = __shfl_up(F2, 1), q2 = __shfl_up(F2, 2);
    if (lane < 1) p1 = q1 = 0.0;
    if (lane < 2) q2 = 0.0;
    const double P = (p & 1) ? F1 : F1 + p1;
    const double Q = (p & 1) ? F2 - q2 : F2 - q1;
    const double h = 0.5 * (P + Q);
    if (lane <= p) a[row * a_pitch + lane] = lane == 0 ? 1.0f : h != h ? qnanf() : (float)h;
}

}  // namespace

hipError_t launch_lpc_to_lsf(const float* a, int order, long long rows, long long a_pitch, float* lsf, float* rc,
                             int* flags, hipStream_t s) {
    const unsigned grid = (unsigned)((rows + 3) / 4);
    hipLaunchKernelGGL(k_lpc_to_lsf, dim3(grid), dim3(256), 0, s, a, order, rows, a_pitch, lsf, rc, flags);
    return hipGetLastError();
}

hipError_t launch_lsf_to_lpc(const float* lsf, int order, long long rows, float* a, long long a_pitch, hipStream_t s) {
    const unsigned grid = (unsigned)((rows + 3) / 4);
    hipLaunchKernelGGL(k_lsf_to_lpc, dim3(grid), dim3(256), 0, s, lsf, order, rows, a, a_pitch);
    return hipGetLastError();
}

}  // namespace vvh
