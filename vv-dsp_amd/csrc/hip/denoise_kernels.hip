// denoise_kernels.hip -- the minimum-statistics noise floor and gain of
// include/vv_dsp/spectral/denoise.h in one launch.
//
// A block of eight waves takes (group, bin tile, time segment): lanes are
// consecutive bins, so every row access of a wave is one coalesced span, and the
// walk goes down the rows of the group.  For a segment of L rows from t0 and a
// window of B = back + ahead + 1 rows the block needs the smoothed values of rows
// t0 - back .. t0 + L - 1 + ahead: a halo of L + B - 1 rows, kept in LDS as keys
// (the uint32 order of median.h; a row outside the group is the key above every
// value, so every window has exactly B rows and no edge case).
//   1. smooth   each wave takes a run of halo rows, four rows at a time: the W + 3
//               powers they share are loaded once, twelve loads in flight, and
//               added oldest first into four f64 sums, the W adds of each in the
//               header's order (no sliding add/subtract).  `smooth` is stored
//               from here.
//   2. minima   blockwise: the minimum of every aligned sub-block of `sub` rows;
//   3. output   each wave takes every eighth row of the segment: the window's
//               minimum from the head and tail rows and the sub-block minima
//               between them (about sub + B / sub LDS reads instead of B), or from
//               all B rows (direct); then noise and gain, each operation on its own.
// A minimum is a selection, so the two ways give the same bits.  The tile is 64
// bins; where the halo of such a tile cannot fit LDS (a long window) it is 16
// bins, the other lanes idle.
#include "vvhip_internal.hpp"

#include <cstdint>

namespace vvh {

namespace {

constexpr uint32_t DN_QNAN = 0x7FC00000u;
constexpr uint32_t DN_KEY_NONE = 0xFFFFFFFFu;     // above the key of NaN (0xFFC00000): no row
constexpr int DN_WAVES = DN_THREADS / 64;
constexpr int DN_BATCH = 12;                      // powers loaded together: W + 3 at the default W = 8
constexpr size_t DN_LDS_SMALL = 64u << 10;        // dynamic LDS a launch gets without asking: two blocks per CU
constexpr size_t DN_LDS_LARGE = 152u << 10;       // one block per CU
constexpr long long DN_MIN_BLOCKS = 1024;         // shorter segments until a launch has this many blocks

// median.h's key of a float and back (as median_kernels.hip's med_key / med_value)
__device__ inline uint32_t dn_key(float v) {
    const uint32_t b = v != v ? DN_QNAN : __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}

__device__ inline float dn_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

__device__ inline float dn_canon(float v) { return v != v ? __uint_as_float(DN_QNAN) : v; }

// denoise.h's gain of power a against noise r
__device__ inline float dn_gain(double a, double r, double F, int mode) {
#pragma clang fp contract(off)
    double g;
    if (mode == DN_GATE) {
        g = a > r ? 1.0 : F;
    } else {
        const double d = a - r;
        double q = d / a;
        if (mode == DN_WIENER) {
            g = q > F ? q : F;
        } else {
            const double f2 = F * F;
            q = q > f2 ? q : f2;
            g = __dsqrt_rn(q);
        }
    }
    g = g > 1.0 ? 1.0 : g;
    return (float)g;
}

struct DnGeom {
    int L, nb, sub, halo;        // segment rows, bins per tile, sub-block rows, L + B - 1
    unsigned tiles, segs;
};

template <bool DIRECT>
__global__ void __launch_bounds__(DN_THREADS) k_denoise(DenoiseArgs a, DnGeom ge) {
#pragma clang fp contract(off)
    extern __shared__ uint32_t dn_lds[];          // keys [halo][nb], then sub-block minima [halo / sub][nb]
    const int nb = ge.nb;
    uint32_t* const keys = dn_lds;
    uint32_t* const mins = dn_lds + (size_t)ge.halo * nb;
    const long long r = blockIdx.x / ge.tiles;
    const long long g = r / ge.segs;
    const long long t0 = (r % ge.segs) * ge.L;
    const long long rest = a.rows - g * a.rpg;
    const long long G = rest < a.rpg ? rest : a.rpg;    // the rows of this group
    if (t0 >= G) return;                                 // a short last group (the whole block leaves)
    const int run = (int)(G - t0 < ge.L ? G - t0 : ge.L);
    const int B = a.back + a.ahead + 1, W = a.W;
    const int halo = run + B - 1;
    const long long u0 = t0 - a.back;                    // the row of halo index 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long k = (long long)(blockIdx.x % ge.tiles) * nb + lane;
    const bool in = lane < nb && k < a.K;
    const float* __restrict__ x = a.p + g * a.rpg * a.p_pitch + k;
    const long long obase = g * a.rpg * a.o_pitch + k;

    // 1. the halo: rows [h_lo, h_hi) of it are rows of the group
    const int h_lo = (int)(u0 < 0 ? -u0 : 0);
    const int h_hi = (int)(G - u0 < halo ? G - u0 : halo);
    if (in) {
        for (int h = wave; h < halo; h += DN_WAVES)
            if (h < h_lo || h >= h_hi) keys[h * nb + lane] = DN_KEY_NONE;
        const int per = ((h_hi - h_lo + DN_WAVES - 1) / DN_WAVES + 3) & ~3;
        const int c0 = h_lo + wave * per;
        const int c1 = c0 + per < h_hi ? c0 + per : h_hi;
        const double Wd = (double)W;
        for (int h = c0; h < c1; h += 4) {
            const int nr = c1 - h < 4 ? c1 - h : 4;
            const long long first = u0 + h - (W - 1);    // the oldest row of the first sum
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
            // the loads of a batch are issued together (a row past the newest one needed is that row again)
            const int n = W + nr - 1;
            const long long last = u0 + h + nr - 1;      // <= G - 1
            for (int j0 = 0; j0 < n; j0 += DN_BATCH) {
                float v[DN_BATCH];
#pragma unroll
                for (int q = 0; q < DN_BATCH; ++q) {
                    const long long ri = first + j0 + q;
                    v[q] = x[(ri < 0 ? 0 : ri > last ? last : ri) * a.p_pitch];
                }
#pragma unroll
                for (int q = 0; q < DN_BATCH; ++q) {
                    const int j = j0 + q;
                    const double d = (double)v[q];
                    if (j < W) acc0 += d;
                    if (j >= 1 && j < W + 1) acc1 += d;
                    if (j >= 2 && j < W + 2) acc2 += d;
                    if (j >= 3 && j < W + 3) acc3 += d;
                }
            }
            const double acc[4] = {acc0, acc1, acc2, acc3};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q >= nr) break;
                const float S = dn_canon((float)(acc[q] / Wd));
                keys[(h + q) * nb + lane] = dn_key(S);
                const long long t = u0 + h + q;
                if (a.smooth && t >= t0 && t < t0 + run) a.smooth[obase + t * a.o_pitch] = S;
            }
        }
    }
    __syncthreads();
    if (!(a.noise || a.gain)) return;

    // 2. the minimum of every whole sub-block
    const int sub = ge.sub;
    if (!DIRECT) {
        if (in) {
            for (int j = wave; j < halo / sub; j += DN_WAVES) {
                uint32_t m = DN_KEY_NONE;
                for (int i = 0; i < sub; ++i) m = min(m, keys[(j * sub + i) * nb + lane]);
                mins[j * nb + lane] = m;
            }
        }
        __syncthreads();
    }
    if (!in) return;

    // 3. row t0 + i: the window is halo rows [i, i + B)
    float next = wave < run ? x[(t0 + wave) * a.p_pitch] : 0.0f;       // the power of the row after this one, in flight
    for (int i = wave; i < run; i += DN_WAVES) {
        const long long t = t0 + i;
        const double pw = (double)next;
        if (i + DN_WAVES < run) next = x[(t + DN_WAVES) * a.p_pitch];
        uint32_t m = DN_KEY_NONE;
        const int lo = i, hi = i + B;
        const int jb0 = (lo + sub - 1) / sub, jb1 = hi / sub;    // whole sub-blocks [jb0, jb1)
        if (DIRECT || jb0 >= jb1) {
#pragma unroll 8
            for (int h = lo; h < hi; ++h) m = min(m, keys[h * nb + lane]);
        } else {
            for (int h = lo; h < jb0 * sub; ++h) m = min(m, keys[h * nb + lane]);
#pragma unroll 4
            for (int j = jb0; j < jb1; ++j) m = min(m, mins[j * nb + lane]);
            for (int h = jb1 * sub; h < hi; ++h) m = min(m, keys[h * nb + lane]);
        }
        const double rn = a.bias * (double)dn_value(m);
        const long long o = obase + t * a.o_pitch;
        if (a.noise) a.noise[o] = dn_canon((float)rn);
        if (a.gain) a.gain[o] = dn_gain(pw, rn, a.floor, a.mode);
    }
}

size_t dn_lds_bytes(int nb, int sub, long long halo) {
    return sizeof(uint32_t) * (size_t)nb * (size_t)(halo + halo / sub + 1);
}

// the longest segment whose halo fits `budget` bytes (may be < 1)
long long dn_longest(int nb, int sub, int B, size_t budget) {
    const long long cells = (long long)(budget / (sizeof(uint32_t) * nb)) - 1;
    return cells * sub / (sub + 1) - (B - 1);
}

}  // namespace

hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t s) {
    const int B = a.back + a.ahead + 1;
    DnGeom ge;
    ge.sub = B <= 128 ? 8 : B <= 512 ? 16 : 32;
    ge.nb = 64;
    long long L;
    if (a.seg > 0) {
        L = a.seg;
        if (dn_lds_bytes(64, ge.sub, L + B - 1) > DN_LDS_LARGE) ge.nb = 16;
        const long long most = dn_longest(16, ge.sub, B, DN_LDS_LARGE);
        if (L > most) L = most;
    } else {
        L = dn_longest(64, ge.sub, B, DN_LDS_SMALL);
        if (L < B) L = dn_longest(64, ge.sub, B, DN_LDS_LARGE);      // a halo of more than half the rows: one block per CU
        if (L < 16) {
            ge.nb = 16;
            L = dn_longest(16, ge.sub, B, DN_LDS_SMALL);
            if (L < 16) L = dn_longest(16, ge.sub, B, DN_LDS_LARGE);  // 1335 rows at the longest window
        }
    }
    if (L > a.rpg) L = a.rpg;
    const long long groups = (a.rows + a.rpg - 1) / a.rpg;
    ge.tiles = (unsigned)((a.K + ge.nb - 1) / ge.nb);
    if (a.seg <= 0)
        while (L >= 2 * (B > 32 ? B : 32) && groups * ge.tiles * ((a.rpg + L - 1) / L) < DN_MIN_BLOCKS) L = (L + 1) / 2;
    ge.L = (int)L;
    ge.halo = (int)(L + B - 1);
    ge.segs = (unsigned)((a.rpg + L - 1) / L);
    const size_t lds = dn_lds_bytes(ge.nb, ge.sub, ge.halo);
    auto kern = a.direct ? k_denoise<true> : k_denoise<false>;
    if (lds > DN_LDS_SMALL) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)DN_LDS_LARGE);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)(groups * ge.segs * ge.tiles)), block(DN_THREADS);
    hipLaunchKernelGGL(kern, grid, block, lds, s, a, ge);
    stat_inc(STAT_DENOISE);
    return hipGetLastError();
}

}  // namespace vvh
