// median_kernels.hip -- the running median of include/vv_dsp/filter/median.h in two
// access directions, and the masks of include/vv_dsp/spectral/hpss.h.
//
// Both kernels turn the values of a tile and of its 2h halo into keys in LDS once,
// with the boundary mode resolved while filling, so the select has no edge case;
// then every lane selects rank h of its own window:
//   k_med_rows  lanes across 256 positions of one line, the window along the line
//               (key j of lane l at keys[l + j]: consecutive banks);
//   k_med_cols  lanes across 64 bins, the window down the lines of a group: a
//               block takes MED_RUN lines of a 64-bin span, its four waves every
//               fourth line (key j at tile[(s + j) * 64 + lane]: bank = lane).
// The select is exact and branch-free, on the uint32 keys:
//   counting    the median is the largest candidate with fewer than h + 1 keys
//               below it (a key above the median has at least h + 1); four
//               candidates share one pass over the window, a compare and an
//               add-with-carry per pair: 2 L^2 lane-instructions per output;
//   bitwise     the median is the largest v with at most h keys below v, built
//               bit by bit from the top: 32 passes, 64 L lane-instructions.
// The second is cheaper from L = 33 on (MED_RADIX_FROM); both give the same bits.
// With masks, k_med_rows reads the other median where it has just selected its
// own, so only one of the two planes goes through memory.
#include "vvhip_internal.hpp"

#include <cstdint>

namespace vvh {

namespace {

constexpr uint32_t MED_QNAN = 0x7FC00000u;
constexpr uint32_t MED_KEY_ZERO = 0x80000000u;   // the key of +0.0f

__device__ inline uint32_t med_key(float v, int sqrt_w) {
    if (sqrt_w) v = sqrtf(v);
    const uint32_t b = v != v ? MED_QNAN : __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}

__device__ inline float med_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

// the index that stands for i on a line of n values, or -1: the value +0.0f
__device__ inline long long med_fold(long long i, long long n, int mode) {
    if (i >= 0 && i < n) return i;
    if (mode == MED_ZERO) return -1;
    if (mode == MED_NEAREST) return i < 0 ? 0 : n - 1;
    if (n == 1) return 0;
    const long long p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// rank L / 2 of the keys w[0], w[S], .. w[(L - 1) S]
template <int S>
__device__ inline uint32_t med_select_rank(const uint32_t* w, int L) {
    const int h = L >> 1;
    uint32_t best = 0;
    int i = 0;
    for (; i + 4 <= L; i += 4) {
        const uint32_t c0 = w[i * S], c1 = w[(i + 1) * S], c2 = w[(i + 2) * S], c3 = w[(i + 3) * S];
        int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
#pragma unroll 4
        for (int j = 0; j < L; ++j) {
            const uint32_t k = w[j * S];
            n0 += k < c0;
            n1 += k < c1;
            n2 += k < c2;
            n3 += k < c3;
        }
        best = max(best, n0 <= h ? c0 : 0u);
        best = max(best, n1 <= h ? c1 : 0u);
        best = max(best, n2 <= h ? c2 : 0u);
        best = max(best, n3 <= h ? c3 : 0u);
    }
    for (; i < L; ++i) {
        const uint32_t c = w[i * S];
        int n = 0;
        for (int j = 0; j < L; ++j) n += w[j * S] < c;
        best = max(best, n <= h ? c : 0u);
    }
    return best;
}

template <int S>
__device__ inline uint32_t med_select_radix(const uint32_t* w, int L) {
    const int h = L >> 1;
    uint32_t v = 0;
    for (int b = 31; b >= 0; --b) {
        const uint32_t t = v | (1u << b);
        int n = 0;
#pragma unroll 8
        for (int j = 0; j < L; ++j) n += w[j * S] < t;
        v = n <= h ? t : v;
    }
    return v;
}

template <int S, bool RADIX>
__device__ inline uint32_t med_select(const uint32_t* w, int L) {
    return RADIX ? med_select_radix<S>(w, L) : med_select_rank<S>(w, L);
}

// hpss.h's mask of (a, b) = (this median, margin x the other), every operation on its own
__device__ inline float hpss_mask(double a, double b, int kind) {
#pragma clang fp contract(off)
    if (kind == HPSS_HARD) return a > b ? 1.0f : 0.0f;
    if (kind == HPSS_WIENER) {
        a = a * a;
        b = b * b;
    }
    const double d = a + b;
    const float q = (float)(d == 0.0 ? 0.5 : a / d);
    return q != q ? __uint_as_float(MED_QNAN) : q;
}

template <bool RADIX, bool MASKS>
__global__ void __launch_bounds__(MED_TILE) k_med_rows(MedArgs a, unsigned tiles) {
#pragma clang fp contract(off)
    __shared__ uint32_t keys[MED_TILE + MED_MAX_WINDOW - 1];
    const long long line = blockIdx.x / tiles;
    const long long i0 = (long long)(blockIdx.x % tiles) * MED_TILE;
    const int h = a.L >> 1;
    const float* __restrict__ x = a.x + line * a.x_pitch;
    const long long left = a.n - i0;
    const int span = (int)(left < MED_TILE ? left : MED_TILE) + 2 * h;
    for (int s = threadIdx.x; s < span; s += MED_TILE) {
        const long long f = med_fold(i0 + s - h, a.n, a.mode);
        keys[s] = f < 0 ? MED_KEY_ZERO : med_key(x[f], a.sqrt_w);
    }
    __syncthreads();
    const long long i = i0 + threadIdx.x;
    if (i >= a.n) return;
    const float m = med_value(med_select<1, RADIX>(keys + threadIdx.x, a.L));
    const long long o = line * a.y_pitch + i;
    if (!MASKS || a.y) a.y[o] = m;
    if (MASKS) {
        const double H = (double)a.H[line * a.h_pitch + i], P = (double)m;
        if (a.mask_h) a.mask_h[o] = hpss_mask(H, a.margin_h * P, a.mask);
        if (a.mask_p) a.mask_p[o] = hpss_mask(P, a.margin_p * H, a.mask);
    }
}

template <bool RADIX>
__global__ void __launch_bounds__(256) k_med_cols(MedArgs a, unsigned spans, unsigned runs_per_group) {
    extern __shared__ uint32_t tile[];   // [run + 2h][64]
    const long long r = blockIdx.x / spans;
    const long long g = r / runs_per_group;
    const long long t0 = (r % runs_per_group) * MED_RUN;
    const long long rest = a.lines - g * a.rpg;
    const long long G = rest < a.rpg ? rest : a.rpg;   // the lines of this group
    if (t0 >= G) return;                                // a short last group (the whole block leaves)
    const int run = (int)(G - t0 < MED_RUN ? G - t0 : MED_RUN);
    const int h = a.L >> 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long k = (long long)(blockIdx.x % spans) * 64 + lane;
    const bool in = k < a.n;
    const float* __restrict__ x = a.x + g * a.rpg * a.x_pitch + k;
    for (int s = wave; s < run + 2 * h; s += 4) {
        const long long f = med_fold(t0 + s - h, G, a.mode);
        tile[s * 64 + lane] = !in ? 0u : f < 0 ? MED_KEY_ZERO : med_key(x[f * a.x_pitch], a.sqrt_w);
    }
    __syncthreads();
    if (!in) return;
    float* __restrict__ y = a.y + (g * a.rpg + t0) * a.y_pitch + k;
    for (int s = wave; s < run; s += 4)
        y[s * a.y_pitch] = med_value(med_select<64, RADIX>(tile + s * 64 + lane, a.L));
}

// lanes across the n_fft bins of one row; bin j >= K takes the mask of bin n_fft - j
__global__ void __launch_bounds__(256) k_hpss_apply(const float2* __restrict__ spec, const float* __restrict__ mask,
                                                    float2* __restrict__ out, long long n_fft, unsigned chunks) {
    const long long row = blockIdx.x / chunks;
    const long long j = (long long)(blockIdx.x % chunks) * 256 + threadIdx.x;
    if (j >= n_fft) return;
    const long long K = n_fft / 2 + 1;
    const float m = mask[row * K + (j < K ? j : n_fft - j)];
    const float2 v = spec[row * n_fft + j];
    out[row * n_fft + j] = make_float2(v.x * m, v.y * m);
}

}  // namespace

bool med_rows_supported(long long lines, long long n) {
    const long long tiles = (n + MED_TILE - 1) / MED_TILE;
    return lines < (1ll << 31) && tiles < (1ll << 31) && lines * tiles < (1ll << 31);
}

bool med_cols_supported(long long lines, long long n, long long rpg) {
    const long long lim = 1ll << 31;
    if (lines >= lim || rpg >= lim || rpg < 1) return false;
    const long long groups = (lines + rpg - 1) / rpg, runs = (rpg + MED_RUN - 1) / MED_RUN, spans = (n + 63) / 64;
    return spans < lim && groups * runs < lim && groups * runs * spans < lim;
}

hipError_t launch_med_rows(const MedArgs& a, hipStream_t s) {
    const unsigned tiles = (unsigned)((a.n + MED_TILE - 1) / MED_TILE);
    const dim3 grid((unsigned)(a.lines * tiles)), block(MED_TILE);
    const bool masks = a.mask_h || a.mask_p;
    if (a.radix) {
        if (masks) hipLaunchKernelGGL((k_med_rows<true, true>), grid, block, 0, s, a, tiles);
        else hipLaunchKernelGGL((k_med_rows<true, false>), grid, block, 0, s, a, tiles);
    } else {
        if (masks) hipLaunchKernelGGL((k_med_rows<false, true>), grid, block, 0, s, a, tiles);
        else hipLaunchKernelGGL((k_med_rows<false, false>), grid, block, 0, s, a, tiles);
    }
    return hipGetLastError();
}

hipError_t launch_med_cols(const MedArgs& a, hipStream_t s) {
    const long long groups = (a.lines + a.rpg - 1) / a.rpg;
    const unsigned runs = (unsigned)((a.rpg + MED_RUN - 1) / MED_RUN), spans = (unsigned)((a.n + 63) / 64);
    const long long longest = a.rpg < MED_RUN ? a.rpg : MED_RUN;
    const size_t lds = sizeof(uint32_t) * 64 * (size_t)(longest + (a.L - 1));
    const dim3 grid((unsigned)(groups * runs * spans)), block(256);
    if (a.radix) hipLaunchKernelGGL(k_med_cols<true>, grid, block, lds, s, a, spans, runs);
    else hipLaunchKernelGGL(k_med_cols<false>, grid, block, lds, s, a, spans, runs);
    return hipGetLastError();
}

hipError_t launch_hpss_apply(const float2* spec, const float* mask, float2* out, long long rows, long long n_fft,
                             hipStream_t s) {
    const unsigned chunks = (unsigned)((n_fft + 255) / 256);
    hipLaunchKernelGGL(k_hpss_apply, dim3((unsigned)(rows * chunks)), dim3(256), 0, s, spec, mask, out, n_fft, chunks);
    return hipGetLastError();
}

}  // namespace vvh
