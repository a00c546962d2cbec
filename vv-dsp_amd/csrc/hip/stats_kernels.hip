// stats_kernels.hip -- array statistics and signal measurements for gfx950:
// sum, mean, var, min, max, argmin, argmax (src/core/core.c:42-108), rms, peak,
// crest factor, zero crossings, skewness, kurtosis and the lagged correlations
// (src/core/stats.c:10-139), over rows or over the frames of a signal.
//
// One order.  A row is cut into chunks of STATS_CHUNK samples.  One wave takes
// a chunk: lane l walks samples l, l + 64, ... of the chunk with its own
// accumulators, the 64 lanes combine by an xor butterfly (32, 16, .. 1), and
// the chunks' results are combined one after the other in chunk order.  The
// wave kernel walks all chunks of a row itself; the long route gives every
// (row, chunk) a wave of its own, leaves the chunks' results in scratch and
// combines them per row with the same function in the same order.  So a value
// depends on the row's samples and its length alone -- not on the route, the
// batch, the stride, the requested outputs or the entry point.
//
// Exact class (min, max, argmin, argmax, zero crossings).  The running
// extreme is a (value, index) pair seeded with (x[0], 0) in every lane and
// every chunk; a sample replaces it when strictly smaller (larger), two pairs
// combine to the smaller value or, at equal values, the lower index.  A NaN
// sample compares false and never enters; a NaN x[0] makes every comparison
// false and stays.  That is the reference's sequential loop, bits included
// (+0 and -0 are equal: the earlier one is returned).  Crossings are counted
// on adjacent samples: lane l takes its left neighbour from lane l - 1 by a
// shuffle, lane 0 from the previous step's lane 63 (or, at a chunk's start,
// from the sample before the chunk), so every pair is counted once.
//
// f64 class.  sum and the sum of squares accumulate in f64 (pass 1).  var,
// skewness and kurtosis are moments about mean = sum / n in f64, accumulated in
// a second pass over the row (which the first left in cache): the two-pass form
// is as accurate as the reference's running update and, unlike it, splits into
// independent partial sums.  A constant row has an exact f64 sum (n x[0] for
// n < 2^29), so its deviations and its variance are exactly 0.  Everything is
// rounded to float once, at the end, as in the reference.
//
// The kernels are specialised on what is wanted: MOM = false (rms, min, max,
// crest, crossings, arg*) carries no f64 sum and runs no second pass.
//
// Correlations: one workgroup per (row, lag); thread t adds the f64 products of
// samples t, t + 256, ..., a butterfly per wave, the four waves in order.
#include "frame_src.hpp"

#include <cmath>

namespace vvh {

namespace {

struct Ext {          // a running extreme
    float v;
    unsigned i;
};

struct StatsPart {    // pass 1 over a chunk (or, combined, over a row)
    double s1, s2;
    Ext mn, mx;
    unsigned zc, pad;
};

struct StatsMom {     // pass 2: sums of (x - mean)^2, ^3, ^4
    double m2, m3, m4;
};

struct StatsTotal {
    StatsPart p;
    StatsMom m;
};

using StatsRow = FrameRow<long long>;   // at: where the row's values go in every output plane

__device__ __forceinline__ StatsRow stats_row(const FrameSrc& s, long long out_ch_stride, long long row) {
    return frame_row(
        s, row, [&]() -> long long { return row; },
        [&](unsigned ch, unsigned f) -> long long { return ch * out_ch_stride + f; });
}

__device__ __forceinline__ Ext ext_min(Ext a, Ext b) {
    const bool take = b.v < a.v || (b.v == a.v && b.i < a.i);
    return {take ? b.v : a.v, take ? b.i : a.i};
}
__device__ __forceinline__ Ext ext_max(Ext a, Ext b) {
    const bool take = b.v > a.v || (b.v == a.v && b.i < a.i);
    return {take ? b.v : a.v, take ? b.i : a.i};
}
__device__ __forceinline__ Ext ext_xor(const Ext& a, int m) { return {__shfl_xor(a.v, m), __shfl_xor(a.i, m)}; }

__device__ __forceinline__ bool crossing(float a, float b) { return (a > 0 && b < 0) || (a < 0 && b > 0); }

// sample c0 + j of the row, j < 4096: a row inside the signal is read through the
// chunk's own pointers with a 32-bit offset
template <bool INSIDE>
__device__ __forceinline__ float chunk_sample(const FrameSrc& src, const StatsRow& rw, const float* xp,
                                              const float* wp, long long c0, int j) {
    if (!INSIDE) return frame_sample<false>(src, rw, c0 + j);
    float v = xp[j];
    if (wp) v = v * wp[j];
    return v;
}

// Pass 1 over samples [c0, c1) of a row by one wave; every lane returns the chunk's result.
template <bool MOM, bool INSIDE>
__device__ __forceinline__ StatsPart chunk_pass1(const FrameSrc& src, const StatsRow& rw, long long c0, long long c1,
                                                 float x0, int lane) {
#pragma clang fp contract(off)
    double s1 = 0.0, s2 = 0.0;
    Ext mn = {x0, 0u}, mx = {x0, 0u};
    unsigned zc = 0;
    const float* xp = rw.p + rw.start + c0;
    const float* wp = src.win ? src.win + c0 : nullptr;
    const int len = (int)(c1 - c0);
    const unsigned i0 = (unsigned)c0;
    // the sample left of the chunk (lane 0's first neighbour); no pair ends at sample 0
    float carry = c0 > 0 ? frame_sample<INSIDE>(src, rw, c0 - 1) : 0.0f;
    for (int j0 = 0; j0 < len; j0 += 64) {
        const int j = j0 + lane;
        const bool act = j < len;
        const float v = act ? chunk_sample<INSIDE>(src, rw, xp, wp, c0, j) : 0.0f;
        float left = __shfl_up(v, 1);
        if (lane == 0) left = carry;
        carry = __shfl(v, 63);
        if (act) {
            const unsigned i = i0 + (unsigned)j;
            const double d = (double)v;
            if (MOM) s1 += d;
            s2 = __builtin_fma(d, d, s2);
            if (v < mn.v) mn = {v, i};
            if (v > mx.v) mx = {v, i};
            if (i > 0 && crossing(left, v)) ++zc;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        if (MOM) s1 += __shfl_xor(s1, m);
        s2 += __shfl_xor(s2, m);
        mn = ext_min(mn, ext_xor(mn, m));
        mx = ext_max(mx, ext_xor(mx, m));
        zc += __shfl_xor(zc, m);
    }
    return {s1, s2, mn, mx, zc, 0u};
}

template <bool INSIDE>
__device__ __forceinline__ StatsMom chunk_pass2(const FrameSrc& src, const StatsRow& rw, long long c0, long long c1,
                                                double mean, int lane) {
#pragma clang fp contract(off)
    double m2 = 0.0, m3 = 0.0, m4 = 0.0;
    const float* xp = rw.p + rw.start + c0;
    const float* wp = src.win ? src.win + c0 : nullptr;
    const int len = (int)(c1 - c0);
    for (int j = lane; j < len; j += 64) {
        const double d = (double)chunk_sample<INSIDE>(src, rw, xp, wp, c0, j) - mean;
        const double d2 = d * d;
        m2 += d2;
        m3 = __builtin_fma(d2, d, m3);
        m4 = __builtin_fma(d2, d2, m4);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        m2 += __shfl_xor(m2, m);
        m3 += __shfl_xor(m3, m);
        m4 += __shfl_xor(m4, m);
    }
    return {m2, m3, m4};
}

// the chunks of a row, one after the other: tot starts from stats_zero(x0)
__device__ __forceinline__ StatsPart stats_zero(float x0) { return {0.0, 0.0, {x0, 0u}, {x0, 0u}, 0u, 0u}; }
__device__ __forceinline__ void stats_add(StatsPart& t, const StatsPart& p) {
#pragma clang fp contract(off)
    t.s1 += p.s1;
    t.s2 += p.s2;
    t.mn = ext_min(t.mn, p.mn);
    t.mx = ext_max(t.mx, p.mx);
    t.zc += p.zc;
}
__device__ __forceinline__ void stats_add(StatsMom& t, const StatsMom& p) {
#pragma clang fp contract(off)
    t.m2 += p.m2;
    t.m3 += p.m3;
    t.m4 += p.m4;
}

__device__ __forceinline__ double stats_mean(const StatsPart& t, long long n) { return t.s1 / (double)n; }

// the row's values from its sums, each formed as the reference forms it
__device__ __forceinline__ void stats_store(const StatsPart& t, const StatsMom& m, long long n, const StatsOut& out,
                                            long long at) {
#pragma clang fp contract(off)
    auto fo = [&](int k) { return static_cast<float*>(out.p[k]) + at; };
    auto uo = [&](int k) { return static_cast<unsigned*>(out.p[k]) + at; };
    const double dn = (double)n;
    const float sum = (float)t.s1;
    const float rms = (float)sqrt(t.s2 / dn);
    if (out.p[STATS_SUM]) *fo(STATS_SUM) = sum;
    if (out.p[STATS_MEAN]) *fo(STATS_MEAN) = sum / (float)n;
    if (out.p[STATS_RMS]) *fo(STATS_RMS) = rms;
    if (out.p[STATS_MIN]) *fo(STATS_MIN) = t.mn.v;
    if (out.p[STATS_MAX]) *fo(STATS_MAX) = t.mx.v;
    if (out.p[STATS_CREST]) {
        const float peak = (t.mx.v > -t.mn.v) ? t.mx.v : -t.mn.v;
        *fo(STATS_CREST) = rms == 0.0f ? INFINITY : peak / rms;
    }
    if (out.p[STATS_ZC]) *uo(STATS_ZC) = t.zc;
    if (out.p[STATS_ARGMIN]) *uo(STATS_ARGMIN) = t.mn.i;
    if (out.p[STATS_ARGMAX]) *uo(STATS_ARGMAX) = t.mx.i;
    const double var = m.m2 / dn;
    if (out.p[STATS_VAR]) *fo(STATS_VAR) = (float)var;
    if (out.p[STATS_SKEW]) *fo(STATS_SKEW) = var <= 0.0 ? 0.0f : (float)((m.m3 / dn) / pow(var, 1.5));
    if (out.p[STATS_KURT]) *fo(STATS_KURT) = var <= 0.0 ? 0.0f : (float)((m.m4 / dn) / (var * var) - 3.0);
}

template <bool MOM, bool INSIDE>
__device__ __forceinline__ void stats_wave_row(const FrameSrc& src, const StatsRow& rw, bool central,
                                               const StatsOut& out, int lane) {
    const long long n = src.len;
    const float x0 = frame_sample<INSIDE>(src, rw, 0);
    StatsPart tot = stats_zero(x0);
    for (long long c0 = 0; c0 < n; c0 += STATS_CHUNK) {
        const long long c1 = c0 + STATS_CHUNK < n ? c0 + STATS_CHUNK : n;
        stats_add(tot, chunk_pass1<MOM, INSIDE>(src, rw, c0, c1, x0, lane));
    }
    StatsMom mom = {0.0, 0.0, 0.0};
    if (MOM && central) {
        const double mean = stats_mean(tot, n);
        for (long long c0 = 0; c0 < n; c0 += STATS_CHUNK) {
            const long long c1 = c0 + STATS_CHUNK < n ? c0 + STATS_CHUNK : n;
            stats_add(mom, chunk_pass2<INSIDE>(src, rw, c0, c1, mean, lane));
        }
    }
    if (lane == 0) stats_store(tot, mom, n, out, rw.at);
}

// one wave per row, four rows per workgroup
template <bool MOM>
__global__ void __launch_bounds__(256) k_stats_wave(FrameSrc src, int central, StatsOut out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= src.rows) return;
    const StatsRow rw = stats_row(src, out.ch_stride, row);
    if (rw.inside) stats_wave_row<MOM, true>(src, rw, central != 0, out, lane);
    else stats_wave_row<MOM, false>(src, rw, central != 0, out, lane);
}

// long route, pass 1: one wave per (row, chunk) -> parts[row * chunks + c]
template <bool MOM>
__global__ void __launch_bounds__(256) k_stats_part(FrameSrc src, long long chunks, StatsPart* __restrict__ parts) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + wave;
    if (item >= src.rows * chunks) return;
    const long long row = item / chunks, c0 = (item - row * chunks) * STATS_CHUNK;
    const long long c1 = c0 + STATS_CHUNK < src.len ? c0 + STATS_CHUNK : src.len;
    const StatsRow rw = stats_row(src, 0, row);
    StatsPart p;
    if (rw.inside) p = chunk_pass1<MOM, true>(src, rw, c0, c1, frame_sample<true>(src, rw, 0), lane);
    else p = chunk_pass1<MOM, false>(src, rw, c0, c1, frame_sample<false>(src, rw, 0), lane);
    if (lane == 0) parts[item] = p;
}

// one thread per row: the chunks' pass-1 results in chunk order -> totals[row].p;
// last != 0: nothing about the mean is wanted, the outputs are written here
__global__ void __launch_bounds__(64) k_stats_combine(FrameSrc src, long long chunks,
                                                      const StatsPart* __restrict__ parts,
                                                      StatsTotal* __restrict__ totals, int last, StatsOut out) {
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= src.rows) return;
    const StatsPart* pr = parts + row * chunks;
    // every chunk's pairs hold the seed (x[0], 0), so chunk 0's pairs are what the
    // seed becomes once chunk 0 is added: starting from them gives the wave kernel's result
    StatsPart tot = {0.0, 0.0, pr[0].mn, pr[0].mx, 0u, 0u};
    for (long long c = 0; c < chunks; ++c) {
        const StatsPart p = {pr[c].s1, pr[c].s2, pr[c].mn, pr[c].mx, pr[c].zc, 0u};
        stats_add(tot, p);
    }
    totals[row].p = tot;
    const StatsMom none = {0.0, 0.0, 0.0};
    if (last) stats_store(tot, none, src.len, out, stats_row(src, out.ch_stride, row).at);
}

// long route, pass 2: one wave per (row, chunk) -> moms[row * chunks + c]
__global__ void __launch_bounds__(256) k_stats_mom(FrameSrc src, long long chunks,
                                                   const StatsTotal* __restrict__ totals,
                                                   StatsMom* __restrict__ moms) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + wave;
    if (item >= src.rows * chunks) return;
    const long long row = item / chunks, c0 = (item - row * chunks) * STATS_CHUNK;
    const long long c1 = c0 + STATS_CHUNK < src.len ? c0 + STATS_CHUNK : src.len;
    const StatsRow rw = stats_row(src, 0, row);
    const double mean = stats_mean(totals[row].p, src.len);
    StatsMom m;
    if (rw.inside) m = chunk_pass2<true>(src, rw, c0, c1, mean, lane);
    else m = chunk_pass2<false>(src, rw, c0, c1, mean, lane);
    if (lane == 0) moms[item] = m;
}

__global__ void __launch_bounds__(64) k_stats_finish(FrameSrc src, long long chunks,
                                                     const StatsTotal* __restrict__ totals,
                                                     const StatsMom* __restrict__ moms, StatsOut out) {
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= src.rows) return;
    StatsMom mom = {0.0, 0.0, 0.0};
    for (long long c = 0; c < chunks; ++c) stats_add(mom, moms[row * chunks + c]);
    stats_store(totals[row].p, mom, src.len, out, stats_row(src, out.ch_stride, row).at);
}

// one workgroup per (row, lag)
__global__ void __launch_bounds__(256) k_xcorr(const float* __restrict__ x, long long nx, const float* __restrict__ y,
                                               long long ny, long long r_len, int biased, float* __restrict__ r) {
    __shared__ double red[4];
    const long long item = blockIdx.x;
    const long long row = item / r_len, lag = item - row * r_len;
    // samples i < nx with i + lag < ny
    long long count = lag < ny ? ny - lag : 0;
    if (count > nx) count = nx;
    const float* xr = x + row * nx;
    const float* yr = y + row * ny + lag;
    const int t = threadIdx.x;
    double acc = 0.0;
    for (long long i = t; i < count; i += 256) acc = __builtin_fma((double)xr[i], (double)yr[i], acc);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t != 0) return;
    const double sum = ((red[0] + red[1]) + red[2]) + red[3];
    r[item] = count == 0 ? 0.0f : (float)(sum / (double)(biased ? nx : count));
}

bool stats_src_ok(const FrameSrc& src) {
    return src.len > 0 && src.len < (1LL << 32) && src.rows < (1LL << 31) && src.frames > 0;
}

}  // namespace

size_t stats_part_bytes() { return sizeof(StatsPart) + sizeof(StatsMom); }
size_t stats_total_bytes() { return sizeof(StatsTotal); }

hipError_t launch_stats_wave(const FrameSrc& src, const StatsOut& out, hipStream_t s) {
    const unsigned mask = out.mask();
    if (src.rows <= 0 || mask == 0) return hipSuccess;
    if (!stats_src_ok(src)) return hipErrorInvalidValue;
    const long long blocks = (src.rows + 3) / 4;
    const int central = (mask & STATS_CENTRAL_MASK) != 0;
    auto kern = (mask & STATS_MOMENT_MASK) ? k_stats_wave<true> : k_stats_wave<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, src, central, out);
    return hipGetLastError();
}

hipError_t launch_stats_long(const FrameSrc& src, const StatsOut& out, void* parts, void* totals, hipStream_t s) {
    const unsigned mask = out.mask();
    if (src.rows <= 0 || mask == 0) return hipSuccess;
    if (!stats_src_ok(src)) return hipErrorInvalidValue;
    const long long chunks = (src.len + STATS_CHUNK - 1) / STATS_CHUNK;
    const long long items = src.rows * chunks;
    if (items >= (1LL << 32)) return hipErrorInvalidValue;
    const unsigned wblocks = (unsigned)((items + 3) / 4), rblocks = (unsigned)((src.rows + 63) / 64);
    const bool central = (mask & STATS_CENTRAL_MASK) != 0;
    StatsPart* pp = static_cast<StatsPart*>(parts);
    StatsMom* mp = reinterpret_cast<StatsMom*>(pp + items);
    StatsTotal* tp = static_cast<StatsTotal*>(totals);
    auto kern = (mask & STATS_MOMENT_MASK) ? k_stats_part<true> : k_stats_part<false>;
    hipLaunchKernelGGL(kern, dim3(wblocks), dim3(256), 0, s, src, chunks, pp);
    hipLaunchKernelGGL(k_stats_combine, dim3(rblocks), dim3(64), 0, s, src, chunks, pp, tp, central ? 0 : 1, out);
    if (central) {
        hipLaunchKernelGGL(k_stats_mom, dim3(wblocks), dim3(256), 0, s, src, chunks, tp, mp);
        hipLaunchKernelGGL(k_stats_finish, dim3(rblocks), dim3(64), 0, s, src, chunks, tp, mp, out);
    }
    return hipGetLastError();
}

hipError_t launch_xcorr(const float* x, long long nx, const float* y, long long ny, long long rows, long long r_len,
                        int biased, float* r, hipStream_t s) {
    if (rows <= 0 || r_len <= 0) return hipSuccess;
    if (nx <= 0 || ny <= 0 || rows * r_len >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_xcorr, dim3((unsigned)(rows * r_len)), dim3(256), 0, s, x, nx, y, ny, r_len, biased, r);
    return hipGetLastError();
}

}  // namespace vvh
