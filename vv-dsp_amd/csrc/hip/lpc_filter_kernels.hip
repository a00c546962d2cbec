// lpc_filter_kernels.hip -- LPC rows applied to a signal for gfx950, as
// include/vv_dsp/envelope/lpc_filter.h defines it: the time-varying inverse
// filter A(z) (residual) and the all-pole filter g / A(z) (synthesis), every
// pinned value an IEEE f64 operation in the header's order, nothing fused.
//
// k_lpc_residual: a workgroup takes a tile of LPCF_TILE samples of one channel.
//   The tile and its p samples of history sit in LDS as doubles (the history
//   before sample 0 comes from the state, which need not be a float), with the
//   first RES_ROWS coefficient rows the tile spans; a sample governed by a later
//   row (seg_len small) reads its row from global memory: correct, not fast.
//   k_lpc_residual_state then leaves the last p inputs in the state.
// k_lpc_synth_walk<P>: the recursion.  One lane owns one sub-row -- a whole row,
//   or one chunk of a row -- with the last P values of Y and the governing row's
//   coefficients in registers.  The history is a ring whose position is a
//   compile-time constant: a tile of 32 samples is unrolled and P divides 32.
//   Orders are dispatched in groups (P/2, P]; a padded term is computed and then
//   not selected, never added: 0 * inf is a NaN and -0 - (-0) is +0.  As in
//   iir_kernels.hip a wave stages tiles of 64 sub-rows x 32 samples through LDS so
//   that loads and stores touch whole 128 B lines.  A lane reloads its row when
//   its own sample counter reaches the row's end, so sub-rows that start at
//   different times (chunks) share a wave.
// Long rows: k_lpc_synth_phi<P> takes one wave per (row, chunk): lanes i < p walk
//   the unit states with zero input, lane p the zero state with the chunk's
//   excitation, in lockstep through the same rows of coefficients (uniform
//   loads), which gives the chunk's p x p transition and its zero-state end
//   values.  k_lpc_synth_scan<P> carries s_{c+1} = Phi_c s_c + z_c over a row's
//   chunks in f64, one wave per row, lane r component r, the next chunk's column
//   values in flight.  k_lpc_synth_walk then walks every chunk from s_c.  Only
//   that last walk is pinned to the header's operation order.
#include "vvhip_internal.hpp"

#pragma clang fp contract(off)

namespace vvh {

namespace {

constexpr int LANES = 64;
constexpr int WTILE = 32;            // samples of a sub-row per LDS tile: one 128 B line
constexpr int WROW = WTILE + 1;      // floats per tile row in LDS
constexpr int RES_THREADS = 256;
constexpr int RES_ROWS = 8;          // coefficient rows of a tile staged in LDS
constexpr long long NEVER = 0x7fffffffffffffffLL;

__device__ __forceinline__ float store_float(double v) { return v != v ? __uint_as_float(0x7FC00000u) : (float)v; }

// ---------------------------------------------------------------- residual
__global__ void __launch_bounds__(RES_THREADS) k_lpc_residual(const LpcFilt a, long long tiles) {
    __shared__ double xs[LPCF_TILE + LPCF_MAX_ORDER];
    __shared__ float cs[RES_ROWS][LPCF_MAX_ORDER + 1];   // [r][0]: the row's gain
    const int p = a.order;
    const long long row = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * LPCF_TILE;
    const int len = (int)(a.n - t0 < LPCF_TILE ? a.n - t0 : LPCF_TILE);
    const float* x = a.x + row * a.x_stride;
    const float* ar = a.a + row * a.a_ch_stride;
    const float* gr = a.gain ? a.gain + row * a.g_ch_stride : nullptr;
    for (int j = threadIdx.x; j < p + len; j += RES_THREADS) {
        const long long t = t0 - p + j;
        xs[j] = t >= 0 ? (double)x[t] : (a.state ? a.state[row * p + (-t - 1)] : 0.0);
    }
    // the row of the tile's first sample, and how far into it that sample is
    const long long u0 = t0 + a.offset;
    long long f0 = u0 < 0 ? 0 : u0 / a.seg_len;
    const long long rem0 = u0 < 0 ? u0 : u0 - f0 * a.seg_len;
    if (f0 > a.frames - 1) f0 = a.frames - 1;
    for (int j = threadIdx.x; j < RES_ROWS * (p + 1); j += RES_THREADS) {
        const int r = j / (p + 1), k = j % (p + 1);
        const long long f = f0 + r;
        if (f < a.frames) cs[r][k] = k ? ar[f * a.a_pitch + k] : (gr ? gr[f] : 1.0f);
    }
    __syncthreads();
    float* y = a.y + row * a.y_stride + t0;
    for (int i = threadIdx.x; i < len; i += RES_THREADS) {
        // rows past f0: r < seg_len + LPCF_TILE, so the quotient is 32-bit or at most 1
        const long long r = rem0 + i;
        long long f = f0;
        if (r >= a.seg_len) f += a.seg_len <= 0x7fffffffLL ? (long long)((unsigned)r / (unsigned)a.seg_len) : 1;
        if (f > a.frames - 1) f = a.frames - 1;
        const int d = (int)(f - f0);
        const double* xi = xs + p + i;
        double acc = xi[0];
        float g;
        if (d < RES_ROWS) {
            const float* c = cs[d];
            for (int k = 1; k <= p; ++k) acc = acc + (double)c[k] * xi[-k];
            g = c[0];
        } else {
            const float* c = ar + f * a.a_pitch;
            for (int k = 1; k <= p; ++k) acc = acc + (double)c[k] * xi[-k];
            g = gr ? gr[f] : 1.0f;
        }
        if (gr) acc = acc / (double)g;
        y[i] = store_float(acc);
    }
}

// the last p inputs as the state, newest first; entries older than the call shift
__global__ void __launch_bounds__(LANES) k_lpc_residual_state(const LpcFilt a) {
    const int p = a.order, k = threadIdx.x + 1;
    const long long row = blockIdx.x, t = a.n - k;
    double v = 0.0;
    if (k <= p) v = t >= 0 ? (double)a.x[row * a.x_stride + t] : a.state[row * p + (-t - 1)];
    __syncthreads();
    if (k <= p) a.state[row * p + k - 1] = v;
}

// ---------------------------------------------------------------- the recursion
// The row that governs sample t of a signal and the first sample of the next row.
struct RowPos {
    long long f, next;
};
__device__ __forceinline__ RowPos row_at(const LpcFilt& a, long long t) {
    const long long u = t + a.offset;
    const long long f = u < 0 ? 0 : u / a.seg_len;
    RowPos r;
    if (f >= a.frames - 1) {
        r.f = a.frames - 1;
        r.next = NEVER;
    } else {
        r.f = f;
        r.next = (f + 1) * a.seg_len - a.offset;
    }
    return r;
}

// c[k] = (double)a[f][k] for k <= p (0 beyond: never selected), c[0] = the gain
template <int P>
__device__ __forceinline__ void load_row(double (&c)[P + 1], const float* ar, const float* gr, long long f,
                                         long long a_pitch, int p) {
    const float* r = ar + f * a_pitch;
#pragma unroll
    for (int k = 1; k <= P; ++k) c[k] = (k <= P / 2 || k <= p) ? (double)r[k] : 0.0;
    c[0] = gr ? (double)gr[f] : 1.0;
}

// One sample at ring position J: acc = in - sum_k c[k] Y[t-k], k ascending, each
// product and each difference rounded; Y[t-k] is h[(J - k) mod P].
template <int P, int J>
__device__ __forceinline__ double synth_step(double (&h)[P], const double (&c)[P + 1], int p, double in) {
    double acc = in;
#pragma unroll
    for (int k = 1; k <= P; ++k) {
        const double t = acc - c[k] * h[(J - k + 2 * P) % P];
        acc = (k <= P / 2 || k <= p) ? t : acc;
    }
    h[J % P] = acc;
    return acc;
}

// h[P - k] = state[k - 1], the value at t = -k, k <= p; null: zeros
template <int P>
__device__ __forceinline__ void load_state(double (&h)[P], const double* st, int p) {
#pragma unroll
    for (int k = 1; k <= P; ++k) h[P - k] = (st && k <= p) ? st[k - 1] : 0.0;
}

// The ring of every lane goes to LDS ([slot][lane]), where a lane can read the
// slot of a sample by a run-time index: the value at t (sub-row time, t >= -p) is
// in slot t mod P.
template <int P>
__device__ __forceinline__ void dump_ring(double* sh, const double (&h)[P], int lane) {
#pragma unroll
    for (int k = 0; k < P; ++k) sh[k * LANES + lane] = h[k];
}
template <int P>
__device__ __forceinline__ double ring_at(const double* sh, int lane, int t) {
    return sh[(((t % P) + P) % P) * LANES + lane];
}

template <int P, int J>
struct TileWalk {
    // samples J .. WTILE - 1 of a tile for one lane: mine[j] in, out when WRITE
    template <bool WRITE>
    static __device__ __forceinline__ void run(double (&h)[P], double (&c)[P + 1], int p, const LpcFilt& a,
                                               const float* ar, const float* gr, RowPos& pos, long long t,
                                               int m, float* mine) {
        if (J < m) {
            if (t + J == pos.next) {
                ++pos.f;
                pos.next = pos.f >= a.frames - 1 ? NEVER : pos.next + a.seg_len;
                load_row<P>(c, ar, gr, pos.f, a.a_pitch, p);
            }
            const double v = synth_step<P, J>(h, c, p, c[0] * (double)mine[J]);
            if (WRITE) mine[J] = store_float(v);
        }
        TileWalk<P, J + 1>::template run<WRITE>(h, c, p, a, ar, gr, pos, t, m, mine);
    }
};
template <int P>
struct TileWalk<P, WTILE> {
    template <bool WRITE>
    static __device__ __forceinline__ void run(double (&)[P], double (&)[P + 1], int, const LpcFilt&, const float*,
                                               const float*, RowPos&, long long, int, float*) {}
};

constexpr int walk_lds_doubles(int P) {
    return P * LANES > (LANES * WROW + 1) / 2 ? P * LANES : (LANES * WROW + 1) / 2;
}

template <int P>
__global__ void __launch_bounds__(LANES)
k_lpc_synth_walk(const LpcFilt a, long long chunks, long long L, const double* __restrict__ zin) {
    __shared__ double sh[walk_lds_doubles(P)];
    __shared__ long long s_xoff[LANES], s_yoff[LANES];
    __shared__ int s_len[LANES];
    float* tile = (float*)sh;
    const int lane = threadIdx.x, p = a.order;
    const long long nsub = a.rows * chunks;
    const long long q = (long long)blockIdx.x * LANES + lane;
    const bool live = q < nsub;
    const long long row = live ? q / chunks : 0, c = live ? q % chunks : 0;
    const long long start = c * L;
    const int len = live ? (int)(a.n - start < L ? a.n - start : L) : 0;
    s_xoff[lane] = row * a.x_stride + start;
    s_yoff[lane] = row * a.y_stride + start;
    s_len[lane] = len;
    const float* ar = a.a + row * a.a_ch_stride;
    const float* gr = a.gain ? a.gain + row * a.g_ch_stride : nullptr;

    double h[P], cf[P + 1];
    load_state<P>(h, !live ? nullptr : zin ? zin + q * p : a.state ? a.state + row * p : nullptr, p);
    RowPos pos = row_at(a, start);
    load_row<P>(cf, ar, gr, pos.f, a.a_pitch, p);
    __syncthreads();

    const int half = lane >> 5, j = lane & 31;   // this lane's part of a load / store instruction
    float* mine = tile + lane * WROW;
    for (int t0 = 0; t0 < (int)L; t0 += WTILE) {
#pragma unroll 8
        for (int i = 0; i < LANES / 2; ++i) {
            const int r = 2 * i + half;
            tile[r * WROW + j] = t0 + j < s_len[r] ? a.x[s_xoff[r] + t0 + j] : 0.0f;
        }
        __syncthreads();
        TileWalk<P, 0>::template run<true>(h, cf, p, a, ar, gr, pos, start + t0, len - t0, mine);
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < LANES / 2; ++i) {
            const int r = 2 * i + half;
            if (t0 + j < s_len[r]) a.y[s_yoff[r] + t0 + j] = tile[r * WROW + j];
        }
        __syncthreads();
    }

    // the row's end state: the values at sub-row times len - 1 .. len - p of its last sub-row
    dump_ring<P>(sh, h, lane);
    __syncthreads();
    if (!live || !a.state || c != chunks - 1) return;
    for (int k = 1; k <= p; ++k) a.state[row * p + k - 1] = ring_at<P>(sh, lane, len - k);
}

// lane's value of v at a constant lane index
__device__ __forceinline__ float lane_float(float v, int k) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

template <int P, int J>
struct TilePhi {
    static __device__ __forceinline__ void run(double (&h)[P], double (&c)[P + 1], int p, const LpcFilt& a,
                                               const float* ar, const float* gr, RowPos& pos, long long t, int m,
                                               float ev, bool driven) {
        if (J < m) {   // uniform
            if (t + J == pos.next) {
                ++pos.f;
                pos.next = pos.f >= a.frames - 1 ? NEVER : pos.next + a.seg_len;
                load_row<P>(c, ar, gr, pos.f, a.a_pitch, p);
            }
            const double in = c[0] * (double)lane_float(ev, J);
            (void)synth_step<P, J>(h, c, p, driven ? in : 0.0);
        }
        TilePhi<P, J + 1>::run(h, c, p, a, ar, gr, pos, t, m, ev, driven);
    }
};
template <int P>
struct TilePhi<P, WTILE> {
    static __device__ __forceinline__ void run(double (&)[P], double (&)[P + 1], int, const LpcFilt&, const float*,
                                               const float*, RowPos&, long long, int, float, bool) {}
};

template <int P>
__global__ void __launch_bounds__(LANES)
k_lpc_synth_phi(const LpcFilt a, long long chunks, long long L, double* __restrict__ phi, double* __restrict__ z) {
    __shared__ double sh[P * LANES];
    const int lane = threadIdx.x, p = a.order;
    const long long q = blockIdx.x, row = q / chunks, c = q % chunks;
    const long long start = c * L;
    const int len = (int)(a.n - start < L ? a.n - start : L);
    const float* x = a.x + row * a.x_stride + start;
    const float* ar = a.a + row * a.a_ch_stride;
    const float* gr = a.gain ? a.gain + row * a.g_ch_stride : nullptr;

    double h[P], cf[P + 1];
#pragma unroll
    for (int k = 1; k <= P; ++k) h[P - k] = lane == k - 1 && lane < p ? 1.0 : 0.0;   // unit state `lane`
    const bool driven = lane == p;
    RowPos pos = row_at(a, start);
    load_row<P>(cf, ar, gr, pos.f, a.a_pitch, p);
    for (int t0 = 0; t0 < len; t0 += WTILE) {
        const float ev = (lane < WTILE && t0 + lane < len) ? x[t0 + lane] : 0.0f;
        TilePhi<P, 0>::run(h, cf, p, a, ar, gr, pos, start + t0, len - t0, ev, driven);
    }
    dump_ring<P>(sh, h, lane);
    __syncthreads();
    if (lane > p) return;
    double* out = lane < p ? phi + (q * p + lane) * p : z + q * p;
    for (int r = 0; r < p; ++r) out[r] = ring_at<P>(sh, lane, len - 1 - r);
}

template <int P>
__global__ void __launch_bounds__(LANES)
k_lpc_synth_scan(const LpcFilt a, long long chunks, const double* __restrict__ phi, const double* __restrict__ z,
                 double* __restrict__ zin) {
    const int r = threadIdx.x, p = a.order;
    const long long row = blockIdx.x;
    const bool mine = r < p;
    double s = mine && a.state ? a.state[row * p + r] : 0.0;
    double cur[P], nxt[P], zc, zn = 0.0;
    auto load = [&](long long c, double (&col)[P], double& zz) {
        const long long q = row * chunks + c;
#pragma unroll
        for (int i = 0; i < P; ++i) col[i] = mine && i < p ? phi[(q * p + i) * p + r] : 0.0;
        zz = mine ? z[q * p + r] : 0.0;
    };
    load(0, cur, zc);
    for (long long c = 0; c < chunks; ++c) {
        if (c + 1 < chunks) load(c + 1, nxt, zn);
        if (mine) zin[(row * chunks + c) * p + r] = s;
        double acc0 = zc, acc1 = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const double si = __shfl(s, i);
            if (i < p) {
                if (i & 1) acc1 = fma(cur[i], si, acc1);
                else acc0 = fma(cur[i], si, acc0);
            }
        }
        s = acc0 + acc1;
#pragma unroll
        for (int i = 0; i < P; ++i) cur[i] = nxt[i];
        zc = zn;
    }
}

constexpr int ring_of(int order) {
    return order <= 1 ? 1 : order <= 2 ? 2 : order <= 4 ? 4 : order <= 8 ? 8 : order <= 16 ? 16 : 32;
}

#define LPCF_DISPATCH(order, CALL)       \
    switch (ring_of(order)) {            \
        case 1: CALL(1); break;          \
        case 2: CALL(2); break;          \
        case 4: CALL(4); break;          \
        case 8: CALL(8); break;          \
        case 16: CALL(16); break;        \
        default: CALL(32); break;        \
    }

bool filt_ok(const LpcFilt& f) {
    return f.order >= 1 && f.order <= LPCF_MAX_ORDER && f.frames >= 1 && f.seg_len >= 1 && f.n > 0 && f.rows > 0 &&
           f.n < 0x7fffffffLL - WTILE;
}

}  // namespace

hipError_t launch_lpc_residual(const LpcFilt& f, hipStream_t s) {
    if (!filt_ok(f)) return hipErrorInvalidValue;
    const long long tiles = (f.n + LPCF_TILE - 1) / LPCF_TILE;
    if (tiles * f.rows > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lpc_residual, dim3((unsigned)(tiles * f.rows)), dim3(RES_THREADS), 0, s, f, tiles);
    if (f.state) hipLaunchKernelGGL(k_lpc_residual_state, dim3((unsigned)f.rows), dim3(LANES), 0, s, f);
    return hipGetLastError();
}

hipError_t launch_lpc_synth_walk(const LpcFilt& f, long long chunks, long long L, const double* zin, hipStream_t s) {
    if (!filt_ok(f) || chunks < 1 || L < 1 || (chunks - 1) * L >= f.n || chunks * L < f.n || (!zin && chunks != 1))
        return hipErrorInvalidValue;
    const long long blocks = (f.rows * chunks + LANES - 1) / LANES;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
#define CALL(P) hipLaunchKernelGGL((k_lpc_synth_walk<P>), dim3((unsigned)blocks), dim3(LANES), 0, s, f, chunks, L, zin)
    LPCF_DISPATCH(f.order, CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_lpc_synth_phi(const LpcFilt& f, long long chunks, long long L, double* phi, double* z,
                                hipStream_t s) {
    if (!filt_ok(f) || chunks < 1 || L < 1 || (chunks - 1) * L >= f.n || chunks * L < f.n ||
        f.rows * chunks > 0x7fffffffLL)
        return hipErrorInvalidValue;
#define CALL(P) \
    hipLaunchKernelGGL((k_lpc_synth_phi<P>), dim3((unsigned)(f.rows * chunks)), dim3(LANES), 0, s, f, chunks, L, phi, z)
    LPCF_DISPATCH(f.order, CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_lpc_synth_scan(const LpcFilt& f, long long chunks, const double* phi, const double* z, double* zin,
                                 hipStream_t s) {
    if (!filt_ok(f) || chunks < 1 || f.rows > 0x7fffffffLL) return hipErrorInvalidValue;
#define CALL(P) hipLaunchKernelGGL((k_lpc_synth_scan<P>), dim3((unsigned)f.rows), dim3(LANES), 0, s, f, chunks, phi, z, zin)
    LPCF_DISPATCH(f.order, CALL)
#undef CALL
    return hipGetLastError();
}

}  // namespace vvh
