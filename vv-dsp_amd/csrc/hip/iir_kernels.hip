// iir_kernels.hip -- biquad cascades (src/filter/iir.c:21-43), Direct Form II
// Transposed per stage, the reference's operations in its order:
//     y = b0 x + z1;  z1 = (b1 x - a1 y) + z2;  z2 = b2 x - a2 y
// in float, every product and sum rounded (contraction is switched off in the
// walk by pragma: the library's flags leave it on, and the __f*_rn intrinsics
// are plain operators that inherit it).
//
// k_iir_walk<S, WRITE_Y>: one lane owns one sub-row -- a whole row, or one chunk
// of a row -- and runs the S <= 8 stages over it with the 2 S states in
// registers; the coefficients are wave-uniform (scalar registers).  A lane
// reading its own sub-row sample by sample would touch 64 cache lines per load,
// so a wave stages tiles of 64 sub-rows x 32 samples through LDS: each load
// instruction fetches two sub-rows' 32 consecutive samples (two 128 B lines),
// the tile row stride of 33 floats puts lane l's sample j on bank (l + j) mod 32
// (conflict-free for the row-wise stores and the column-wise walk alike), and the
// outputs go back through the same tile.  A workgroup is one wave: waves share
// nothing, so a wider group would only couple them at the barriers.  The tile
// and the sub-row table take 9.7 KB of LDS, which allows 4 waves per SIMD (the
// 76 - 123 VGPRs would allow 4 - 6): enough to cover the recurrence's dependent
// chain, measured in DESIGN.md section 4.
//
// Long rows (launch order of shim_iir.hip, no inter-workgroup waiting): walk
// every chunk of L samples from zero state without output and keep its final
// state zs_c; k_iir_scan propagates z_{c+1} = Phi z_c + zs_c per row in f64,
// Phi the cascade's L-step transition from k_iir_phi; walk every chunk again
// from (float)z_c with output.  The last chunk may be short: the walk's length
// covers it, and nothing follows it, so no second Phi is needed.
#include "vvhip_internal.hpp"

namespace vvh {

namespace {

constexpr int IIR_LANES = 64;
constexpr int IIR_ROW = IIR_TILE + 1;   // floats per tile row in LDS

template <int S>
struct IirCoef {
    float b0[S], b1[S], b2[S], a1[S], a2[S];
};

template <int S>
__device__ __forceinline__ IirCoef<S> iir_load_coef(const float* __restrict__ coef) {
    IirCoef<S> c;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        c.b0[s] = coef[5 * s + 0];
        c.b1[s] = coef[5 * s + 1];
        c.b2[s] = coef[5 * s + 2];
        c.a1[s] = coef[5 * s + 3];
        c.a2[s] = coef[5 * s + 4];
    }
    return c;
}

// one sample through the cascade (iir.c:23-25 per stage, :37-39)
template <int S>
__device__ __forceinline__ float iir_step(const IirCoef<S>& c, float (&z1)[S], float (&z2)[S], float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const float y = c.b0[s] * v + z1[s];
        z1[s] = (c.b1[s] * v - c.a1[s] * y) + z2[s];
        z2[s] = c.b2[s] * v - c.a2[s] * y;
        v = y;
    }
    return v;
}

template <int S, bool WRITE_Y>
__global__ void __launch_bounds__(IIR_LANES) k_iir_walk(const IirWalk a) {
    __shared__ float tile[IIR_LANES * IIR_ROW];
    __shared__ long long s_xoff[IIR_LANES], s_yoff[IIR_LANES];
    __shared__ int s_len[IIR_LANES];
    const int lane = threadIdx.x;
    const long long nsub = a.rows * a.chunks;
    const long long q = (long long)blockIdx.x * IIR_LANES + lane;
    const bool live = q < nsub;
    const long long row = live ? q / a.chunks : 0, c = live ? q % a.chunks : 0;
    const long long start = c * a.L;
    const int len = live ? (int)(a.n - start < a.L ? a.n - start : a.L) : 0;
    s_xoff[lane] = row * a.x_stride + start;
    s_yoff[lane] = row * a.y_stride + start;
    s_len[lane] = len;

    const IirCoef<S> cf = iir_load_coef<S>(a.coef);
    float z1[S], z2[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        z1[s] = live && a.zin ? a.zin[q * a.zin_stride + 2 * s] : 0.0f;
        z2[s] = live && a.zin ? a.zin[q * a.zin_stride + 2 * s + 1] : 0.0f;
    }
    __syncthreads();

    const int half = lane >> 5, j = lane & 31;   // this lane's part of a load / store instruction
    float* mine = tile + lane * IIR_ROW;
    // A tile's 32 loads are issued together, with no branch between them (a load
    // behind a branch waits for the one before it): a slot past its sub-row's end
    // reads the block's first sample instead (sub-row 0 of a block is never
    // empty) and the walk never looks at it.  The next tile's loads are in
    // flight while this tile is walked.
    float pre[IIR_LANES / 2];
    const long long safe = s_xoff[0];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int i = 0; i < IIR_LANES / 2; ++i) {
            const int r = 2 * i + half;
            pre[i] = a.x[t0 + j < s_len[r] ? s_xoff[r] + t0 + j : safe];
        }
    };
    fetch(0);
    for (int t0 = 0; t0 < (int)a.L; t0 += IIR_TILE) {
#pragma unroll
        for (int i = 0; i < IIR_LANES / 2; ++i) tile[(2 * i + half) * IIR_ROW + j] = pre[i];
        __syncthreads();
        if (t0 + IIR_TILE < (int)a.L) fetch(t0 + IIR_TILE);
        const int m = len - t0;   // samples of this lane's sub-row in the tile (<= 0: none)
        if (__all(m >= IIR_TILE)) {
#pragma unroll
            for (int k = 0; k < IIR_TILE; ++k) {
                const float v = iir_step<S>(cf, z1, z2, mine[k]);
                if (WRITE_Y) mine[k] = v;
            }
        } else {
            for (int k = 0; k < IIR_TILE; ++k) {
                if (k < m) {
                    const float v = iir_step<S>(cf, z1, z2, mine[k]);
                    if (WRITE_Y) mine[k] = v;
                }
            }
        }
        __syncthreads();
        if (WRITE_Y) {
#pragma unroll 8
            for (int i = 0; i < IIR_LANES / 2; ++i) {
                const int r = 2 * i + half;
                if (t0 + j < s_len[r]) a.y[s_yoff[r] + t0 + j] = tile[r * IIR_ROW + j];
            }
            __syncthreads();
        }
    }

    if (!live || !a.zout) return;
    long long o;
    if (WRITE_Y) {
        if (c != a.chunks - 1) return;
        o = row * a.zout_stride;
    } else {
        o = q * a.zout_stride;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        a.zout[o + 2 * s] = z1[s];
        a.zout[o + 2 * s + 1] = z2[s];
    }
}

// Column j of Phi: the state after L samples of zero input from the unit state
// e_j, in f64 from the float coefficients.  One thread per column.
__global__ void k_iir_phi(const float* __restrict__ coef, int stages, long long L, double* phi) {
    const int D = 2 * stages, col = threadIdx.x;
    if (col >= D) return;
    double z1[IIR_MAX_STAGES], z2[IIR_MAX_STAGES];
    for (int s = 0; s < IIR_MAX_STAGES; ++s) {
        z1[s] = col == 2 * s ? 1.0 : 0.0;
        z2[s] = col == 2 * s + 1 ? 1.0 : 0.0;
    }
    for (long long t = 0; t < L; ++t) {
        double v = 0.0;
        for (int s = 0; s < IIR_MAX_STAGES; ++s) {
            if (s < stages) {
                const double b0 = coef[5 * s], b1 = coef[5 * s + 1], b2 = coef[5 * s + 2], a1 = coef[5 * s + 3],
                             a2 = coef[5 * s + 4];
                const double y = b0 * v + z1[s];
                z1[s] = b1 * v - a1 * y + z2[s];
                z2[s] = b2 * v - a2 * y;
                v = y;
            }
        }
    }
    for (int s = 0; s < IIR_MAX_STAGES; ++s) {
        if (s < stages) {
            phi[(2 * s) * D + col] = z1[s];
            phi[(2 * s + 1) * D + col] = z2[s];
        }
    }
}

// lane k's value of v, the same in every lane (k a constant)
__device__ __forceinline__ double lane_value(double v, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

// One wave per row.  The 2 S state components of G = 64 / D consecutive chunks
// fill the wave's lanes: lane l = g D + i loads chunk (c0 + g)'s zero-state final
// component i (one coalesced load per G chunks, issued two blocks ahead: the
// step below is a dependent chain, and a load inside it would set its length)
// and stores chunk (c0 + g)'s incoming component i.  Every lane carries the
// chain of its component i in f64 with row i of Phi in registers -- the G lane
// groups compute the same values, and group g keeps the one of its chunk.
template <int S>
__global__ void __launch_bounds__(IIR_LANES) k_iir_scan(const double* __restrict__ phi, const float* __restrict__ zs,
                                                        const float* __restrict__ zrow, long long zrow_stride,
                                                        long long chunks, float* __restrict__ zin) {
    constexpr int D = 2 * S, G = IIR_LANES / D;
    __shared__ float s_add[IIR_LANES];
    const int lane = threadIdx.x, i = lane % D, g = lane / D;
    const bool active = g < G;
    const long long row = blockIdx.x, total = chunks * D;   // floats of this row in zs and zin
    const float* zsr = zs + row * total;
    float* zinr = zin + row * total;
    double p[D];
#pragma unroll
    for (int k = 0; k < D; ++k) p[k] = phi[i * D + k];
    double z = zrow ? (double)zrow[row * zrow_stride + i] : 0.0;
    auto load = [&](long long c0) {
        const long long e = c0 * D + lane;
        return active && e < total ? zsr[e] : 0.0f;
    };
    float ld0 = load(0), ld1 = load(G);
    for (long long c0 = 0; c0 < chunks; c0 += G) {
        s_add[lane] = ld0;
        ld0 = ld1;
        ld1 = load(c0 + 2 * G);
        __syncthreads();
        float keep = 0.0f;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            if (g == u) keep = (float)z;   // chunk c0 + u starts from z, rounded to float
            // component k comes from lane k's registers (no LDS round trip), and
            // the D products are summed as two interleaved chains
            double acc0 = (double)s_add[u * D + i], acc1 = 0.0;
#pragma unroll
            for (int k = 0; k < D; k += 2) {
                acc0 = fma(p[k], lane_value(z, k), acc0);
                acc1 = fma(p[k + 1], lane_value(z, k + 1), acc1);
            }
            z = acc0 + acc1;
        }
        const long long e = c0 * D + lane;
        if (active && e < total) zinr[e] = keep;
        __syncthreads();
    }
}

template <int S>
hipError_t iir_walk_s(const IirWalk& w, int write_y, unsigned blocks, hipStream_t s) {
    if (write_y) hipLaunchKernelGGL((k_iir_walk<S, true>), dim3(blocks), dim3(IIR_LANES), 0, s, w);
    else hipLaunchKernelGGL((k_iir_walk<S, false>), dim3(blocks), dim3(IIR_LANES), 0, s, w);
    return hipGetLastError();
}

template <int S>
hipError_t iir_scan_s(const double* phi, const float* zs, const float* zrow, long long zrow_stride, long long rows,
                      long long chunks, float* zin, hipStream_t s) {
    hipLaunchKernelGGL((k_iir_scan<S>), dim3((unsigned)rows), dim3(IIR_LANES), 0, s, phi, zs, zrow, zrow_stride, chunks,
                       zin);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_iir_walk(const IirWalk& w, int stages, int write_y, hipStream_t s) {
    if (w.rows <= 0 || w.n <= 0) return hipSuccess;
    if (stages < 1 || stages > IIR_MAX_STAGES || w.chunks < 1 || w.L < 1 || w.L > 0x7fffffffLL - IIR_TILE ||
        (w.chunks - 1) * w.L >= w.n)
        return hipErrorInvalidValue;
    const long long blocks = (w.rows * w.chunks + IIR_LANES - 1) / IIR_LANES;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    switch (stages) {
        case 1: return iir_walk_s<1>(w, write_y, (unsigned)blocks, s);
        case 2: return iir_walk_s<2>(w, write_y, (unsigned)blocks, s);
        case 3: return iir_walk_s<3>(w, write_y, (unsigned)blocks, s);
        case 4: return iir_walk_s<4>(w, write_y, (unsigned)blocks, s);
        case 5: return iir_walk_s<5>(w, write_y, (unsigned)blocks, s);
        case 6: return iir_walk_s<6>(w, write_y, (unsigned)blocks, s);
        case 7: return iir_walk_s<7>(w, write_y, (unsigned)blocks, s);
        default: return iir_walk_s<8>(w, write_y, (unsigned)blocks, s);
    }
}

hipError_t launch_iir_phi(const float* coef, int stages, long long L, double* phi, hipStream_t s) {
    if (stages < 1 || stages > IIR_MAX_STAGES || L < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_iir_phi, dim3(1), dim3(IIR_LANES), 0, s, coef, stages, L, phi);
    return hipGetLastError();
}

hipError_t launch_iir_scan(const double* phi, int stages, const float* zs, const float* zrow, long long zrow_stride,
                           long long rows, long long chunks, float* zin, hipStream_t s) {
    if (rows <= 0 || chunks <= 0) return hipSuccess;
    if (stages < 1 || stages > IIR_MAX_STAGES || rows > 0x7fffffffLL) return hipErrorInvalidValue;
    switch (stages) {
        case 1: return iir_scan_s<1>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
        case 2: return iir_scan_s<2>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
        case 3: return iir_scan_s<3>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
        case 4: return iir_scan_s<4>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
        case 5: return iir_scan_s<5>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
        case 6: return iir_scan_s<6>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
        case 7: return iir_scan_s<7>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
        default: return iir_scan_s<8>(phi, zs, zrow, zrow_stride, rows, chunks, zin, s);
    }
}

}  // namespace vvh
