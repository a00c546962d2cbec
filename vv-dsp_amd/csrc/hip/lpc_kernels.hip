// lpc_kernels.hip -- batched linear prediction for gfx950: autocorrelation,
// the Levinson-Durbin recursion and the all-pole spectrum of
// src/envelope/lpc.c, over rows or over the frames of a signal.
//
// Autocorrelation, wave kernel (order <= 32, row length <= 4096).  One wave
// takes one row.  The row (of a FrameSrc: a frame is read through frame_sample,
// frame_src.hpp, as k_fetch_frames reads it) goes to LDS; lane l owns samples
// [l C, (l + 1) C), C = the row length over 64 rounded up to a multiple of 8, and walks them in
// tiles of 8: one tile is 8 + P samples read as float4 (P = 16 or 32, the
// template's order bound) and 8 (P + 1) FMAs from registers, 0.15 LDS floats
// per FMA at P = 32.  Samples past the row's end are stored as zeros, so their
// products add exact zeros.  The P + 1 partial sums per lane are transposed
// through LDS and lane k adds lag k's 64 partials in a fixed shape.  The order
// of every sum depends on the row length alone -- not on the batch, the
// frame's position or the entry point -- which is what makes lpc == levinson
// (autocorr) and lpc_frames == lpc(fetch_frames) hold bit for bit.
//
// LDS image of a row: logical sample i at i + 4 (i / C).  Lane l's float4 reads
// start (C + 4) floats apart, an odd number of 16-B slots (C / 4 is even), so
// the 16 lanes of a ds_read_b128 group cover 16 distinct slots.  A lane stages
// its own chunk (wide loads, float4 stores, no index arithmetic); only a row
// that leaves the signal -- a frame at either end -- is staged sample by sample.
// A non-finite sample makes r[0] non-finite as in the reference; the other
// lags may then be NaN where the reference has an infinity (0 x inf in the
// zero padding).
//
// Levinson: one lane per row with a[] and r[] in registers (all indices static
// after unrolling), the reference's operation order with every product, sum and
// quotient rounded separately (lpc.c:24-38 under -ffp-contract=off): bit-identical
// to the reference given the same r.  A workgroup of the wave kernel takes 64
// rows: its four waves leave 16 autocorrelation rows each in LDS, then wave 0
// runs the 64 recursions, one per lane.
//
// Generic kernels (any order < row length): one workgroup per autocorrelation
// row, lag by lag; one thread per Levinson row working in the output row.
#include "frame_src.hpp"
#include "wave_sync.hpp"

namespace vvh {

namespace {

__device__ __forceinline__ float* lpc_out_row(const LpcOut& o, long long row, int order, float** err) {
    const long long ch = row / o.frames, f = row - ch * o.frames;
    *err = o.err + ch * o.err_ch_stride + f;
    return o.a + ch * o.a_ch_stride + f * (order + 1);
}

// four consecutive floats at any 4-byte-aligned address as one load (a frame
// starts wherever its hop puts it)
struct __attribute__((packed, aligned(4))) F4u {
    float x, y, z, w;
};
__device__ __forceinline__ F4u ld4u(const float* p) { return *reinterpret_cast<const F4u*>(p); }

constexpr int RED_STRIDE = 68;   // floats per lag row of the transpose: 17 slots, odd

// lpc.c:24-38 on registers.  a[0] is 1 once the loop has run and the calloc'd 0
// at order 0, as the reference leaves it.  r[0] <= 0 (the reference's INTERNAL):
// a = {1, 0, ...}, err = 0, returns false.
template <int P>
__device__ __forceinline__ bool levinson_regs(const float (&r)[P + 1], int order, float (&a)[P + 1], float* err) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i <= P; ++i) a[i] = 0.0f;
    float e = r[0];
    if (e <= 0.0f) {
        a[0] = 1.0f;
        *err = 0.0f;
        return false;
    }
    if (order > 0) a[0] = 1.0f;
#pragma unroll
    for (int m = 1; m <= P; ++m) {
        if (m <= order) {
            float acc = r[m];
#pragma unroll
            for (int i = 1; i < m; ++i) acc = acc + a[i] * r[m - i];
            const float k = -acc / e;
#pragma unroll
            for (int i = 1; 2 * i <= m; ++i) {
                const float ai = a[i], aj = a[m - i];
                a[i] = ai + k * aj;
                if (2 * i < m) a[m - i] = aj + k * ai;
            }
            a[m] = k;
            e = e * (1.0f - k * k);
        }
    }
    *err = e;
    return true;
}

template <int P>
__device__ __forceinline__ void levinson_store(const float (&r)[P + 1], int order, long long row, const LpcOut& out) {
    float a[P + 1], e;
    const bool ok = levinson_regs<P>(r, order, a, &e);
    float* ep;
    float* ap = lpc_out_row(out, row, order, &ep);
#pragma unroll
    for (int k = 0; k <= P; ++k)
        if (k <= order) ap[k] = a[k];
    *ep = e;
    if (!ok && out.flag) *out.flag = 1;
}

// 64 rows per workgroup, 16 per wave.  Dynamic LDS: r rows [64][P + 1], then one
// buffer of wbuf floats per wave (the row's image, then the transpose).
template <int P>
__global__ void __launch_bounds__(256) k_lpc_wave(FrameSrc src, int order, int C, int wbuf, float* __restrict__ r_out,
                                                  LpcOut out) {
    extern __shared__ float4 lpc_lds4[];
    constexpr int RS = P + 1;            // odd: 64 lanes read 64 rows conflict-free
    constexpr int RR = (64 * RS + 3) / 4 * 4;
    constexpr int NV = (8 + P) / 4;      // float4 reads per tile
    float* rrows = reinterpret_cast<float*>(lpc_lds4);
    // the wave's number as a scalar: the row, its channel and frame and the
    // row's base pointer are then wave-uniform values the scalar unit keeps
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    float* xb = rrows + RR + wave * wbuf;
    const long long row0 = (long long)blockIdx.x * 64;
    // (channel, frame) of the workgroup's first row: one division per workgroup, steps from there
    const long long ch0 = src.framed ? row0 / src.frames : 0;
    const long long f0 = row0 - ch0 * src.frames;
    const int n = (int)src.len;
    const int total = 64 * C + P;        // logical samples of the image, zeros from n on
    const int dq = 64 / C, dr = 64 % C;
    const int lq = lane / C, lr = lane % C;
    // the lane's chunk in the image (16-B aligned: xb is, and C + 4 is a multiple of 4),
    // and the image's place for look-ahead sample 64 C + lane
    float* xl = static_cast<float*>(__builtin_assume_aligned(xb + lane * (C + 4), 16));
    const int zoff = 64 * (C + 4) + lane + 4 * lq;

    for (int f = wave; f < 64; f += 4) {
        const long long row = row0 + f;
        if (row >= src.rows) break;      // the same for the whole wave
        long long ch = ch0, fr = f0 + f;
        while (src.framed && fr >= src.frames) {
            fr -= src.frames;
            ++ch;
        }
        const FrameRow<> rw = frame_row(src, row, ch, fr);
        wave_sync();                     // the previous row's transpose has been read
        // A row inside the signal and at least a chunk long (every row of a batch,
        // every frame but the few at the ends): a lane loads its own chunk, 8
        // consecutive samples at a time by straight-line code, so the loads are wide
        // and all in flight before the first store, and its part of the image is two
        // float4 stores with no index arithmetic.  A lane whose chunk passes the
        // row's end stores zeros (it loads from the row's start, a valid place);
        // the one lane the end falls inside then adds its few samples one by one.
        if (rw.inside && n >= C) {
            const bool full = lane * C + C <= n;
            const float* fp = rw.p + rw.start + (full ? lane * C : 0);
            const float* wp = src.win + (full ? lane * C : 0);
            float* xw = xl;
            if (src.win) {
#pragma unroll 1
                for (int u0 = 0; u0 < C; u0 += 8) {
                    const F4u xa = ld4u(fp + u0), xc = ld4u(fp + u0 + 4), wa = ld4u(wp + u0), wc = ld4u(wp + u0 + 4);
                    float v[8] = {xa.x * wa.x, xa.y * wa.y, xa.z * wa.z, xa.w * wa.w,
                                  xc.x * wc.x, xc.y * wc.y, xc.z * wc.z, xc.w * wc.w};
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = full ? v[u] : 0.0f;
                    *reinterpret_cast<float4*>(xw + u0) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(xw + u0 + 4) = make_float4(v[4], v[5], v[6], v[7]);
                }
            } else {
#pragma unroll 1
                for (int u0 = 0; u0 < C; u0 += 8) {
                    const F4u xa = ld4u(fp + u0), xc = ld4u(fp + u0 + 4);
                    float v[8] = {xa.x, xa.y, xa.z, xa.w, xc.x, xc.y, xc.z, xc.w};
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = full ? v[u] : 0.0f;
                    *reinterpret_cast<float4*>(xw + u0) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4*>(xw + u0 + 4) = make_float4(v[4], v[5], v[6], v[7]);
                }
            }
            if (lane < P) xb[zoff] = 0.0f;           // the look-ahead past the last chunk
            if (!full && lane * C < n)               // the chunk the row ends in
                for (int i = lane * C; i < n; ++i) xw[i - lane * C] = frame_sample<true>(src, rw, i);
        } else {
            int q = lq, rem = lr;
            for (int i = lane; i < total; i += 64) {
                xb[i + 4 * q] = i < n ? frame_sample(src, rw, i) : 0.0f;
                q += dq;
                rem += dr;
                if (rem >= C) {
                    rem -= C;
                    ++q;
                }
            }
        }
        wave_sync();
        float acc[P + 1];
#pragma unroll
        for (int k = 0; k <= P; ++k) acc[k] = 0.0f;
        int q0 = 0, r0 = 0;              // (8 t) / C and (8 t) % C
        for (int t = 0; t < C; t += 8) {
            float ys[8 + P];
            int q = q0, rem = r0;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float4 v = *reinterpret_cast<const float4*>(xl + t + 4 * j + 4 * q);
                ys[4 * j] = v.x;
                ys[4 * j + 1] = v.y;
                ys[4 * j + 2] = v.z;
                ys[4 * j + 3] = v.w;
                rem += 4;
                if (rem == C) {
                    rem = 0;
                    ++q;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int k = 0; k <= P; ++k) acc[k] = __builtin_fmaf(ys[u], ys[u + k], acc[k]);
            r0 += 8;
            if (r0 == C) {
                r0 = 0;
                ++q0;
            }
        }
        wave_sync();                     // every lane's tile reads are done: the buffer becomes the transpose
#pragma unroll
        for (int k = 0; k <= P; ++k)
            if (k <= order) xb[k * RED_STRIDE + lane] = acc[k];
        wave_sync();
        if (lane <= order) {
            const float4* pr = reinterpret_cast<const float4*>(xb + lane * RED_STRIDE);
            float4 s4 = pr[0];
#pragma unroll
            for (int j = 1; j < 16; ++j) {
                const float4 v = pr[j];
                s4.x += v.x;
                s4.y += v.y;
                s4.z += v.z;
                s4.w += v.w;
            }
            const float rk = (s4.x + s4.y) + (s4.z + s4.w);
            if (r_out) r_out[row * (order + 1) + lane] = rk;
            else rrows[f * RS + lane] = rk;
        }
    }
    if (r_out) return;
    __syncthreads();
    if (wave != 0) return;
    const long long row = row0 + lane;
    if (row >= src.rows) return;
    float r[P + 1];
#pragma unroll
    for (int k = 0; k <= P; ++k) r[k] = k <= order ? rrows[lane * RS + k] : 0.0f;
    levinson_store<P>(r, order, row, out);
}

template <int P>
__global__ void __launch_bounds__(64) k_levinson(const float* __restrict__ rin, int order, long long rows, LpcOut out) {
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const float* rr = rin + row * (order + 1);
    float r[P + 1];
#pragma unroll
    for (int k = 0; k <= P; ++k) r[k] = k <= order ? rr[k] : 0.0f;
    levinson_store<P>(r, order, row, out);
}

// the same recursion in the output row (any order); a and r must not overlap
__global__ void __launch_bounds__(64) k_levinson_generic(const float* __restrict__ rin, long long order, long long rows,
                                                         LpcOut out) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const float* r = rin + row * (order + 1);
    float* ep;
    float* a = lpc_out_row(out, row, (int)order, &ep);
    for (long long i = 0; i <= order; ++i) a[i] = 0.0f;
    float e = r[0];
    if (e <= 0.0f) {
        a[0] = 1.0f;
        *ep = 0.0f;
        if (out.flag) *out.flag = 1;
        return;
    }
    if (order > 0) a[0] = 1.0f;
    for (long long m = 1; m <= order; ++m) {
        float acc = r[m];
        for (long long i = 1; i < m; ++i) acc = acc + a[i] * r[m - i];
        const float k = -acc / e;
        for (long long i = 1; 2 * i <= m; ++i) {
            const float ai = a[i], aj = a[m - i];
            a[i] = ai + k * aj;
            if (2 * i < m) a[m - i] = aj + k * ai;
        }
        a[m] = k;
        e = e * (1.0f - k * k);
    }
    *ep = e;
}

// one workgroup per row: thread t adds the products of samples t, t + 256, ...
// of lag k, then a fixed tree over the 256 partial sums
__global__ void __launch_bounds__(256) k_autocorr_generic(FrameSrc src, long long order, float* __restrict__ r_out) {
    __shared__ float red[256];
    const long long row = blockIdx.x;
    const FrameRow<> rw = frame_row(src, row);
    const int t = threadIdx.x;
    for (long long k = 0; k <= order; ++k) {
        float s = 0.0f;
        for (long long i = t; i < src.len - k; i += 256)
            s = __builtin_fmaf(frame_sample(src, rw, i), frame_sample(src, rw, i + k), s);
        red[t] = s;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (t < h) red[t] += red[t + h];
            __syncthreads();
        }
        if (t == 0) r_out[row * (order + 1) + k] = red[0];
        __syncthreads();
    }
}

// One wave per row, one lane per bin k <= nfft / 2; bin nfft - k is the same
// value (real coefficients: A(e^-jw) = conj A(e^jw)) and is stored from it.  The
// angle of term (m, k) is 2 pi ((m k) mod nfft) / nfft with the residue kept as
// an integer; its cosine and sine come from a table built per workgroup in f64
// and rounded once (TABLE), or from sincospi in f64.  The row's coefficients
// are wave-uniform loads.  Table entry j sits at j + j / 32: lanes k, k + 1, ..
// read entries m apart, and without the skew an even m puts them on few banks.
// Dynamic LDS (TABLE): float2 tab[lpspec_slot(nfft)].
__host__ __device__ constexpr unsigned lpspec_slot(unsigned j) { return j + (j >> 5); }

template <bool TABLE>
__global__ void __launch_bounds__(256) k_lpspec(const float* __restrict__ a, int order, const float* __restrict__ gain,
                                                float gain1, unsigned nfft, long long batch, int plus,
                                                float* __restrict__ mag) {
    extern __shared__ float4 lpspec_lds4[];
    float2* tab = reinterpret_cast<float2*>(lpspec_lds4);
    if (TABLE) {
        for (unsigned j = threadIdx.x; j < nfft; j += 256) {
            double sn, cs;
            sincospi(2.0 * (double)j / (double)nfft, &sn, &cs);
            tab[lpspec_slot(j)] = make_float2((float)cs, (float)sn);
        }
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned lane = threadIdx.x & 63;
    const unsigned half = nfft / 2 + 1;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < batch; row += (long long)gridDim.x * 4) {
        const float* ar = a + row * (order + 1);
        const float g = gain ? gain[row] : gain1;
        float* out = mag + row * nfft;
        for (unsigned k = lane; k < half; k += 64) {
            float re = 1.0f, im = 0.0f;
            unsigned j = 0;
            for (int m = 1; m <= order; ++m) {
                j += k;
                j = min(j, j - nfft);   // j < 2 nfft: j - nfft wraps above j exactly when j < nfft
                float2 w;
                if (TABLE) {
                    w = tab[lpspec_slot(j)];
                } else {
                    double sn, cs;
                    sincospi(2.0 * (double)j / (double)nfft, &sn, &cs);
                    w = make_float2((float)cs, (float)sn);
                }
                const float am = plus ? ar[m] : -ar[m];
                re = __builtin_fmaf(am, w.x, re);
                im = __builtin_fmaf(am, w.y, im);
            }
            const float den = sqrtf(__builtin_fmaf(re, re, im * im));
            const float v = den > 0.0f ? g / den : 0.0f;
            __builtin_nontemporal_store(v, out + k);
            if (k != 0 && nfft - k != k) __builtin_nontemporal_store(v, out + (nfft - k));
        }
    }
}

constexpr size_t LPSPEC_TABLE_BYTES = 64u << 10;

}  // namespace

hipError_t launch_lpc_wave(const FrameSrc& src, int order, float* r, const LpcOut& out, hipStream_t s) {
    if (src.rows <= 0) return hipSuccess;
    if (!lpc_wave_supported(src.len, order)) return hipErrorInvalidValue;
    const long long blocks = (src.rows + 63) / 64;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const int P = order <= 16 ? 16 : 32;
    const int C = (int)(((src.len + 63) / 64 + 7) / 8 * 8);
    const int total = 64 * C + P;
    int wbuf = total + 4 * ((total - 1) / C);   // physical index of the last logical sample, plus one
    if (wbuf < (P + 1) * RED_STRIDE) wbuf = (P + 1) * RED_STRIDE;
    wbuf = (wbuf + 3) / 4 * 4;
    const size_t lds = ((size_t)(64 * (P + 1) + 3) / 4 * 4 + 4 * (size_t)wbuf) * sizeof(float);
    auto kern = P == 16 ? k_lpc_wave<16> : k_lpc_wave<32>;
    if (lds > (48u << 10)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 96 << 10);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, s, src, order, C, wbuf, r, out);
    return hipGetLastError();
}

hipError_t launch_autocorr_generic(const FrameSrc& src, long long order, float* r, hipStream_t s) {
    if (src.rows <= 0) return hipSuccess;
    if (src.rows > 0x7fffffffLL || order >= src.len) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_autocorr_generic, dim3((unsigned)src.rows), dim3(256), 0, s, src, order, r);
    return hipGetLastError();
}

hipError_t launch_levinson(const float* r, long long order, long long rows, int generic, const LpcOut& out,
                           hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    const long long blocks = (rows + 63) / 64;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (generic) {
        hipLaunchKernelGGL(k_levinson_generic, dim3((unsigned)blocks), dim3(64), 0, s, r, order, rows, out);
        return hipGetLastError();
    }
    if (order > LPC_WAVE_ORDER) return hipErrorInvalidValue;
    auto kern = order <= 16 ? k_levinson<16> : k_levinson<32>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), 0, s, r, (int)order, rows, out);
    return hipGetLastError();
}

hipError_t launch_lpspec(const float* a, long long order, const float* gain, float gain1, long long nfft,
                         long long batch, int plus, float* mag, hipStream_t s) {
    if (batch <= 0 || nfft <= 0) return hipSuccess;
    if (nfft >= (1LL << 30) || order >= (1LL << 30)) return hipErrorInvalidValue;
    const size_t need = 8 * ((size_t)lpspec_slot((unsigned)nfft - 1) + 1);
    const bool table = need <= LPSPEC_TABLE_BYTES;
    const size_t lds = table ? (need + 15) / 16 * 16 : 0;
    auto kern = table ? k_lpspec<true> : k_lpspec<false>;
    if (lds > (48u << 10)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)LPSPEC_TABLE_BYTES);
        if (e != hipSuccess) return e;
    }
    // a workgroup builds its table once and its four waves walk rows: enough workgroups to fill the chip
    const long long need_blocks = (batch + 3) / 4;
    const long long blocks = need_blocks < 2048 ? need_blocks : 2048;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, s, a, (int)order, gain, gain1, (unsigned)nfft,
                       batch, plus, mag);
    return hipGetLastError();
}

}  // namespace vvh
