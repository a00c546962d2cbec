// mixed_common.hpp -- what the mixed-radix kernel families share (the LDS plan
// kernel mixed_plan.hip, the four-step mixed_fourstep.hip, the register kernel
// sq_kernel.hpp) and what their router mixed_fft.hip calls: the plan, the
// transform's I/O description, the small odd DFTs, and the one copy of each
// rule for STFT frame pairs and row stores.  Private to these units.
#pragma once
#include "fft_core.hpp"
#include "vvhip_internal.hpp"

namespace vvh {

constexpr int MIX_MAXP = 12;    // 3^7 = 2187 needs 7 passes; 4096-bounded lengths fit in 12
constexpr int MIX_MAXN = 4096;

struct MixedPlan {
    int n;
    int np;
    int radix[MIX_MAXP];
    int ns[MIX_MAXP];
    int tstep[MIX_MAXP];   // n / (Ns * R): W_{Ns R}^m = W_n^(m * tstep)
    float rns[MIX_MAXP];   // 1 / Ns for the butterfly index split
};

// Where a transform's points come from and go to.
//   MODE 0: complex rows (nout bins out, scaled; the inverse by conjugation).
//   MODE 4: real rows (imaginary zero), nout bins out.
//   MODE 5: real rows of length 2n through an n-point transform of
//           z[m] = x[2m] + i x[2m+1] and the split step (nout <= n + 1 bins).
//   MODE 1/2/3: STFT frames of a [ch][n] signal, frames (2j, 2j+1) of one
//           channel per complex transform (frame f starts at sample f*hop, zero
//           past the end, times the window: frame_gather's single rounded
//           product) -> |X| rows (1), complex rows (2) or |X|^2 for bins
//           0..n/2 (3).  Pairs never span channels.
struct MixIO {
    const void* in;
    float2* out;
    long long nout, in_dist, out_dist;
    // STFT: output rows 16 B aligned (base and channel stride), for 16 B/lane row stores.
    // Here, not with the STFT fields: at the end the scalar loads of k_fft_mixed<64, 0>
    // group differently and 1000-point c2c rows measured 1.1 % slower.
    int a16;
    float scale;
    float isign;   // -1 for the inverse: conj(FFT(conj x))
    // STFT
    long long sig_n, ch_stride, frames, ppc, hop, out_ch_stride;
    const float* win;
    const float2* twn;   // MODE 5: W_n^k, k < n (n = 2 * the transform length)
};

// ---- host side: the router (mixed_fft.hip) and the units it routes to -------
// radices largest first: 8s, then a 4 or 2, then 7, 5, 3; false: n has no single-pass plan
bool make_plan(long long n, MixedPlan* pl);
// threads per transform of the plan kernels (16, 32, 64 or 256)
int mixed_threads(long long n);
// f(integral_constant<int, T>) for the thread count T of an n-point plan
template <class F>
hipError_t with_mixed_threads(long long n, F&& f) {
    switch (mixed_threads(n)) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        default: return f(std::integral_constant<int, 256>{});
    }
}
// Blocks of a plan or register kernel over `work` blocks of work: persistent
// (the kernel's resident grid), or every block's work once
inline int mixed_grid(bool once, const void* kernel, size_t lds, long long work) {
    return once ? capped_grid(1 << 30, work) : persistent_grid(kernel, 256, lds, work);
}
// mixed_plan.hip: k_fft_mixed<T, mode> over `batch` transforms of plan pl
hipError_t run_mixed(int mode, const MixedPlan& pl, const MixIO& io, long long batch, hipStream_t s);
// mixed_fourstep.hip: 7-smooth n > 4096 as N1 x N2; fs_split false: no such split
bool fs_split(long long n, int* n1, int* n2);
hipError_t launch_fft_mixed_fs(long long n, int fwd, const void* in, int real_in, float2* out, long long nout,
                               long long batch, long long in_dist, long long out_dist, float scale, hipStream_t s);
// The register kernel (sq_kernel.hpp) for its lengths; false: not one of them
// (or knob STFT_SQ = 0), else *e is the launch's status.
// sq_rows.hip: c2c rows of n points; real rows of n2 = 2 x a (half) length
bool sq_c2c(long long n, const MixIO& io, long long batch, hipStream_t s, hipError_t* e);
bool sq_r2c(long long n2, const MixIO& io, long long batch, hipStream_t s, hipError_t* e);
// sq_stft.hip: STFT frame pairs, kind 0 |X|, 1 complex, 2 |X|^2 rows
bool sq_stft(long long nfft, int kind, const MixIO& io, long long pairs, hipStream_t s, hipError_t* e);

// ---- device side -----------------------------------------------------------
// cos / sin(2*pi*j/R) for the odd radices, j = 1 .. (R-1)/2
template <int R>
struct OddC;
template <>
struct OddC<3> {
    __device__ static constexpr float c(int) { return -0.5f; }
    __device__ static constexpr float s(int) { return 0.86602540378443864676f; }
};
template <>
struct OddC<5> {
    __device__ static constexpr float c(int j) { return j == 1 ? 0.30901699437494742410f : -0.80901699437494742410f; }
    __device__ static constexpr float s(int j) { return j == 1 ? 0.95105651629515357212f : 0.58778525229247312917f; }
};
template <>
struct OddC<7> {
    __device__ static constexpr float c(int j) {
        return j == 1 ? 0.62348980185873353053f : j == 2 ? -0.22252093395631440429f : -0.90096886790241912624f;
    }
    __device__ static constexpr float s(int j) {
        return j == 1 ? 0.78183148246802980871f : j == 2 ? 0.97492791218182360702f : 0.43388373911755812048f;
    }
};

// forward DFT of odd length R over symmetric pairs s_m = x_m + x_{R-m},
// d_m = x_m - x_{R-m}:  X_k = x0 + sum_m cos(2 pi k m / R) s_m - i sum_m sin(2 pi k m / R) d_m,
// X_{R-k} the same with +i.
template <int R>
__device__ __forceinline__ void odd_dft(float2* v) {
    constexpr int H = (R - 1) / 2;
    float2 s[H], d[H];
#pragma unroll
    for (int m = 1; m <= H; ++m) {
        s[m - 1] = cadd(v[m], v[R - m]);
        d[m - 1] = csub(v[m], v[R - m]);
    }
    const float2 x0 = v[0];
    float2 sum = x0;
#pragma unroll
    for (int m = 0; m < H; ++m) sum = cadd(sum, s[m]);
    v[0] = sum;
#pragma unroll
    for (int k = 1; k <= H; ++k) {
        vf2_t a = pk(x0), b = vf2_t{0.0f, 0.0f};
#pragma unroll
        for (int m = 1; m <= H; ++m) {
            const int j = (k * m) % R;
            const int jj = j <= H ? j : R - j;            // cos symmetric, sin antisymmetric
            const float c = OddC<R>::c(jj);
            const float sn = j <= H ? OddC<R>::s(jj) : -OddC<R>::s(jj);
            a = a + pk(s[m - 1]) * c;
            b = b + pk(d[m - 1]) * sn;
        }
        // X_k = a - i b = (a.x + b.y, a.y - b.x);  X_{R-k} = a + i b
        v[k] = cadd_i<false>(upk(a), upk(b));
        v[R - k] = cadd_i<true>(upk(a), upk(b));
    }
}

template <int R>
__device__ __forceinline__ void dft_fwd(float2* v) {
    if constexpr (R == 2 || R == 4 || R == 8)
        Dft<R, true>::run(v);
    else
        odd_dft<R>(v);
}

// Frame pair q of an STFT (MODE 1/2/3) with rows of W bins: frames fra and
// fra + 1 of channel c.  (k_stft_sq's pass 1 and staged emit write this rule out
// themselves, sq_kernel.hpp says why.)
struct FramePair {
    long long c, fra;
    const float *ra, *rb;   // the frames' first samples
    long long lima, limb;   // samples of each frame inside the signal (limb 0: no second frame)
    bool has_b;
    long long out;          // row a's first bin in the output, in bins; row b follows it
};
__device__ __forceinline__ FramePair frame_pair(const MixIO& io, long long q, long long W) {
    FramePair p;
    p.c = q / io.ppc;
    p.fra = 2 * (q - p.c * io.ppc);
    p.has_b = p.fra + 1 < io.frames;
    const long long st = p.fra * io.hop;
    p.ra = reinterpret_cast<const float*>(io.in) + p.c * io.ch_stride + st;
    p.rb = p.ra + io.hop;
    p.lima = io.sig_n - st;
    p.limb = p.has_b ? p.lima - io.hop : 0;
    p.out = p.c * io.out_ch_stride + p.fra * W;
    return p;
}

// Sample s of the frames starting at ra and rb (lima, limb samples inside the
// signal) times the window value win[s].  Past the signal's end a load reads
// `mapped` (the window in global memory, always mapped) instead and the value
// is zeroed: no branch around the loads.
__device__ __forceinline__ float2 pair_load(const float* ra, const float* rb, long long lima, long long limb, int s,
                                            const float* mapped, const float* win) {
    const bool ia = s < lima, ib = s < limb;
    const float a = *(ia ? ra + s : mapped + s), b = *(ib ? rb + s : mapped + s);
    const float w = win[s];
    return make_float2((ia ? a : 0.0f) * w, (ib ? b : 0.0f) * w);
}

// Bin e of real frames a and b from Z = FFT(a + i b): z = Z[e], m = Z[n - e]
// (m = Z[0] at e = 0) -> X_a = (z + conj m) / 2, X_b = -i (z - conj m) / 2.
__device__ __forceinline__ void pair_split(float2 z, float2 m, float2* xa, float2* xb) {
    const float h = 0.5f;
    *xa = make_float2((z.x + m.x) * h, (z.y - m.y) * h);
    *xb = make_float2((z.y + m.y) * h, (m.x - z.x) * h);
}

// What a row stores of bin x: |x| (MODE 1), |x|^2 (MODE 3), else x itself
template <int MODE>
__device__ __forceinline__ auto row_value(float2 x) {
    if constexpr (MODE == 1)
        return __builtin_amdgcn_sqrtf(__builtin_fmaf(x.x, x.x, x.y * x.y));
    else if constexpr (MODE == 3)
        return __builtin_fmaf(x.x, x.x, x.y * x.y);
    else
        return x;
}
// A row's bin n - e from its bin e (real frames): X[n-e] = conj X[e], |X[n-e]| = |X[e]|
__device__ __forceinline__ float2 row_mirror(float2 x) { return cconj(x); }
__device__ __forceinline__ float row_mirror(float x) { return x; }
template <int MODE>
using RowValue = decltype(row_value<MODE>(float2{}));

// Bin e <= n of a real row of length 2n from Z, the n-point transform of its
// even/odd pairs (MODE 5): X[k] = (Z[k] + conj Z[n-k])/2 + W_2n^k (-i (Z[k] - conj Z[n-k])/2)
// with tw[k] = W_2n^k.  Im X[n] (the row's Nyquist bin) = 0 exactly, as the
// reference (fft_kiss.c:140-145); W_2n^n rounded from double is not exactly -1 + 0i.
__device__ __forceinline__ float2 r2c_split_bin(const float2* Z, int e, int n, const float2* tw, float scale) {
    const float2 A = Z[e < n ? e : 0], B = cconj(Z[e == 0 || e == n ? 0 : n - e]);
    const float2 X = split_fwd(A, B, tw[e]);
    return make_float2(X.x * scale, e == n ? 0.0f : X.y * scale);
}

// A c2c bin, scaled, and conjugated back for the inverse: sx = scale, sy = scale *
// isign (isign -1 for the inverse).  nyq: the Nyquist bin of a real row (MODE 4),
// Im = 0 exactly, as the reference's R2C (fft_kiss.c:140-145).
__device__ __forceinline__ float2 c2c_bin(float2 x, float sx, float sy, bool nyq = false) {
    return make_float2(x.x * sx, nyq ? 0.0f : x.y * sy);
}

}  // namespace vvh
