// fourstep_fft.hip -- power-of-two C2C transforms longer than one workgroup's
// register/LDS FFT (n > 4096, up to 2^24).
//
// The reference computes every power of two with one radix-2 DIT
// (src/spectral/fft_kiss.c:27-74).  Here n = N1*N2:
// n <= 2^20 (N1, N2 <= 1024): the two kernels of fourstep.hpp, two HBM passes.
//   Batches are processed in chunks whose intermediate fits the 256 MiB
//   Infinity Cache, so the rows pass reads the columns pass's output on-die.
// n > 2^20: transpose -> N1-pt FFTs -> twiddled transpose -> N2-pt FFTs ->
//   transpose (five passes of 8n bytes each way).
// The backward 1/n is applied once, in the last pass.
#include "fourstep.hpp"
#include "pow2_launch.hpp"

namespace vvh {

// ---------------------------------------------------------------------------
// Two-pass four-step
// ---------------------------------------------------------------------------
namespace {
// One pass over `batch` transforms: PASS 0 the columns (N = N1, other = N2),
// PASS 1 the rows (N = N2, other = N1); split / lo_bits feed the columns pass,
// scale the rows pass.
struct FsPass {
    const float2* in;
    float2* out;
    int other;
    long long batch;
    const float2* split;
    int lo_bits;
    float scale;
};

template <int PASS, int N, int G, bool RI, bool FWD>
hipError_t fs_launch(const FsPass& a, const FsHooks& hk, hipStream_t s) {
    const Pow2Tables tb(N);
    if (!tb.ok()) return hipErrorOutOfMemory;
    const int per = a.other / G;   // workgroups per transform
    const long long blocks = (long long)per * a.batch;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), wg(FsGeo<N, G, RI>::THREADS);
    if constexpr (PASS == 0)
        hipLaunchKernelGGL((k_fs_cols<N, G, RI, FWD>), grid, wg, 0, s, a.in, a.out, a.other, per, tb.pass, tb.tab,
                           a.split, a.lo_bits, hk);
    else
        hipLaunchKernelGGL((k_fs_rows<N, G, RI, FWD>), grid, wg, 0, s, a.in, a.out, a.other, per, tb.pass, tb.tab,
                           a.scale, hk);
    return hipGetLastError();
}

// variant (knob FS_VAR): 0 = RI exchange, G 16; 1 = float2 exchange, G 16 (default: fastest measured,
// profiles/r01_kbench_fourstep.jsonl); 2 = float2, G 8; 3 = RI, G 8
template <int PASS>
hipError_t fs_pass(int N, int var, int fwd, const FsPass& a, const FsHooks& hk, hipStream_t s) {
    return pow2_dispatch<64, 1024>(N, [&](auto nn) {
        constexpr int NN = decltype(nn)::value;
        auto dir = [&](auto g, auto ri) {
            constexpr int G = decltype(g)::value;
            constexpr bool RI = decltype(ri)::value;
            return fwd ? fs_launch<PASS, NN, G, RI, true>(a, hk, s) : fs_launch<PASS, NN, G, RI, false>(a, hk, s);
        };
        using G16 = std::integral_constant<int, 16>;
        using G8 = std::integral_constant<int, 8>;
        switch (var) {
            case 1: return dir(G16{}, std::false_type{});
            case 2: return dir(G8{}, std::false_type{});
            case 3: return dir(G8{}, std::true_type{});
            default: return dir(G16{}, std::true_type{});
        }
    });
}
}  // namespace

// n = N1*N2, 64 <= N1 <= N2 <= 1024 (fourstep_chain.hpp)
hipError_t twopass_chain(long long n, int lg, int fwd, const float2* in, float2* out, long long batch, hipStream_t s,
                         FsHooks hk) {
    const int N1 = 1 << (lg / 2), N2 = (int)(n / N1);
    int lo_bits = 0;
    const float2* split = twiddle_split(n, &lo_bits);
    if (!split) return hipErrorOutOfMemory;
    const int var = (int)knob(KNOB_FS_VAR, 1);
    // chunk of transforms whose intermediate stays in the Infinity Cache
    const long long chunk_bytes = knob(KNOB_FS_CHUNK_MB, 0) << 20;
    long long chunk = chunk_bytes > 0 ? chunk_bytes / (8 * n) : batch;
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    float2* y = nullptr;
    hipError_t e = hipMallocAsync((void**)&y, sizeof(float2) * (size_t)n * (size_t)chunk, s);
    if (e != hipSuccess) return e;
    const float scale = 1.0f / (float)n;
    for (long long c = 0; c < batch && e == hipSuccess; c += chunk) {
        const long long nb = batch - c < chunk ? batch - c : chunk;
        const float2* src = hk.pre_chirp ? nullptr : in + c * n;
        float2* dst = hk.post_chirp ? nullptr : out + c * n;
        hk.b0 = c;
        e = fs_pass<0>(N1, var, fwd, FsPass{src, y, N2, nb, split, lo_bits, scale}, hk, s);
        if (e == hipSuccess) e = fs_pass<1>(N2, var, fwd, FsPass{y, dst, N1, nb, split, lo_bits, scale}, hk, s);
    }
    (void)hipFreeAsync(y, s);
    return e;
}

// ---------------------------------------------------------------------------
// Five-pass four-step (n > 2^20)
// ---------------------------------------------------------------------------

constexpr int TT = 64;   // transpose tile

// out_b[c][r] = in_b[r][c] (* W_n^(+-r*c) when TW), matrices R x C, batch-major.
template <bool TW>
__global__ void __launch_bounds__(256)
k_transpose(const float2* __restrict__ in, float2* __restrict__ out, long long R, long long C, long long tiles_c,
            long long tiles_per_mat, const float2* __restrict__ tw, int lo_bits, long long nlo, int fwd) {
    __shared__ float2 tile[TT][TT + 1];
    const long long b = blockIdx.x / tiles_per_mat, tt = blockIdx.x % tiles_per_mat;
    const long long r0 = (tt / tiles_c) * TT, c0 = (tt % tiles_c) * TT;
    const float2* src = in + b * R * C;
    float2* dst = out + b * R * C;
    const int tx = threadIdx.x % TT, ty = threadIdx.x / TT;
    for (int i = ty; i < TT; i += 256 / TT) {
        const long long r = r0 + i, c = c0 + tx;
        if (r < R && c < C) tile[i][tx] = src[r * C + c];
    }
    __syncthreads();
    for (int i = ty; i < TT; i += 256 / TT) {
        const long long c = c0 + i, r = r0 + tx;
        if (r < R && c < C) {
            float2 v = tile[tx][i];
            if constexpr (TW) {
                const long long k = r * c;   // < n: r < N2, c < N1
                float2 w = cmul(tw[k & (nlo - 1)], tw[nlo + (k >> lo_bits)]);
                if (!fwd) w.y = -w.y;
                v = cmul(v, w);
            }
            dst[c * R + r] = v;
        }
    }
}

static hipError_t transpose(const float2* in, float2* out, long long R, long long C, long long batch, bool tw,
                            const float2* tab, int lo_bits, int fwd, hipStream_t s) {
    const long long tc = (C + TT - 1) / TT, tr = (R + TT - 1) / TT, per = tc * tr;
    const long long blocks = per * batch;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const long long nlo = 1LL << lo_bits;
    if (tw)
        hipLaunchKernelGGL(k_transpose<true>, dim3((unsigned)blocks), dim3(256), 0, s, in, out, R, C, tc, per, tab,
                           lo_bits, nlo, fwd);
    else
        hipLaunchKernelGGL(k_transpose<false>, dim3((unsigned)blocks), dim3(256), 0, s, in, out, R, C, tc, per,
                           tab, lo_bits, nlo, fwd);
    return hipGetLastError();
}

bool c2c_large_supported(long long n) { return n > 4096 && n <= (1LL << 24) && (n & (n - 1)) == 0; }

hipError_t launch_c2c_large(long long n, int fwd, const float2* in, float2* out, long long batch, hipStream_t s) {
    if (!c2c_large_supported(n)) return hipErrorInvalidValue;
    if (batch <= 0) return hipSuccess;
    if (c2c_supported(n))   // 8192: one pass in LDS (fft_c2c.hip)
        return launch_c2c(n, fwd, in, out, batch, n, n, 1.0f / (float)n, s);
    int lg = 0;
    while ((1LL << lg) < n) ++lg;
    if (lg <= 20 && knob(KNOB_FS_OLD, 0) == 0) return twopass_chain(n, lg, fwd, in, out, batch, s, FsHooks{});
    const long long N1 = 1LL << (lg / 2), N2 = n / N1;   // N1 <= N2 <= 4096
    int lo_bits = 0;
    const float2* tab = twiddle_split(n, &lo_bits);
    if (!tab) return hipErrorOutOfMemory;
    float2 *s1 = nullptr, *s2 = nullptr;
    const size_t bytes = sizeof(float2) * (size_t)n * (size_t)batch;
    hipError_t e = hipMallocAsync((void**)&s1, bytes, s);
    if (e != hipSuccess) return e;
    e = hipMallocAsync((void**)&s2, bytes, s);
    if (e != hipSuccess) {
        (void)hipFreeAsync(s1, s);
        return e;
    }
    do {
        if ((e = transpose(in, s1, N1, N2, batch, false, tab, lo_bits, fwd, s)) != hipSuccess) break;
        if ((e = launch_c2c(N1, fwd, s1, s2, batch * N2, N1, N1, 1.0f / (float)N1, s)) != hipSuccess) break;
        if ((e = transpose(s2, s1, N2, N1, batch, true, tab, lo_bits, fwd, s)) != hipSuccess) break;
        if ((e = launch_c2c(N2, fwd, s1, s2, batch * N1, N2, N2, 1.0f / (float)N2, s)) != hipSuccess) break;
        e = transpose(s2, out, N1, N2, batch, false, tab, lo_bits, fwd, s);
    } while (false);
    (void)hipFreeAsync(s1, s);
    (void)hipFreeAsync(s2, s);
    return e;
}

}  // namespace vvh
