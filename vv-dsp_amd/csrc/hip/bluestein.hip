// bluestein.hip -- Bluestein (chirp-z) for non-power-of-two n: O(M log M), M = pow2 >= 2n-1.
// With a[m] = exp(-+i*pi*m^2/n) (sign of the transform), n*k = (n^2 + k^2 -
// (k-n)^2)/2 gives X[k] = a[k] * sum_j (x[j] a[j]) conj(a[k-j]): a length-M
// circular convolution of u = x*a (zero padded) with v[m] = conj(a[m]) for
// |m| < n, done as IFFT(FFT(u) * V) with V = FFT(v) cached per (n, sign).
// The reference computes these lengths with an O(n^2) f32 DFT
// (src/spectral/fft_kiss.c:76-92); this path replaces it above
// BLUESTEIN_MIN, where it is both faster and closer to f64.
#include "fft_core.hpp"
#include "fourstep_chain.hpp"
#include "vvhip_internal.hpp"

#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace vvh {

namespace {
struct ChirpPlan {
    long long M;
    float2* chirp;   // a[m], m < n
    float2* V;       // FFT_M(v)
};
std::mutex g_bmu;
std::map<std::tuple<int, long long, int>, ChirpPlan> g_bplans;   // (device, n, fwd)

long long pow2_ge(long long x) {
    long long m = 1;
    while (m < x) m <<= 1;
    return m;
}

hipError_t fft_pow2(long long m, int fwd, const float2* in, float2* out, long long batch, hipStream_t s) {
    if (c2c_supported(m)) return launch_c2c(m, fwd, in, out, batch, m, m, 1.0f / (float)m, s);
    return launch_c2c_large(m, fwd, in, out, batch, s);
}

__global__ void k_chirp_v(const float2* __restrict__ a, float2* __restrict__ v, long long n, long long M) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float2 r = make_float2(0.0f, 0.0f);
    if (m < n) r = a[m];
    else if (m > M - n) r = a[M - m];
    v[m] = make_float2(r.x, -r.y);   // conj(a[|m|])
}

const ChirpPlan* chirp_plan(long long n, int fwd, hipStream_t s) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const auto key = std::make_tuple(dev, n, fwd);
    std::lock_guard<std::mutex> lk(g_bmu);
    auto it = g_bplans.find(key);
    if (it != g_bplans.end()) return &it->second;
    ChirpPlan p{pow2_ge(2 * n - 1), nullptr, nullptr};
    if (p.M > (1LL << 24)) return nullptr;
    // a[m] = exp(-+i*pi*(m^2 mod 2n)/n), reduced exactly in integers, rounded from double
    std::vector<float2> h((size_t)n);
    for (long long m = 0; m < n; ++m) {
        const long long q = (long long)(((unsigned __int128)m * (unsigned __int128)m) % (unsigned __int128)(2 * n));
        const double ang = (fwd ? -M_PI : M_PI) * (double)q / (double)n;
        h[(size_t)m] = make_float2((float)std::cos(ang), (float)std::sin(ang));
    }
    float2* v = nullptr;
    bool ok = hipMalloc(&p.chirp, sizeof(float2) * n) == hipSuccess &&
              hipMalloc(&p.V, sizeof(float2) * p.M) == hipSuccess && hipMalloc(&v, sizeof(float2) * p.M) == hipSuccess &&
              hipMemcpyAsync(p.chirp, h.data(), sizeof(float2) * n, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_chirp_v, dim3((unsigned)((p.M + 255) / 256)), dim3(256), 0, s, p.chirp, v, n, p.M);
        ok = hipGetLastError() == hipSuccess && fft_pow2(p.M, 1, v, p.V, 1, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    }
    if (v) (void)hipFree(v);
    if (!ok) {
        if (p.chirp) (void)hipFree(p.chirp);
        if (p.V) (void)hipFree(p.V);
        return nullptr;
    }
    return &(g_bplans[key] = p);
}
}  // namespace

bool bluestein_supported(long long n) { return n >= 2 && pow2_ge(2 * n - 1) <= (1LL << 24); }

hipError_t launch_bluestein(long long n, int fwd, const void* in, int real_in, float2* out, long long nout,
                            long long batch, long long in_dist, long long out_dist, float scale, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    const ChirpPlan* p = chirp_plan(n, fwd, s);
    if (!p) return hipErrorOutOfMemory;
    const long long M = p->M, total = M * batch;
    const int lgM = ilog2((int)(M < (1LL << 30) ? M : (1LL << 30)));
    if (!c2c_supported(M) && lgM <= 20 && knob(KNOB_FS_OLD, 0) == 0 && knob(KNOB_BLUE_UNFUSED, 0) == 0) {
        // two-pass M (8192..2^20): chirp pre-multiply and zero padding in the forward
        // columns pass, the product with V in its rows pass, and the post-multiply,
        // scale and truncation to nout in the inverse rows pass -- four kernels,
        // no u / padded-input pass and no full-length output pass
        float2* U = nullptr;
        hipError_t e = hipMallocAsync((void**)&U, sizeof(float2) * total, s);
        if (e != hipSuccess) return e;
        FsHooks f;
        f.pre_chirp = p->chirp;
        f.raw = in;
        f.in_dist = in_dist;
        f.nsig = n;
        f.real_in = real_in;
        f.mulv = p->V;
        e = twopass_chain(M, lgM, 1, nullptr, U, batch, s, f);
        if (e == hipSuccess) {
            FsHooks b;
            b.post_chirp = p->chirp;
            b.post_out = out;
            b.out_dist = out_dist;
            b.nout = nout;
            b.post_scale = scale;
            e = twopass_chain(M, lgM, 0, U, nullptr, batch, s, b);
        }
        (void)hipFreeAsync(U, s);
        return e;
    }
    float2 *u = nullptr, *U = nullptr;
    hipError_t e = hipMallocAsync((void**)&u, sizeof(float2) * total, s);
    if (e != hipSuccess) return e;
    e = hipMallocAsync((void**)&U, sizeof(float2) * total, s);
    if (e != hipSuccess) {
        (void)hipFreeAsync(u, s);
        return e;
    }
    do {
        if ((e = launch_chirp_pre(in, real_in, n, M, batch, in_dist, p->chirp, u, s)) != hipSuccess) break;
        if ((e = fft_pow2(M, 1, u, U, batch, s)) != hipSuccess) break;
        if ((e = launch_cmul_rows(U, p->V, M, batch, s)) != hipSuccess) break;
        if ((e = fft_pow2(M, 0, U, u, batch, s)) != hipSuccess) break;   // includes 1/M
        e = launch_chirp_post_scaled(u, 0, M, nout, batch, p->chirp, out, out_dist, scale, s);
    } while (false);
    (void)hipFreeAsync(u, s);
    (void)hipFreeAsync(U, s);
    return e;
}

}  // namespace vvh
