// shim_analytic.hip -- Hilbert / analytic signal, instantaneous phase and
// frequency (hilbert.c), and the DCT (dct.c) over analytic_kernels.hip,
// phase_kernels.hip and spectral_kernels.hip.
#include "shim_common.hpp"

using namespace vvh;

// Instantaneous phase / frequency (hilbert.c:77-113)
static constexpr double kTwoPiD = 2.0 * 3.141592653589793238462643383279502884;   // 2 * VV_DSP_PI_D

// *out_written: whether d_out was written (the ERROR policy stops at a NaN/Inf
// input before anything is written, as dct.c:96-100 returns before the output)
static int dct_run(const float* d_in, float* d_out, size_t n, size_t batch, int type, int dir, int nan_policy,
                   hipStream_t s, bool* out_written) {
    *out_written = false;
    if (!d_in || !d_out) return ST_NULL;
    if (n == 0) return ST_SIZE;
    if ((type != 2 && type != 3 && type != 4) || (dir != 1 && dir != -1)) return ST_RANGE;
    const long long N = (long long)n, B = (long long)batch;
    if (type == 2 && dir > 0 && nan_policy != 2 && dct2_fused_supported(N)) {   // one pass, policy on read
        HIPCHK(launch_dct2_fused(N, d_in, d_out, B, nan_policy, s), ST_INTERNAL);
        *out_written = true;
        return ST_OK;
    }
    Scratch xin(s), flag(s), v(s), V(s);
    HIPCHK(xin.alloc(sizeof(float) * n * batch), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(xin.p, d_in, sizeof(float) * n * batch, hipMemcpyDeviceToDevice, s), ST_INTERNAL);
    int* dflag = nullptr;
    if (nan_policy == 2) {
        HIPCHK(flag.alloc(sizeof(int)), ST_INTERNAL);
        dflag = (int*)flag.p;
        HIPCHK(hipMemsetAsync(dflag, 0, sizeof(int), s), ST_INTERNAL);
    }
    HIPCHK(launch_nan_policy((float*)xin.p, N * B, nan_policy, dflag, s), ST_INTERNAL);
    if (nan_policy == 2) {
        int h = 0;
        HIPCHK(hipMemcpyAsync(&h, dflag, sizeof(int), hipMemcpyDeviceToHost, s), ST_INTERNAL);
        HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
        if (h) return ST_NAN;
    }
    // Makhoul re-ordering + a real FFT: power-of-two n, and even 7-smooth n
    // through the mixed-radix kernels (odd n would need the other permutation)
    const bool fast = (is_pow2(n) && n >= 4 && n <= 16384) || (n % 2 == 0 && n >= 4 && use_mixed(N));
    if (fast && type == 2 && dir > 0) {
        const float2* tw4n = twiddle_table((int)(4 * n));
        if (!tw4n) return fail(ST_INTERNAL, "dct twiddles");
        HIPCHK(v.alloc(sizeof(float) * n * batch), ST_INTERNAL);
        HIPCHK(V.alloc(8 * (n / 2 + 1) * batch), ST_INTERNAL);
        HIPCHK(launch_dct2_pre(N, (const float*)xin.p, (float*)v.p, B, s), ST_INTERNAL);
        int st = fft_run(n, 1, 1, v.p, V.p, batch, s);
        if (st) return st;
        HIPCHK(launch_dct2_post(N, (const float2*)V.p, d_out, B, tw4n, s), ST_INTERNAL);
    } else if (fast && (type == 2 || type == 3) && dir < 0) {
        const float2* tw4n = twiddle_table((int)(4 * n));
        if (!tw4n) return fail(ST_INTERNAL, "dct twiddles");
        HIPCHK(v.alloc(sizeof(float) * n * batch), ST_INTERNAL);
        HIPCHK(V.alloc(8 * (n / 2 + 1) * batch), ST_INTERNAL);
        HIPCHK(launch_dct3_pre(N, (const float*)xin.p, (float2*)V.p, B, tw4n, s), ST_INTERNAL);
        int st = fft_run(n, 2, -1, V.p, v.p, batch, s);
        if (st) return st;
        HIPCHK(launch_dct3_post(N, (const float*)v.p, d_out, B, 1.0f, s), ST_INTERNAL);
    } else {
        HIPCHK(launch_dct_naive(N, type, dir, (const float*)xin.p, d_out, B, s), ST_INTERNAL);
    }
    *out_written = true;
    if (nan_policy != 0) {
        if (nan_policy == 2) HIPCHK(hipMemsetAsync(dflag, 0, sizeof(int), s), ST_INTERNAL);
        HIPCHK(launch_nan_policy(d_out, N * B, nan_policy, dflag, s), ST_INTERNAL);
        if (nan_policy == 2) {
            int h = 0;
            HIPCHK(hipMemcpyAsync(&h, dflag, sizeof(int), hipMemcpyDeviceToHost, s), ST_INTERNAL);
            HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
            if (h) return ST_NAN;
        }
    }
    return ST_OK;
}

extern "C" {

// ---------------------------------------------------------------------------
// Hilbert
// ---------------------------------------------------------------------------
int vvhip_hilbert_device(const float* d_x, size_t n, size_t batch, float* d_z, void* stream) {
    if (!d_x || !d_z) return ST_NULL;
    if (n == 0) return ST_SIZE;
    hipStream_t s = (hipStream_t)stream;
    if (hilbert_fused_supported((long long)n)) {   // one pass: rows in, analytic rows out
        HIPCHK(launch_hilbert_fused((long long)n, d_x, (float2*)d_z, (long long)batch, s), ST_INTERNAL);
        return ST_OK;
    }
    const size_t nh = n / 2 + 1;
    Scratch half(s);
    HIPCHK(half.alloc(8 * nh * batch), ST_INTERNAL);
    int st = fft_run(n, 1, 1, d_x, half.p, batch, s);
    if (st) return st;
    // mask straight into the output buffer, then inverse C2C in place
    HIPCHK(launch_hilbert_mask((long long)n, (const float2*)half.p, (float2*)d_z, (long long)batch, (long long)nh, s),
           ST_INTERNAL);
    return fft_run(n, 0, -1, d_z, d_z, batch, s);
}

int vvhip_hilbert_host(const float* x, size_t n, float* z_out) {
    if (!x || !z_out) return ST_NULL;
    if (n == 0) return ST_SIZE;
    HostCall c("hilbert");
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    float* dz = (float*)c.out(z_out, 8 * n);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_hilbert_device(dx, n, 1, dz, c.s));
}

int vvhip_inst_phase_device(const float* d_z, size_t n, size_t batch, float* d_phase, void* stream) {
    if (!d_z || !d_phase) return ST_NULL;
    if (n == 0) return ST_SIZE;
    if (batch == 0) return ST_OK;
    if (batch > 65535) return fail(ST_RANGE, "instantaneous phase: more than 65535 rows per call");
    HIPCHK(launch_inst_phase((const float2*)d_z, (long long)n, (long long)batch, d_phase, (hipStream_t)stream),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_inst_freq_device(const float* d_phase, size_t n, size_t batch, double fs, float* d_freq, void* stream) {
    if (!d_phase || !d_freq) return ST_NULL;
    if (n == 0) return ST_SIZE;
    if (batch == 0) return ST_OK;
    hipStream_t s = (hipStream_t)stream;
    Scratch tmp(s);
    if (d_phase == d_freq) {   // f[i] needs p[i-1], which a neighbouring thread overwrites: read a copy
        HIPCHK(tmp.alloc(4 * n * batch), ST_INTERNAL);
        HIPCHK(hipMemcpyAsync(tmp.p, d_phase, 4 * n * batch, hipMemcpyDeviceToDevice, s), ST_INTERNAL);
        d_phase = (const float*)tmp.p;
    }
    HIPCHK(launch_inst_freq(d_phase, (long long)n, (long long)batch, fs / kTwoPiD, d_freq, s), ST_INTERNAL);
    return ST_OK;
}

int vvhip_inst_phase_host(const float* z, size_t n, float* phase) {
    if (!z || !phase) return ST_NULL;
    if (n == 0) return ST_SIZE;
    HostCall c("instantaneous phase");
    const float* dz = (const float*)c.in(z, 8 * n);
    float* dp = (float*)c.out(phase, sizeof(float) * n);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_inst_phase_device(dz, n, 1, dp, c.s));
}

int vvhip_inst_freq_host(const float* phase, size_t n, double fs, float* freq) {
    if (!phase || !freq) return ST_NULL;
    if (n == 0) return ST_SIZE;
    HostCall c("instantaneous frequency");
    const float* dp = (const float*)c.in(phase, sizeof(float) * n);
    float* df = (float*)c.out(freq, sizeof(float) * n);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_inst_freq_device(dp, n, 1, fs, df, c.s));
}

// ---------------------------------------------------------------------------
// DCT
// ---------------------------------------------------------------------------
int vvhip_dct_device(const float* d_in, float* d_out, size_t n, size_t batch, int type, int dir,
                     int nan_policy, void* stream) {
    bool wrote = false;
    return dct_run(d_in, d_out, n, batch, type, dir, nan_policy, (hipStream_t)stream, &wrote);
}

int vvhip_dct_host(const float* in, float* out, size_t n, int type, int dir, int nan_policy) {
    if (!in || !out) return ST_NULL;
    if (n == 0) return ST_SIZE;
    HostCall c("dct");
    const float* di = (const float*)c.in(in, sizeof(float) * n);
    float* dout = (float*)c.out(out, sizeof(float) * n);
    if (!c.ok()) return c.st;
    bool wrote = false;
    const int st = dct_run(di, dout, n, 1, type, dir, nan_policy, c.s, &wrote);
    // the reference writes the output buffer even when the OUTPUT check fails
    // (dct.c:128-131), and leaves it untouched when the input check does (:96-100)
    return c.finish(st, wrote && (st == ST_OK || st == ST_NAN));
}

}  // extern "C"
