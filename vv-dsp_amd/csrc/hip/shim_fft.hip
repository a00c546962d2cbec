// shim_fft.hip -- the FFT dispatch over the kernel launchers (fft_run, which
// every other shim module transforms through) and the FFT plans: own stream,
// lazily grown host-path staging buffers.
#include "shim_common.hpp"

using namespace vvh;

struct vvhip_fft {
    size_t n = 0;
    int type = 0;   // 0 C2C 1 R2C 2 C2R
    int dir = 1;
    size_t batch = 1;
    HostStage host;
    DevBuf din, dout;
};

static size_t fft_in_elems_bytes(const vvhip_fft* p) {
    switch (p->type) {
        case 0: return p->n * 8;
        case 1: return p->n * 4;
        default: return (p->n / 2 + 1) * 8;
    }
}
static size_t fft_out_elems_bytes(const vvhip_fft* p) {
    switch (p->type) {
        case 0: return p->n * 8;
        case 1: return (p->n / 2 + 1) * 8;
        default: return p->n * 4;
    }
}

namespace vvh {

bool use_mixed(long long n) { return knob(KNOB_NO_MIXED, 0) != 1 && mixed_supported(n); }
hipError_t dft_any(long long n, int fwd, const void* in, int real_in, float2* out, long long nout, long long batch,
                   long long in_dist, long long out_dist, float scale, hipStream_t s) {
    if (use_mixed(n))
        return launch_fft_mixed(n, fwd, in, real_in, out, nout, batch, in_dist, out_dist, scale, s);
    if (n >= BLUESTEIN_MIN && bluestein_supported(n))
        return launch_bluestein(n, fwd, in, real_in, out, nout, batch, in_dist, out_dist, scale, s);
    return launch_dft_naive(n, fwd, in, real_in, out, nout, batch, in_dist, out_dist, scale, s);
}

int fft_run(size_t n, int type, int dir, const void* in, void* out, size_t batch, hipStream_t s) {
    const long long N = (long long)n, B = (long long)batch;
    if (B == 0) return ST_OK;
    const int fwd = dir > 0;
    if (type == 0) {
        if (c2c_supported(N)) {
            HIPCHK(launch_c2c(N, fwd, (const float2*)in, (float2*)out, B, N, N, 1.0f / (float)N, s), ST_INTERNAL);
            return ST_OK;
        }
        if (n == 1) {
            if (in != out) HIPCHK(hipMemcpyAsync(out, in, 8 * batch, hipMemcpyDeviceToDevice, s), ST_INTERNAL);
            return ST_OK;
        }
        if (is_pow2(n)) {
            if (!c2c_large_supported(N)) return fail(ST_UNSUP, "C2C power-of-two length > 2^24 not supported");
            HIPCHK(launch_c2c_large(N, fwd, (const float2*)in, (float2*)out, B, s), ST_INTERNAL);
            return ST_OK;
        }
        const void* src = in;
        Scratch tmp(s);
        if (in == out && !use_mixed(N)) {   // the mixed-radix kernel reads a transform whole before writing it
            HIPCHK(tmp.alloc(8 * n * batch), ST_INTERNAL);
            HIPCHK(hipMemcpyAsync(tmp.p, in, 8 * n * batch, hipMemcpyDeviceToDevice, s), ST_INTERNAL);
            src = tmp.p;
        }
        HIPCHK(dft_any(N, fwd, src, 0, (float2*)out, N, B, N, N, fwd ? 1.0f : 1.0f / (float)N, s),
               ST_INTERNAL);
        return ST_OK;
    }
    const long long NH = N / 2 + 1;
    if (type == 1) {   // R2C: real[n] -> cpx[n/2+1]
        if (r2c_supported(N)) {
            HIPCHK(launch_r2c(N, (const float*)in, (float2*)out, B, N, NH, s), ST_INTERNAL);
            return ST_OK;
        }
        if (is_pow2(n) && n > 8192 && c2c_large_supported(N / 2) && knob(KNOB_REAL_PROMOTE, 0) != 1) {
            // the n/2-point C2C of the rows as complex pairs, then the split step
            Scratch Z(s);
            HIPCHK(Z.alloc(8 * (n / 2) * batch), ST_INTERNAL);
            HIPCHK(launch_c2c_large(N / 2, 1, (const float2*)in, (float2*)Z.p, B, s), ST_INTERNAL);
            HIPCHK(launch_real_split_fwd((const float2*)Z.p, (float2*)out, N / 2, B, s), ST_INTERNAL);
            return ST_OK;
        }
        if (is_pow2(n) && n > 8192) {   // promote, four-step C2C, keep bins 0..n/2 (fft_kiss.c:120-147)
            if (!c2c_large_supported(N)) return fail(ST_UNSUP, "R2C power-of-two length > 2^24 not supported");
            Scratch z(s), Z(s);
            HIPCHK(z.alloc(8 * n * batch), ST_INTERNAL);
            HIPCHK(Z.alloc(8 * n * batch), ST_INTERNAL);
            HIPCHK(launch_promote_real((const float*)in, (float2*)z.p, N * B, s), ST_INTERNAL);
            HIPCHK(launch_c2c_large(N, 1, (const float2*)z.p, (float2*)Z.p, B, s), ST_INTERNAL);
            HIPCHK(hipMemcpy2DAsync(out, 8 * NH, Z.p, 8 * n, 8 * NH, batch, hipMemcpyDeviceToDevice, s), ST_INTERNAL);
            HIPCHK(launch_zero_nyquist_imag((float2*)out, N, B, NH, s), ST_INTERNAL);
            return ST_OK;
        }
        HIPCHK(dft_any(N, 1, in, 1, (float2*)out, NH, B, N, NH, 1.0f, s), ST_INTERNAL);
        // the single-pass mixed-radix kernels store Im X[n/2] = 0 themselves;
        // the f64 DFT, Bluestein and four-step paths get it here
        if (!(use_mixed(N) && stft_mixed_supported(N)))
            HIPCHK(launch_zero_nyquist_imag((float2*)out, N, B, NH, s), ST_INTERNAL);
        return ST_OK;
    }
    // C2R: cpx[n/2+1] -> real[n]
    if (r2c_supported(N)) {
        HIPCHK(launch_c2r(N, (const float2*)in, (float*)out, B, NH, N, s), ST_INTERNAL);
        return ST_OK;
    }
    if (is_pow2(n) && n > 8192 && c2c_large_supported(N / 2) && knob(KNOB_REAL_PROMOTE, 0) != 1) {
        // inverse split step, then the n/2-point inverse C2C straight into the real rows
        Scratch V(s);
        HIPCHK(V.alloc(8 * (n / 2) * batch), ST_INTERNAL);
        HIPCHK(launch_real_split_inv((const float2*)in, (float2*)V.p, N / 2, B, s), ST_INTERNAL);
        HIPCHK(launch_c2c_large(N / 2, 0, (const float2*)V.p, (float2*)out, B, s), ST_INTERNAL);
        return ST_OK;
    }
    if (is_pow2(n) && n > 8192 && !c2c_large_supported(N))
        return fail(ST_UNSUP, "C2R power-of-two length > 2^24 not supported");
    Scratch full(s), tim(s);
    HIPCHK(full.alloc(8 * n * batch), ST_INTERNAL);
    HIPCHK(tim.alloc(8 * n * batch), ST_INTERNAL);
    HIPCHK(launch_hermitian_expand(N, (const float2*)in, (float2*)full.p, B, NH, 0, s), ST_INTERNAL);
    if (is_pow2(n) && n > 8192)   // Hermitian expand (fft_kiss.c:149-174), four-step inverse
        HIPCHK(launch_c2c_large(N, 0, (const float2*)full.p, (float2*)tim.p, B, s), ST_INTERNAL);
    else
        HIPCHK(dft_any(N, 0, full.p, 0, (float2*)tim.p, N, B, N, N, 1.0f / (float)N, s), ST_INTERNAL);
    HIPCHK(launch_take_real((const float2*)tim.p, (float*)out, N * B, s), ST_INTERNAL);
    return ST_OK;
}

}  // namespace vvh

extern "C" {

int vvhip_fft_plan_create(size_t n, int type, int dir, size_t batch, vvhip_fft** out) {
    if (!out) return ST_NULL;
    *out = nullptr;
    if (n == 0 || batch == 0) return ST_SIZE;
    if (type < 0 || type > 2 || (dir != 1 && dir != -1)) return ST_RANGE;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (is_pow2(n) && n > (1u << 24)) return fail(ST_UNSUP, "power-of-two length > 2^24 not supported");
    vvhip_fft* p = new (std::nothrow) vvhip_fft;
    if (!p) return ST_INTERNAL;
    p->n = n;
    p->type = type;
    p->dir = dir;
    p->batch = batch;
    *out = p;
    return ST_OK;
}

int vvhip_fft_exec_device(vvhip_fft* p, const void* d_in, void* d_out, size_t batch, void* stream) {
    if (!p || !d_in || !d_out) return ST_NULL;
    return fft_run(p->n, p->type, p->dir, d_in, d_out, batch ? batch : p->batch, (hipStream_t)stream);
}

int vvhip_fft_exec_host(vvhip_fft* p, const void* in, void* out) {
    if (!p || !in || !out) return ST_NULL;
    std::lock_guard<std::mutex> host_lock(p->host.mu);
    const size_t ie = fft_in_elems_bytes(p), oe = fft_out_elems_bytes(p);
    const size_t chunk_b = host_chunk_bytes();
    if ((ie + oe) * p->batch >= 2 * chunk_b && p->batch >= 2) {
        // pipelined: chunks of whole transforms on two lanes
        size_t per = chunk_b / (ie > oe ? ie : oe);
        if (per < 1) per = 1;
        const long long nchunks = (long long)((p->batch + per - 1) / per);
        return run_lanes(p->host.lanes, nchunks, [&](long long c, HostLane& L) -> int {
            const size_t b0 = (size_t)c * per, nb = (p->batch - b0) < per ? (p->batch - b0) : per;
            HIPCHK(L.a.ensure(ie * per), ST_INTERNAL);
            HIPCHK(L.b.ensure(oe * per), ST_INTERNAL);
            HIPCHK(hipMemcpyAsync(L.a.p, (const char*)in + ie * b0, ie * nb, hipMemcpyHostToDevice, L.s),
                   ST_INTERNAL);
            int st = fft_run(p->n, p->type, p->dir, L.a.p, L.b.p, nb, L.s);
            if (st != ST_OK) return st;
            HIPCHK(hipMemcpyAsync((char*)out + oe * b0, L.b.p, oe * nb, hipMemcpyDeviceToHost, L.s), ST_INTERNAL);
            return ST_OK;
        });
    }
    HIPCHK(p->host.stream_or_create(), ST_INTERNAL);
    const hipStream_t s = p->host.stream;
    const size_t ib = ie * p->batch, ob = oe * p->batch;
    HIPCHK(p->din.ensure(ib), ST_INTERNAL);
    HIPCHK(p->dout.ensure(ob), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(p->din.p, in, ib, hipMemcpyHostToDevice, s), ST_INTERNAL);
    int st = fft_run(p->n, p->type, p->dir, p->din.p, p->dout.p, p->batch, s);
    if (st != ST_OK) return st;
    HIPCHK(hipMemcpyAsync(out, p->dout.p, ob, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
    return ST_OK;
}

void vvhip_fft_plan_destroy(vvhip_fft* p) {
    if (!p) return;
    p->host.release();
    p->din.release();
    p->dout.release();
    delete p;
}

}  // extern "C"
