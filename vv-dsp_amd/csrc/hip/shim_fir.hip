// shim_fir.hip -- FIR handles (device taps + per-block-size spectra H) over the
// fir_*.hip launchers: overlap-save, the long-filter four-step path, the direct
// form and filtfilt.
#include "shim_common.hpp"

using namespace vvh;

struct vvhip_fir {
    size_t taps = 0;
    float* d_h = nullptr;
    struct Spec {
        size_t nfft;
        float2* H;
    };
    std::vector<Spec> specs;   // H per overlap-save block size
    std::mutex mu;
    HostStage host;
    DevBuf bx, by, bp;
};

// Overlap-save block N (= complex FFT size of k_fir_pair): the smallest power
// of two >= max(4*(L-1), 64), so that at least 3/4 of every block is output,
// grown toward the preferred size (1024: four transforms per 256-thread
// workgroup, H and twiddles in 51 KB of LDS) while the signal is longer.
// Knob FIR_BLOCK overrides the preferred size.  0 = no OLS block (long
// filters use the direct form).
static size_t fir_block(const vvhip_fir* f, size_t n) {
    size_t pref = (size_t)knob(KNOB_FIR_BLOCK, 1024);
    if (pref < 64 || pref > 8192 || (pref & (pref - 1))) pref = 1024;
    const size_t lm1 = f->taps - 1;
    size_t nr = 64;
    while (nr < 4 * lm1 && nr < 8192) nr <<= 1;
    while (nr < pref && nr < n + lm1) nr <<= 1;
    if (nr <= lm1 || nr - lm1 < nr / 4) return 0;
    return nr;
}

// Overlap-save block for filters the fused kernels cannot take (taps > 6145):
// N = pow2 >= max(4 (L-1), 16384), at most 2^22, so >= 3/4 of a block is output.
// 0 = none (longer filters than that use the direct form).
static size_t fir_long_block(size_t taps) {
    const size_t lm1 = taps - 1;
    size_t nr = 16384;
    while (nr < 4 * lm1 && nr < ((size_t)1 << 22)) nr <<= 1;
    if (nr <= lm1 || nr - lm1 < nr / 4) return 0;
    return nr;
}

// H for block nr: FFT(h zero-padded to nr) over all nr bins, cached per nr.
// nr <= 8192 (fused kernels): scaled by 1/nr.  nr > 8192 (fir_long_block, the
// four-step path whose inverse applies 1/nr itself): unscaled.
static int fir_spectrum(vvhip_fir* f, size_t nr, const float2** H, hipStream_t s) {
    std::lock_guard<std::mutex> lk(f->mu);
    for (auto& sp : f->specs)
        if (sp.nfft == nr) {
            *H = sp.H;
            return ST_OK;
        }
    float2* Hd = nullptr;
    void* t1 = nullptr;
    void* t2 = nullptr;
    hipError_t e = hipMalloc(&Hd, sizeof(float2) * nr);
    if (nr > 8192) {   // promote h, zero pad, four-step FFT
        if (e == hipSuccess) e = hipMalloc(&t1, sizeof(float2) * nr);
        if (e == hipSuccess) e = hipMemsetAsync(t1, 0, sizeof(float2) * nr, s);
        if (e == hipSuccess) e = launch_promote_real(f->d_h, (float2*)t1, (long long)f->taps, s);
        if (e == hipSuccess) e = launch_c2c_large((long long)nr, 1, (const float2*)t1, Hd, 1, s);
    } else {           // R2C of h zero-padded, Hermitian expand, 1/nr
        if (e == hipSuccess) e = hipMalloc(&t1, sizeof(float) * nr);
        if (e == hipSuccess) e = hipMalloc(&t2, sizeof(float2) * (nr / 2 + 1));
        if (e == hipSuccess) e = hipMemsetAsync(t1, 0, sizeof(float) * nr, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(t1, f->d_h, sizeof(float) * f->taps, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = launch_r2c((long long)nr, (const float*)t1, (float2*)t2, 1, (long long)nr, (long long)(nr / 2 + 1), s);
        if (e == hipSuccess)
            e = launch_hermitian_expand((long long)nr, (const float2*)t2, Hd, 1, (long long)(nr / 2 + 1), 0, s);
        if (e == hipSuccess) e = launch_scale_cpx(Hd, (long long)nr, 1.0f / (float)nr, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (t1) (void)hipFree(t1);
    if (t2) (void)hipFree(t2);
    if (e != hipSuccess) {
        if (Hd) (void)hipFree(Hd);
        return fail(ST_INTERNAL, "fir filter spectrum", e);
    }
    f->specs.push_back({nr, Hd});
    *H = Hd;
    return ST_OK;
}

// Zero-state linear convolution (first n outputs) for long filters: overlap-save
// with N = fir_long_block(taps), two blocks per complex row, in chunks of rows
// whose two scratch buffers stay within ~512 MiB.
static int fir_ols_long(vvhip_fir* f, size_t nr, const float* d_x, float* d_y, size_t n, size_t nch,
                        size_t x_stride, size_t y_stride, hipStream_t s) {
    const float2* H = nullptr;
    if (int st = fir_spectrum(f, nr, &H, s)) return st;
    // history taps - 1 as it is (fir_long_block: at most 3/4 of N): the gather needs no aligned block starts
    const long long N = (long long)nr;
    const FirGeo g = fir_geometry(N, (long long)f->taps - 1, (long long)n);
    const long long le = g.le, lout = g.lout, ppc = g.ppc, items = ppc * (long long)nch;
    long long rows = (256LL << 20) / (8 * N);
    if (rows < 1) rows = 1;
    if (rows > items) rows = items;
    Scratch za(s), zb(s);
    HIPCHK(za.alloc(sizeof(float2) * (size_t)(rows * N)), ST_INTERNAL);
    HIPCHK(zb.alloc(sizeof(float2) * (size_t)(rows * N)), ST_INTERNAL);
    float2* A = (float2*)za.p;
    float2* B = (float2*)zb.p;
    for (long long p0 = 0; p0 < items; p0 += rows) {
        const long long r = items - p0 < rows ? items - p0 : rows;
        HIPCHK(launch_fir_long_gather(d_x, (long long)n, (long long)x_stride, N, le, lout, ppc, p0, r, A, s),
               ST_INTERNAL);
        HIPCHK(launch_c2c_large(N, 1, A, B, r, s), ST_INTERNAL);
        HIPCHK(launch_cmul_rows(B, H, N, r, s), ST_INTERNAL);
        HIPCHK(launch_c2c_large(N, 0, B, A, r, s), ST_INTERNAL);
        HIPCHK(launch_fir_long_scatter(A, d_y, (long long)n, (long long)y_stride, N, le, lout, ppc, p0, r, s),
               ST_INTERNAL);
    }
    return ST_OK;
}

extern "C" {

int vvhip_fir_create(const float* h, size_t taps, vvhip_fir** out) {
    if (!out || !h) return ST_NULL;
    *out = nullptr;
    if (taps == 0) return ST_SIZE;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    vvhip_fir* f = new (std::nothrow) vvhip_fir;
    if (!f) return ST_INTERNAL;
    f->taps = taps;
    if (hipMalloc(&f->d_h, sizeof(float) * taps) != hipSuccess ||
        hipMemcpy(f->d_h, h, sizeof(float) * taps, hipMemcpyHostToDevice) != hipSuccess) {
        vvhip_fir_destroy(f);
        return fail(ST_INTERNAL, "fir taps upload");
    }
    *out = f;
    return ST_OK;
}

void vvhip_fir_destroy(vvhip_fir* f) {
    if (!f) return;
    f->host.release();
    if (f->d_h) (void)hipFree(f->d_h);
    for (auto& sp : f->specs) (void)hipFree(sp.H);
    f->bx.release();
    f->by.release();
    f->bp.release();
    delete f;
}

size_t vvhip_fir_block_size(vvhip_fir* f, size_t n) { return f ? fir_block(f, n) : 0; }

int vvhip_fir_apply_device(vvhip_fir* f, const float* d_x, float* d_y, size_t n, size_t nch,
                           size_t x_stride, size_t y_stride, const float* d_prefix, int mode,
                           void* stream) {
    if (!f || !d_x || !d_y) return ST_NULL;
    if (n == 0 || nch == 0) return ST_OK;
    hipStream_t s = (hipStream_t)stream;
    const long long L = (long long)f->taps;
    const size_t nr = mode == 0 ? fir_block(f, n) : 0;
    if (nr) {
        const float2* H = nullptr;
        if (int st = fir_spectrum(f, nr, &H, s)) return st;
        HIPCHK(launch_fir_ols((long long)nr, L, H, d_x, d_y, (long long)n, (long long)nch, (long long)x_stride,
                              (long long)y_stride, d_prefix, s),
               ST_INTERNAL);
        return ST_OK;
    }
    if (mode == 0 && !d_prefix) {   // long zero-state filters: overlap-save over the four-step FFTs
        // (a caller-supplied history takes the direct form below, which reads it)
        const size_t nl = fir_long_block(f->taps);
        if (nl) return fir_ols_long(f, nl, d_x, d_y, n, nch, x_stride, y_stride, s);
    }
    HIPCHK(launch_fir_direct(f->d_h, L, d_x, d_y, (long long)n, (long long)nch, (long long)x_stride,
                             (long long)y_stride, d_prefix, s),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_fir_apply_host(vvhip_fir* f, const float* x, float* y, size_t n, const float* prefix, int mode) {
    if (!f || !x || !y) return ST_NULL;
    std::lock_guard<std::mutex> host_lock(f->host.mu);
    if (n == 0) return ST_OK;
    HIPCHK(f->host.stream_or_create(), ST_INTERNAL);
    const hipStream_t s = f->host.stream;
    HIPCHK(f->bx.ensure(sizeof(float) * n), ST_INTERNAL);
    HIPCHK(f->by.ensure(sizeof(float) * n), ST_INTERNAL);
    const float* dp = nullptr;
    if (prefix && f->taps > 1) {
        HIPCHK(f->bp.ensure(sizeof(float) * (f->taps - 1)), ST_INTERNAL);
        HIPCHK(hipMemcpyAsync(f->bp.p, prefix, sizeof(float) * (f->taps - 1), hipMemcpyHostToDevice, s), ST_INTERNAL);
        dp = (const float*)f->bp.p;
    }
    HIPCHK(hipMemcpyAsync(f->bx.p, x, sizeof(float) * n, hipMemcpyHostToDevice, s), ST_INTERNAL);
    int st = vvhip_fir_apply_device(f, (const float*)f->bx.p, (float*)f->by.p, n, 1, n, n, dp, mode, s);
    if (st) return st;
    HIPCHK(hipMemcpyAsync(y, f->by.p, sizeof(float) * n, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
    return ST_OK;
}

int vvhip_fir_filtfilt_device(vvhip_fir* f, const float* d_x, float* d_y, size_t n, size_t nch, size_t x_stride,
                              size_t y_stride, void* stream) {
    if (!f || !d_x || !d_y) return ST_NULL;
    if (n == 0 || nch == 0) return ST_OK;
    hipStream_t s = (hipStream_t)stream;
    Scratch tmp(s);
    HIPCHK(tmp.alloc(sizeof(float) * (n + f->taps - 1) * nch), ST_INTERNAL);
    HIPCHK(launch_filtfilt(f->d_h, (long long)f->taps, d_x, d_y, (long long)n, (long long)nch, (long long)x_stride,
                           (long long)y_stride, (float*)tmp.p, s),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_fir_filtfilt_host(vvhip_fir* f, const float* x, float* y, size_t n) {
    if (!f || !x || !y) return ST_NULL;
    std::lock_guard<std::mutex> host_lock(f->host.mu);
    if (n == 0) return ST_OK;
    HIPCHK(f->host.stream_or_create(), ST_INTERNAL);
    const hipStream_t s = f->host.stream;
    HIPCHK(f->bx.ensure(sizeof(float) * n), ST_INTERNAL);
    HIPCHK(f->by.ensure(sizeof(float) * n), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(f->bx.p, x, sizeof(float) * n, hipMemcpyHostToDevice, s), ST_INTERNAL);
    int st = vvhip_fir_filtfilt_device(f, (const float*)f->bx.p, (float*)f->by.p, n, 1, n, n, s);
    if (st) return st;
    HIPCHK(hipMemcpyAsync(y, f->by.p, sizeof(float) * n, hipMemcpyDeviceToHost, s), ST_INTERNAL);
    HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
    return ST_OK;
}

}  // extern "C"
