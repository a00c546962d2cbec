// shim_lpc.hip -- linear prediction (src/envelope/lpc.c): the entry points
// over lpc_kernels.hip.  Rows of the wave kernel's shapes (order <= 32, row
// length <= 4096) take it; any other order < length takes the generic kernels
// through a scratch autocorrelation buffer; knob LPC_GENERIC = 1 forces them.
// STAT_LPC_WAVE / STAT_LPC_GENERIC count which ran.
#include "shim_common.hpp"

using namespace vvh;

static bool lpc_generic(long long len, long long order) {
    return knob(KNOB_LPC_GENERIC, 0) == 1 || !lpc_wave_supported(len, order);
}

// contiguous rows
static FrameSrc lpc_rows(const float* d_x, size_t n, size_t batch) { return rows_src(d_x, n, batch, n); }

static LpcOut lpc_rows_out(float* d_a, float* d_err, size_t batch, int* d_flag) {
    LpcOut out;
    out.a = d_a;
    out.err = d_err;
    out.frames = (long long)batch;
    out.flag = d_flag;
    return out;
}

// autocorrelation + Levinson of src's rows
static int lpc_run(const FrameSrc& src, size_t order, const LpcOut& out, hipStream_t s) {
    if (!lpc_generic(src.len, (long long)order)) {
        HIPCHK(launch_lpc_wave(src, (int)order, nullptr, out, s), ST_INTERNAL);
        stat_inc(STAT_LPC_WAVE);
        return ST_OK;
    }
    Scratch r(s);
    HIPCHK(r.alloc(sizeof(float) * (size_t)src.rows * (order + 1)), ST_INTERNAL);
    HIPCHK(launch_autocorr_generic(src, (long long)order, (float*)r.p, s), ST_INTERNAL);
    HIPCHK(launch_levinson((const float*)r.p, (long long)order, src.rows, 1, out, s), ST_INTERNAL);
    stat_inc(STAT_LPC_GENERIC);
    return ST_OK;
}

static int lpc_sizes(size_t n, size_t order, size_t batch) {
    if (order + 1 > n || order + 1 == 0) return ST_SIZE;
    if (n >= ((size_t)1 << 31) || batch >= ((size_t)1 << 31)) return fail(ST_SIZE, "lpc: n or batch >= 2^31");
    return ST_OK;
}

extern "C" {

int vvhip_autocorr_device(const float* d_x, size_t n, size_t order, size_t batch, float* d_r, void* stream) {
    if (!d_x || !d_r) return ST_NULL;
    if (int st = lpc_sizes(n, order, batch)) return st;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (batch == 0) return ST_OK;
    const FrameSrc src = lpc_rows(d_x, n, batch);
    if (!lpc_generic(src.len, (long long)order)) {
        HIPCHK(launch_lpc_wave(src, (int)order, d_r, LpcOut(), (hipStream_t)stream), ST_INTERNAL);
        stat_inc(STAT_LPC_WAVE);
    } else {
        HIPCHK(launch_autocorr_generic(src, (long long)order, d_r, (hipStream_t)stream), ST_INTERNAL);
        stat_inc(STAT_LPC_GENERIC);
    }
    return ST_OK;
}

int vvhip_levinson_device(const float* d_r, size_t order, size_t batch, float* d_a, float* d_err, int* d_flag,
                          void* stream) {
    if (!d_r || !d_a || !d_err) return ST_NULL;
    if (order + 1 == 0 || order >= ((size_t)1 << 31) || batch >= ((size_t)1 << 31))
        return fail(ST_SIZE, "levinson: order or batch >= 2^31");
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (batch == 0) return ST_OK;
    const int generic = knob(KNOB_LPC_GENERIC, 0) == 1 || order > (size_t)LPC_WAVE_ORDER;
    HIPCHK(launch_levinson(d_r, (long long)order, (long long)batch, generic, lpc_rows_out(d_a, d_err, batch, d_flag),
                           (hipStream_t)stream),
           ST_INTERNAL);
    stat_inc(generic ? STAT_LPC_GENERIC : STAT_LPC_WAVE);
    return ST_OK;
}

int vvhip_lpc_device(const float* d_x, size_t n, size_t order, size_t batch, float* d_a, float* d_err, int* d_flag,
                     void* stream) {
    if (!d_x || !d_a || !d_err) return ST_NULL;
    if (int st = lpc_sizes(n, order, batch)) return st;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (batch == 0) return ST_OK;
    return lpc_run(lpc_rows(d_x, n, batch), order, lpc_rows_out(d_a, d_err, batch, d_flag), (hipStream_t)stream);
}

int vvhip_lpc_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                            size_t hop, size_t frames, int center, const float* d_window, size_t order, float* d_a,
                            size_t a_ch_stride, float* d_err, size_t err_ch_stride, void* stream) {
    if (!d_signal || !d_a || !d_err) return ST_NULL;
    const FramesCall fc = {"lpc_frames", n, nch, frame_len, hop, frames};
    if (int st = fc.shape()) return st;
    if (int st = lpc_sizes(frame_len, order, 0)) return st;
    if (int st = fc.limits()) return st;
    int st;
    if (!fc.start(&st)) return st;
    LpcOut out;
    out.a = d_a;
    out.err = d_err;
    out.frames = (long long)frames;
    out.a_ch_stride = (long long)a_ch_stride;
    out.err_ch_stride = (long long)err_ch_stride;
    return lpc_run(frames_src(d_signal, n, nch, ch_stride, frame_len, hop, frames, center, d_window), order, out,
                   (hipStream_t)stream);
}

int vvhip_lpspec_device(const float* d_a, size_t order, const float* d_gain, float gain, size_t nfft, size_t batch,
                        int levinson_sign, float* d_mag, void* stream) {
    if (!d_a || !d_mag) return ST_NULL;
    if (nfft >= ((size_t)1 << 30) || order >= ((size_t)1 << 30)) return fail(ST_SIZE, "lpspec: nfft or order >= 2^30");
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (nfft == 0 || batch == 0) return ST_OK;
    HIPCHK(launch_lpspec(d_a, (long long)order, d_gain, gain, (long long)nfft, (long long)batch, levinson_sign != 0,
                         d_mag, (hipStream_t)stream),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_autocorr_host(const float* x, size_t n, size_t order, float* r) {
    if (!x || !r) return ST_NULL;
    if (order + 1 > n || order + 1 == 0) return ST_SIZE;
    HostCall c("autocorr");
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    float* dr = (float*)c.out(r, sizeof(float) * (order + 1));
    if (!c.ok()) return c.st;
    return c.finish(vvhip_autocorr_device(dx, n, order, 1, dr, c.s));
}

int vvhip_levinson_host(const float* r, size_t order, float* a, float* err) {
    if (!r || !a || !err) return ST_NULL;
    HostCall c("levinson");
    const float* dr = (const float*)c.in(r, sizeof(float) * (order + 1));
    float* da = (float*)c.out(a, sizeof(float) * (order + 1));
    float* de = (float*)c.out(err, sizeof(float));
    if (!c.ok()) return c.st;
    return c.finish(vvhip_levinson_device(dr, order, 1, da, de, nullptr, c.s));
}

// a row whose r[0] <= 0 reports ST_INTERNAL and leaves a and err untouched
// (lpc.c:25, :50): the row's flag comes back from the device with it
int vvhip_lpc_host(const float* x, size_t n, size_t order, float* a, float* err) {
    if (!x || !a || !err) return ST_NULL;
    if (order + 1 > n || order + 1 == 0) return ST_SIZE;
    HostCall c("lpc");
    std::vector<float> res(order + 2);   // a[order + 1], err
    int flag = 0;
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    float* dres = (float*)c.out(res.data(), sizeof(float) * res.size());
    int* dflag = (int*)c.inout(&flag, sizeof(int));
    if (!c.ok()) return c.st;
    const int st = c.finish(vvhip_lpc_device(dx, n, order, 1, dres, dres + order + 1, dflag, c.s));
    if (st != ST_OK) return st;
    if (flag) return ST_INTERNAL;
    for (size_t i = 0; i <= order; ++i) a[i] = res[i];
    *err = res[order + 1];
    return ST_OK;
}

int vvhip_lpspec_host(const float* a, size_t order, float gain, size_t nfft, float* mag) {
    if (!a || !mag) return ST_NULL;
    if (nfft == 0) return ST_OK;
    HostCall c("lpspec");
    const float* da = (const float*)c.in(a, sizeof(float) * (order + 1));
    float* dm = (float*)c.out(mag, sizeof(float) * nfft);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_lpspec_device(da, order, nullptr, gain, nfft, 1, 0, dm, c.s));
}

}  // extern "C"
