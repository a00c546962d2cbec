// shim_median.hip -- the running median (include/vv_dsp/filter/median.h) and
// harmonic-percussive separation (include/vv_dsp/spectral/hpss.h): the entry
// points over median_kernels.hip.  Every check is made before any device work,
// in the headers' order.  Knob MEDIAN_SELECT = 1 / 2 forces the counting / the
// bitwise select (the same bits; for timing the two).  The signal form works in
// groups of channels whose rows fit HPSS_GROUP_BYTES of scratch (knob HPSS_GROUP
// = k: k channels per group); every kernel it runs treats a channel on its own,
// so the grouping changes no value.
#include "shim_common.hpp"
#include "../../../include/vv_dsp/filter/median.h"
#include "../../../include/vv_dsp/spectral/hpss.h"

#include <cmath>

using namespace vvh;

static_assert(MED_MAX_WINDOW == VV_DSP_MEDFILT_MAX_WINDOW, "median.h");
static_assert((int)MED_REFLECT == (int)VV_DSP_MEDFILT_MODE_REFLECT &&
                  (int)MED_NEAREST == (int)VV_DSP_MEDFILT_MODE_NEAREST && (int)MED_ZERO == (int)VV_DSP_MEDFILT_MODE_ZERO,
              "median.h");
static_assert(HPSS_MAX_BINS == VV_DSP_HPSS_MAX_BINS && HPSS_HARD == VV_DSP_HPSS_HARD &&
                  HPSS_SOFT == VV_DSP_HPSS_SOFT && HPSS_WIENER == VV_DSP_HPSS_WIENER,
              "hpss.h");
static_assert(sizeof(vvhip_hpss_params) == sizeof(vv_dsp_hpss_params) &&
                  sizeof(vvhip_hpss_out) == sizeof(vv_dsp_hpss_out),
              "hpss.h");

static constexpr size_t HPSS_GROUP_BYTES = (size_t)1 << 30;

static int med_radix(int L) {
    const long long k = knob(KNOB_MEDIAN_SELECT, 0);
    return k == 1 ? 0 : k == 2 ? 1 : L >= MED_RADIX_FROM;
}

// checks 2 to 4 of median.h (strided: the device form's strides)
static int medfilt_check(size_t n, size_t batch, bool strided, size_t x_stride, size_t y_stride, int L, int mode) {
    if (n == 0) return fail(ST_SIZE, "medfilt: n == 0");
    if (strided && batch > 1 && (x_stride < n || y_stride < n)) return fail(ST_SIZE, "medfilt: a stride below n");
    if (L < 1 || (L & 1) == 0) return fail(ST_RANGE, "medfilt: window_length must be odd and positive");
    if (mode < MED_REFLECT || mode > MED_ZERO) return fail(ST_RANGE, "medfilt: unknown mode");
    if (L > MED_MAX_WINDOW) return fail(ST_UNSUP, "medfilt: window_length above 127");
    if (n >= ((size_t)1 << 40) || batch >= ((size_t)1 << 31) || !med_rows_supported((long long)batch, (long long)n))
        return fail(ST_UNSUP, "medfilt: more tiles than one launch takes");
    return ST_OK;
}

static int medfilt_run(const float* d_x, size_t n, size_t batch, size_t x_stride, int L, int mode, float* d_y,
                       size_t y_stride, hipStream_t s) {
    MedArgs a;
    a.x = d_x;
    a.lines = (long long)batch;
    a.n = (long long)n;
    a.x_pitch = (long long)x_stride;
    a.L = L;
    a.mode = mode;
    a.radix = med_radix(L);
    a.y = d_y;
    a.y_pitch = (long long)y_stride;
    HIPCHK(launch_med_rows(a, s), ST_INTERNAL);
    return ST_OK;
}

// checks 2 to 4 of hpss.h but for the counts (pitched: the device form's pitches)
static int hpss_check(const vvhip_hpss_params* p, bool pitched, size_t row_pitch, size_t out_pitch) {
    if (p->n_fft < 2) return fail(ST_SIZE, "hpss: n_fft below 2");
    const size_t K = p->n_fft / 2 + 1;
    if (pitched && (row_pitch < K || out_pitch < K)) return fail(ST_SIZE, "hpss: a pitch below n_fft/2+1");
    if (p->win_harm < 1 || (p->win_harm & 1) == 0 || p->win_perc < 1 || (p->win_perc & 1) == 0)
        return fail(ST_RANGE, "hpss: windows must be odd and positive");
    if (p->mask < HPSS_HARD || p->mask > HPSS_WIENER) return fail(ST_RANGE, "hpss: unknown mask");
    if (!(std::isfinite(p->margin_harm) && p->margin_harm >= 1.0f && std::isfinite(p->margin_perc) &&
          p->margin_perc >= 1.0f))
        return fail(ST_RANGE, "hpss: margins must be finite and at least 1");
    if (p->win_harm > MED_MAX_WINDOW || p->win_perc > MED_MAX_WINDOW) return fail(ST_UNSUP, "hpss: a window above 127");
    if (K > (size_t)HPSS_MAX_BINS) return fail(ST_UNSUP, "hpss: rows above 8193 bins");
    return ST_OK;
}

// the rest of check 4: rpg the resolved group length (> 0 when rows > 0)
static int hpss_counts(size_t rows, size_t rpg, size_t K) {
    const size_t lim = (size_t)1 << 31;
    if (rpg >= lim) return fail(ST_UNSUP, "hpss: a group of 2^31 rows or more");
    if (rows >= lim || rows * ((K + 63) / 64) >= lim) return fail(ST_UNSUP, "hpss: more rows than one launch takes");
    return ST_OK;
}

static int hpss_run(const float* d_power, size_t rows, size_t row_pitch, size_t rpg, const vvhip_hpss_params* p,
                    const vvhip_hpss_out* o, size_t out_pitch, hipStream_t s) {
    const size_t K = p->n_fft / 2 + 1;
    const bool masks = o->mask_harm || o->mask_perc;
    MedArgs a;
    a.x = d_power;
    a.lines = (long long)rows;
    a.n = (long long)K;
    a.x_pitch = (long long)row_pitch;
    a.rpg = (long long)rpg;
    a.mode = MED_REFLECT;
    a.sqrt_w = p->magnitude != 0;
    a.y_pitch = (long long)out_pitch;
    Scratch hs(s);
    const float* H = o->harm;
    long long h_pitch = (long long)out_pitch;
    if (o->harm || masks) {
        if (!o->harm) {
            HIPCHK(hs.alloc(sizeof(float) * rows * K), ST_INTERNAL);
            H = (const float*)hs.p;
            h_pitch = (long long)K;
        }
        MedArgs c = a;
        c.L = p->win_harm;
        c.radix = med_radix(c.L);
        c.y = const_cast<float*>(H);
        c.y_pitch = h_pitch;
        HIPCHK(launch_med_cols(c, s), ST_INTERNAL);
    }
    if (o->perc || masks) {
        MedArgs r = a;
        r.L = p->win_perc;
        r.radix = med_radix(r.L);
        r.y = o->perc;
        if (masks) {
            r.H = H;
            r.h_pitch = h_pitch;
            r.mask_h = o->mask_harm;
            r.mask_p = o->mask_perc;
            r.margin_h = (double)p->margin_harm;
            r.margin_p = (double)p->margin_perc;
            r.mask = p->mask;
        }
        HIPCHK(launch_med_rows(r, s), ST_INTERNAL);
    }
    return ST_OK;
}

extern "C" {

int vvhip_medfilt_device(const float* d_x, size_t n, size_t batch, size_t x_stride, int window_length, int mode,
                         float* d_y, size_t y_stride, void* stream) {
    if (!d_x || !d_y) return ST_NULL;
    if (int st = medfilt_check(n, batch, true, x_stride, y_stride, window_length, mode)) return st;
    if (batch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    return medfilt_run(d_x, n, batch, x_stride, window_length, mode, d_y, y_stride, (hipStream_t)stream);
}

// One row in host memory through the same kernel.
int vvhip_medfilt_host(const float* x, size_t n, int window_length, int mode, float* y) {
    if (!x || !y) return ST_NULL;
    if (int st = medfilt_check(n, 1, false, 0, 0, window_length, mode)) return st;
    HostCall c("medfilt");
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    float* dy = (float*)c.out(y, sizeof(float) * n);
    if (!c.ok()) return c.st;
    return c.finish(medfilt_run(dx, n, 1, n, window_length, mode, dy, n, c.s));
}

int vvhip_hpss_device(const float* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                      const vvhip_hpss_params* params, const vvhip_hpss_out* o, size_t out_pitch, void* stream) {
    if (!params || !d_power || !o) return ST_NULL;
    if (int st = hpss_check(params, true, row_pitch, out_pitch)) return st;
    const size_t rpg = rows_per_group == 0 || rows_per_group > rows ? rows : rows_per_group;
    if (int st = hpss_counts(rows, rpg, params->n_fft / 2 + 1)) return st;
    if (rows == 0 || !(o->harm || o->perc || o->mask_harm || o->mask_perc)) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    return hpss_run(d_power, rows, row_pitch, rpg, params, o, out_pitch, (hipStream_t)stream);
}

// One group of packed rows in host memory through the same kernels.
int vvhip_hpss_host(const float* power_rows, size_t rows, const vvhip_hpss_params* params, const vvhip_hpss_out* o) {
    if (!params || !power_rows || !o) return ST_NULL;
    if (int st = hpss_check(params, false, 0, 0)) return st;
    const size_t K = params->n_fft / 2 + 1;
    if (int st = hpss_counts(rows, rows, K)) return st;
    if (rows == 0 || !(o->harm || o->perc || o->mask_harm || o->mask_perc)) return ST_OK;
    HostCall c("hpss");
    const size_t bytes = sizeof(float) * rows * K;
    const float* dp = (const float*)c.in(power_rows, bytes);
    // the four planes side by side in one device buffer; each wanted plane is copied down on its own
    float* planes = (float*)c.out(nullptr, 4 * bytes);
    if (!c.ok()) return c.st;
    float* const host[4] = {o->harm, o->perc, o->mask_harm, o->mask_perc};
    vvhip_hpss_out d;
    float** const dev[4] = {&d.harm, &d.perc, &d.mask_harm, &d.mask_perc};
    for (int i = 0; i < 4; ++i) *dev[i] = host[i] ? planes + (size_t)i * rows * K : nullptr;
    if (int st = hpss_run(dp, rows, K, rows, params, &d, K, c.s)) return st;
    for (int i = 0; i < 4; ++i)
        if (host[i]) HIPCHK(hipMemcpyAsync(host[i], *dev[i], bytes, hipMemcpyDeviceToHost, c.s), ST_INTERNAL);
    return c.finish(ST_OK);
}

int vvhip_stft_hpss_device(vvhip_stft* h, const vvhip_hpss_params* params, const float* d_signal, size_t n, size_t nch,
                           size_t ch_stride, float* d_out_harm, float* d_out_perc, size_t out_ch_stride,
                           void* stream, size_t* out_len) {
    if (!h || !params || !d_signal || (!d_out_harm && !d_out_perc)) return ST_NULL;
    const size_t nfft = h->nfft, hop = h->hop;
    if (nfft < 2) return fail(ST_SIZE, "stft_hpss: fft_size below 2");
    if (params->n_fft != nfft) return fail(ST_SIZE, "stft_hpss: n_fft differs from the stft's fft_size");
    if (nch > 1 && ch_stride < n) return fail(ST_SIZE, "stft_hpss: a channel stride shorter than its channel");
    const size_t T = vvhip_stft_num_frames(n, nfft, hop), K = nfft / 2 + 1;
    const size_t lim = (size_t)1 << 31;
    const size_t len = T < lim ? (T - 1) * hop + nfft : SIZE_MAX;
    if (out_ch_stride < len) return fail(ST_SIZE, "stft_hpss: output channel stride below out_len");
    if (int st = hpss_check(params, false, 0, 0)) return st;
    if (int st = hpss_counts(T, T, K)) return st;
    if (nch >= lim) return fail(ST_UNSUP, "stft_hpss: 2^31 channels or more");
    if (out_len) *out_len = len;
    if (nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");

    const hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = 2 * sizeof(float) * nfft, plane = sizeof(float) * T * K;
    // per channel: power, H, two masks; spectrum and masked rows; norm
    const size_t ch_bytes = 4 * plane + 2 * T * row_bytes + sizeof(float) * len;
    const long long forced = knob(KNOB_HPSS_GROUP, 0);
    size_t group = forced > 0 ? (size_t)forced : HPSS_GROUP_BYTES / ch_bytes;
    // one launch of a group's rows must stay inside the kernels' counts
    while (group > 1 && (group * T >= lim || group * T * ((nfft + 255) / 256) >= lim)) group /= 2;
    if (group < 1) group = 1;
    if (group > nch) group = nch;
    if (T * ((nfft + 255) / 256) >= lim) return fail(ST_UNSUP, "stft_hpss: more rows than one launch takes");
    Scratch pw(s), mh(s), mp(s), spec(s), rows(s), norm(s);
    HIPCHK(pw.alloc(group * plane), ST_INTERNAL);
    if (d_out_harm) HIPCHK(mh.alloc(group * plane), ST_INTERNAL);
    if (d_out_perc) HIPCHK(mp.alloc(group * plane), ST_INTERNAL);
    HIPCHK(spec.alloc(group * T * row_bytes), ST_INTERNAL);
    HIPCHK(rows.alloc(group * T * row_bytes), ST_INTERNAL);
    HIPCHK(norm.alloc(group * len * sizeof(float)), ST_INTERNAL);
    vvhip_hpss_out o = {nullptr, nullptr, (float*)mh.p, (float*)mp.p};
    float* const outs[2] = {d_out_harm, d_out_perc};
    const float* const masks[2] = {(const float*)mh.p, (const float*)mp.p};
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const size_t g = nch - c0 < group ? nch - c0 : group;
        const float* sig = d_signal + c0 * ch_stride;
        if (int st = stft_frames_run(h, sig, n, g, ch_stride, pw.p, T * K, 2, s)) return st;
        if (int st = hpss_run((const float*)pw.p, g * T, K, T, params, &o, K, s)) return st;
        if (int st = stft_frames_run(h, sig, n, g, ch_stride, spec.p, T * nfft, 1, s)) return st;
        for (int w = 0; w < 2; ++w) {
            if (!outs[w]) continue;
            float* y = outs[w] + c0 * out_ch_stride;
            HIPCHK(launch_hpss_apply((const float2*)spec.p, masks[w], (float2*)rows.p, (long long)(g * T),
                                     (long long)nfft, s),
                   ST_INTERNAL);
            HIPCHK(hipMemsetAsync(norm.p, 0, g * len * sizeof(float), s), ST_INTERNAL);
            for (size_t c = 0; c < g; ++c) {
                HIPCHK(hipMemsetAsync(y + c * out_ch_stride, 0, len * sizeof(float), s), ST_INTERNAL);
                if (int st = vvhip_stft_reconstruct_device(h, (const float*)rows.p + 2 * c * T * nfft, T, hop,
                                                           y + c * out_ch_stride, (float*)norm.p + c * len, s))
                    return st;
            }
            HIPCHK(launch_pvoc_normalize(y, (long long)out_ch_stride, (const float*)norm.p, (long long)len,
                                         (long long)g, s),
                   ST_INTERNAL);
        }
    }
    return ST_OK;
}

}  // extern "C"
