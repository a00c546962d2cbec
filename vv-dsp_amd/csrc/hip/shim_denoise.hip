// shim_denoise.hip -- spectral noise suppression (include/vv_dsp/spectral/denoise.h):
// the entry points over denoise_kernels.hip.  Every check is made before any
// device work, in the header's order.  Knob DENOISE_SEGMENT = L forces the
// segment length of the walk down the rows, DENOISE_MIN = 1 / 2 the direct / the
// blockwise minimum (the same bits; for timing the two and for putting segment
// seams at chosen rows).  The signal form works in groups of channels whose rows
// fit DENOISE_GROUP_BYTES of scratch (knob DENOISE_GROUP = k: k channels per
// group); every kernel it runs treats a channel on its own, so the grouping
// changes no value.
#include "shim_common.hpp"
#include "../../../include/vv_dsp/spectral/denoise.h"

#include <cmath>

using namespace vvh;

static_assert(DN_MAX_SMOOTH == VV_DSP_DENOISE_MAX_SMOOTH && DN_MAX_REACH == VV_DSP_DENOISE_MAX_REACH &&
                  DN_GATE == VV_DSP_DENOISE_GATE && DN_WIENER == VV_DSP_DENOISE_WIENER &&
                  DN_SUBTRACT == VV_DSP_DENOISE_SUBTRACT,
              "denoise.h");
static_assert(sizeof(vvhip_denoise_params) == sizeof(vv_dsp_denoise_params) &&
                  sizeof(vvhip_denoise_out) == sizeof(vv_dsp_denoise_out),
              "denoise.h");

static constexpr size_t DENOISE_GROUP_BYTES = (size_t)1 << 30;

// checks 2 to 4 of denoise.h but for the counts (pitched: the device form's pitches)
static int denoise_check(const vvhip_denoise_params* p, bool pitched, size_t row_pitch, size_t out_pitch) {
    if (p->n_fft < 2) return fail(ST_SIZE, "denoise: n_fft below 2");
    const size_t K = p->n_fft / 2 + 1;
    if (pitched && (row_pitch < K || out_pitch < K)) return fail(ST_SIZE, "denoise: a pitch below n_fft/2+1");
    if (p->smooth_len < 1) return fail(ST_RANGE, "denoise: smooth_len below 1");
    if (p->back < 0 || p->ahead < 0) return fail(ST_RANGE, "denoise: a negative back or ahead");
    if (p->mode < DN_GATE || p->mode > DN_SUBTRACT) return fail(ST_RANGE, "denoise: unknown mode");
    if (!(std::isfinite(p->bias) && p->bias > 0.0f)) return fail(ST_RANGE, "denoise: bias must be finite and positive");
    if (!(p->floor >= 0.0f && p->floor <= 1.0f)) return fail(ST_RANGE, "denoise: floor outside [0, 1]");
    if (p->smooth_len > DN_MAX_SMOOTH) return fail(ST_UNSUP, "denoise: smooth_len above 64");
    if (p->back > DN_MAX_REACH || p->ahead > DN_MAX_REACH) return fail(ST_UNSUP, "denoise: back or ahead above 511");
    if (K > (size_t)HPSS_MAX_BINS) return fail(ST_UNSUP, "denoise: rows above 8193 bins");
    return ST_OK;
}

// the rest of check 4: rpg the resolved group length (> 0 when rows > 0)
static int denoise_counts(size_t rows, size_t rpg, size_t K) {
    if (rpg >= ((size_t)1 << 31)) return fail(ST_UNSUP, "denoise: a group of 2^31 rows or more");
    const size_t lim = (size_t)1 << 30;
    if (rows >= lim || rows * ((K + 15) / 16) >= lim) return fail(ST_UNSUP, "denoise: more rows than one launch takes");
    return ST_OK;
}

static int denoise_run(const float* d_power, size_t rows, size_t row_pitch, size_t rpg, const vvhip_denoise_params* p,
                       const vvhip_denoise_out* o, size_t out_pitch, hipStream_t s) {
    DenoiseArgs a;
    a.p = d_power;
    a.rows = (long long)rows;
    a.K = (long long)(p->n_fft / 2 + 1);
    a.p_pitch = (long long)row_pitch;
    a.rpg = (long long)rpg;
    a.W = p->smooth_len;
    a.back = p->back;
    a.ahead = p->ahead;
    a.mode = p->mode;
    a.bias = (double)p->bias;
    a.floor = (double)p->floor;
    a.smooth = o->smooth;
    a.noise = o->noise;
    a.gain = o->gain;
    a.o_pitch = (long long)out_pitch;
    a.seg = (int)knob(KNOB_DENOISE_SEGMENT, 0);
    const long long k = knob(KNOB_DENOISE_MIN, 0);
    a.direct = k == 1 ? 1 : k == 2 ? 0 : p->back + p->ahead + 1 < DN_DIRECT_BELOW;
    HIPCHK(launch_denoise(a, s), ST_INTERNAL);
    return ST_OK;
}

extern "C" {

int vvhip_denoise_device(const float* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                         const vvhip_denoise_params* params, const vvhip_denoise_out* o, size_t out_pitch,
                         void* stream) {
    if (!params || !d_power || !o) return ST_NULL;
    if (int st = denoise_check(params, true, row_pitch, out_pitch)) return st;
    const size_t rpg = rows_per_group == 0 || rows_per_group > rows ? rows : rows_per_group;
    if (int st = denoise_counts(rows, rpg, params->n_fft / 2 + 1)) return st;
    if (rows == 0 || !(o->smooth || o->noise || o->gain)) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    return denoise_run(d_power, rows, row_pitch, rpg, params, o, out_pitch, (hipStream_t)stream);
}

// One group of packed rows in host memory through the same kernel.
int vvhip_denoise_host(const float* power_rows, size_t rows, const vvhip_denoise_params* params,
                       const vvhip_denoise_out* o) {
    if (!params || !power_rows || !o) return ST_NULL;
    if (int st = denoise_check(params, false, 0, 0)) return st;
    const size_t K = params->n_fft / 2 + 1;
    if (int st = denoise_counts(rows, rows, K)) return st;
    if (rows == 0 || !(o->smooth || o->noise || o->gain)) return ST_OK;
    HostCall c("denoise");
    const size_t bytes = sizeof(float) * rows * K;
    const float* dp = (const float*)c.in(power_rows, bytes);
    // the three planes side by side in one device buffer; each wanted plane is copied down on its own
    float* planes = (float*)c.out(nullptr, 3 * bytes);
    if (!c.ok()) return c.st;
    float* const host[3] = {o->smooth, o->noise, o->gain};
    vvhip_denoise_out d;
    float** const dev[3] = {&d.smooth, &d.noise, &d.gain};
    for (int i = 0; i < 3; ++i) *dev[i] = host[i] ? planes + (size_t)i * rows * K : nullptr;
    if (int st = denoise_run(dp, rows, K, rows, params, &d, K, c.s)) return st;
    for (int i = 0; i < 3; ++i)
        if (host[i]) HIPCHK(hipMemcpyAsync(host[i], *dev[i], bytes, hipMemcpyDeviceToHost, c.s), ST_INTERNAL);
    return c.finish(ST_OK);
}

int vvhip_stft_denoise_device(vvhip_stft* h, const vvhip_denoise_params* params, const float* d_signal, size_t n,
                              size_t nch, size_t ch_stride, float* d_out, size_t out_ch_stride, void* stream,
                              size_t* out_len) {
    if (!h || !params || !d_signal || !d_out) return ST_NULL;
    const size_t nfft = h->nfft, hop = h->hop;
    if (nfft < 2) return fail(ST_SIZE, "stft_denoise: fft_size below 2");
    if (params->n_fft != nfft) return fail(ST_SIZE, "stft_denoise: n_fft differs from the stft's fft_size");
    if (nch > 1 && ch_stride < n) return fail(ST_SIZE, "stft_denoise: a channel stride shorter than its channel");
    const size_t T = vvhip_stft_num_frames(n, nfft, hop), K = nfft / 2 + 1;
    const size_t lim = (size_t)1 << 31;
    const size_t len = T < lim ? (T - 1) * hop + nfft : SIZE_MAX;
    if (out_ch_stride < len) return fail(ST_SIZE, "stft_denoise: output channel stride below out_len");
    if (int st = denoise_check(params, false, 0, 0)) return st;
    if (int st = denoise_counts(T, T, K)) return st;
    if (nch >= lim) return fail(ST_UNSUP, "stft_denoise: 2^31 channels or more");
    if (out_len) *out_len = len;
    if (nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");

    const hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = 2 * sizeof(float) * nfft, plane = sizeof(float) * T * K;
    // per channel: power and gain; spectrum and scaled rows; norm
    const size_t ch_bytes = 2 * plane + 2 * T * row_bytes + sizeof(float) * len;
    const long long forced = knob(KNOB_DENOISE_GROUP, 0);
    size_t group = forced > 0 ? (size_t)forced : DENOISE_GROUP_BYTES / ch_bytes;
    // one launch of a group's rows must stay inside the kernels' counts
    const size_t dlim = (size_t)1 << 30;
    while (group > 1 && (group * T >= dlim || group * T * ((nfft + 255) / 256) >= lim ||
                         group * T * ((K + 15) / 16) >= dlim))
        group /= 2;
    if (group < 1) group = 1;
    if (group > nch) group = nch;
    if (T * ((nfft + 255) / 256) >= lim) return fail(ST_UNSUP, "stft_denoise: more rows than one launch takes");
    Scratch pw(s), gn(s), spec(s), rows(s), norm(s);
    HIPCHK(pw.alloc(group * plane), ST_INTERNAL);
    HIPCHK(gn.alloc(group * plane), ST_INTERNAL);
    HIPCHK(spec.alloc(group * T * row_bytes), ST_INTERNAL);
    HIPCHK(rows.alloc(group * T * row_bytes), ST_INTERNAL);
    HIPCHK(norm.alloc(group * len * sizeof(float)), ST_INTERNAL);
    const vvhip_denoise_out o = {nullptr, nullptr, (float*)gn.p};
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const size_t g = nch - c0 < group ? nch - c0 : group;
        const float* sig = d_signal + c0 * ch_stride;
        float* y = d_out + c0 * out_ch_stride;
        if (int st = stft_frames_run(h, sig, n, g, ch_stride, pw.p, T * K, 2, s)) return st;
        if (int st = denoise_run((const float*)pw.p, g * T, K, T, params, &o, K, s)) return st;
        if (int st = stft_frames_run(h, sig, n, g, ch_stride, spec.p, T * nfft, 1, s)) return st;
        HIPCHK(launch_hpss_apply((const float2*)spec.p, (const float*)gn.p, (float2*)rows.p, (long long)(g * T),
                                 (long long)nfft, s),
               ST_INTERNAL);
        HIPCHK(hipMemsetAsync(norm.p, 0, g * len * sizeof(float), s), ST_INTERNAL);
        for (size_t c = 0; c < g; ++c) {
            HIPCHK(hipMemsetAsync(y + c * out_ch_stride, 0, len * sizeof(float), s), ST_INTERNAL);
            if (int st = vvhip_stft_reconstruct_device(h, (const float*)rows.p + 2 * c * T * nfft, T, hop,
                                                       y + c * out_ch_stride, (float*)norm.p + c * len, s))
                return st;
        }
        HIPCHK(launch_pvoc_normalize(y, (long long)out_ch_stride, (const float*)norm.p, (long long)len, (long long)g,
                                     s),
               ST_INTERNAL);
    }
    return ST_OK;
}

}  // extern "C"
