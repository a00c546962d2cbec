// shim_pitch.hip -- per-frame pitch by YIN (include/vv_dsp/features/pitch.h): the
// entry points over pitch_kernels.hip.  Every check is made before any device
// work, in this order: null pointers; a zero length (or hop); the parameters'
// ranges and tau_min < tau_max; an integration length below 1; the kernel's
// limits (frame 16384, tau_max 8191); no output wanted (OK, nothing launched);
// strides shorter than what they step over.  One kernel, one wave per row;
// STAT_PITCH_WAVE counts its launches.  Knob PITCH_F32 = 1 keeps the row in LDS
// as f32 at every size (same bits; for timing the two storages).
#include "shim_common.hpp"

#include <cmath>
#include <cstring>

using namespace vvh;

// the lag range of a row of `len` samples, in double from the float parameters
static int pitch_range(const vvhip_pitch_params* p, size_t len, PitchCfg* cfg) {
    if (len == 0) return ST_SIZE;
    const double fs = (double)p->sample_rate, lo = (double)p->fmin, hi = (double)p->fmax, thr = (double)p->threshold;
    if (!(std::isfinite(fs) && std::isfinite(lo) && std::isfinite(hi) && fs > 0.0 && lo > 0.0 && hi > 0.0))
        return fail(ST_RANGE, "pitch: sample_rate, fmin and fmax must be finite and positive");
    if (lo >= hi) return fail(ST_RANGE, "pitch: fmin >= fmax");
    if (hi > fs / 2.0) return fail(ST_RANGE, "pitch: fmax above sample_rate / 2");
    if (!(thr > 0.0 && thr <= 1.0)) return fail(ST_RANGE, "pitch: threshold outside (0, 1]");
    double tmin = std::floor(fs / hi), tmax = std::ceil(fs / lo);
    if (tmin < 2.0) tmin = 2.0;
    if (tmin >= tmax) return fail(ST_RANGE, "pitch: no lag between sample_rate / fmax and sample_rate / fmin");
    if ((double)len <= tmax) return fail(ST_SIZE, "pitch: the frame is no longer than sample_rate / fmin");
    if (len > (size_t)PITCH_MAX_FRAME || tmax > (double)PITCH_MAX_LAG)
        return fail(ST_UNSUP, "pitch: frames above 16384 samples or lags above 8191");
    cfg->sample_rate = fs;
    cfg->threshold = thr;
    cfg->tau_min = (int)tmin;
    cfg->tau_max = (int)tmax;
    cfg->W = (int)len - cfg->tau_max;
    return ST_OK;
}

static PitchOut pitch_out(const vvhip_pitch_out* o) {
    PitchOut out;
    out.f0 = o->f0;
    out.aperiodicity = o->aperiodicity;
    out.lag = o->lag;
    out.cmnd = o->cmnd;
    return out;
}

static int pitch_run(const FrameSrc& src, const PitchCfg& cfg, const PitchOut& out, hipStream_t s) {
    HIPCHK(launch_pitch(src, cfg, out, knob(KNOB_PITCH_F32, 0) == 1, s), ST_INTERNAL);
    stat_inc(STAT_PITCH_WAVE);
    return ST_OK;
}

extern "C" {

int vvhip_pitch_lag_range(const vvhip_pitch_params* params, size_t frame_len, size_t* tau_min, size_t* tau_max,
                          size_t* integration_len) {
    if (!params) return ST_NULL;
    PitchCfg cfg;
    const int st = pitch_range(params, frame_len, &cfg);
    if (st != ST_OK) return st;
    if (tau_min) *tau_min = (size_t)cfg.tau_min;
    if (tau_max) *tau_max = (size_t)cfg.tau_max;
    if (integration_len) *integration_len = (size_t)cfg.W;
    return ST_OK;
}

int vvhip_pitch_device(const float* d_x, size_t n, size_t batch, size_t row_stride, const vvhip_pitch_params* params,
                       const vvhip_pitch_out* o, size_t cmnd_row_stride, void* stream) {
    if (!d_x || !params || !o) return ST_NULL;
    PitchCfg cfg;
    const int st = pitch_range(params, n, &cfg);
    if (st != ST_OK) return st;
    PitchOut out = pitch_out(o);
    if (!out.any()) return ST_OK;
    if ((batch > 1 && row_stride < n) || (out.cmnd && cmnd_row_stride < (size_t)cfg.tau_max + 1))
        return fail(ST_SIZE, "pitch: a stride shorter than its row");
    if (batch >= ((size_t)1 << 31)) return fail(ST_SIZE, "pitch: batch >= 2^31");
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (batch == 0) return ST_OK;
    out.cmnd_row_stride = (long long)cmnd_row_stride;
    return pitch_run(rows_src(d_x, n, batch, row_stride), cfg, out, (hipStream_t)stream);
}

int vvhip_pitch_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                              size_t hop, size_t frames, int center, const float* d_window,
                              const vvhip_pitch_params* params, const vvhip_pitch_out* o, size_t out_ch_stride,
                              size_t cmnd_ch_stride, void* stream) {
    if (!d_signal || !params || !o) return ST_NULL;
    const FramesCall fc = {"pitch_frames", n, nch, frame_len, hop, frames};
    if (int st = fc.shape()) return st;
    PitchCfg cfg;
    if (int st = pitch_range(params, frame_len, &cfg)) return st;
    PitchOut out = pitch_out(o);
    if (!out.any()) return ST_OK;
    if (int st = fc.limits()) return st;
    const size_t curve = (size_t)cfg.tau_max + 1;
    if (nch > 1 && (ch_stride < n || ((out.f0 || out.aperiodicity || out.lag) && out_ch_stride < frames) ||
                    (out.cmnd && cmnd_ch_stride < frames * curve)))
        return fail(ST_SIZE, "pitch_frames: a channel stride shorter than its channel");
    int st;
    if (!fc.start(&st)) return st;
    out.ch_stride = (long long)out_ch_stride;
    out.cmnd_ch_stride = (long long)cmnd_ch_stride;
    out.cmnd_row_stride = (long long)curve;
    return pitch_run(frames_src(d_signal, n, nch, ch_stride, frame_len, hop, frames, center, d_window), cfg, out,
                     (hipStream_t)stream);
}

// One frame in host memory through the same kernel; either output may be null.
int vvhip_pitch_host(const float* x, size_t n, const vvhip_pitch_params* params, float* f0, float* aperiodicity) {
    if (!x || !params) return ST_NULL;
    PitchCfg cfg;
    const int st0 = pitch_range(params, n, &cfg);
    if (st0 != ST_OK) return st0;
    if (!f0 && !aperiodicity) return ST_OK;
    HostCall c("pitch");
    float res[2];
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    float* dres = (float*)c.out(res, sizeof res);
    if (!c.ok()) return c.st;
    const vvhip_pitch_out o = {f0 ? dres : nullptr, aperiodicity ? dres + 1 : nullptr, nullptr, nullptr};
    const int st = c.finish(vvhip_pitch_device(dx, n, 1, n, params, &o, 0, c.s));
    if (st != ST_OK) return st;
    if (f0) *f0 = res[0];
    if (aperiodicity) *aperiodicity = res[1];
    return ST_OK;
}

}  // extern "C"
