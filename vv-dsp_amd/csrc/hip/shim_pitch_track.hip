// shim_pitch_track.hip -- f0 tracking over the YIN curves
// (include/vv_dsp/features/pitch_track.h): the entry points over
// pitch_track_kernels.hip.  Every check is made before any device work, in the
// header's order: null pointers; no frames (OK); the parameters' ranges; strides
// shorter than what they step over; the kernel's limits (max_step 126, 4096
// states, 2^31 frames); nothing wanted or no channel (OK); no device.
// STAT_PITCH_TRACK counts the tracker's launches (one per channel group).
//
// Scratch.  The tracker keeps one predecessor byte per state and frame: channels
// run in groups of at most PTRACK_WORK_BYTES (4 GiB) of it, at least one channel.
// The fused entry writes the curves of a group of channels to scratch with
// vvhip_pitch_frames_device and tracks them: groups of at most
// PTRACK_CURVE_BYTES (2 GiB) of curves, at least one channel (32 channels of ten
// minutes at 16 kHz, hop 160, 201 lags are 1.5 GiB: one group, so the tracker still
// runs all channels side by side).  Channels are
// independent, so no value depends on the grouping; knob PTRACK_GROUP = g > 0
// forces groups of g channels in both (for the tests that cross a boundary).
#include "shim_common.hpp"

#include <cmath>
#include <vector>

using namespace vvh;

static constexpr size_t PTRACK_WORK_BYTES = (size_t)4 << 30;
static constexpr size_t PTRACK_CURVE_BYTES = (size_t)2 << 30;

// checks 3 and 5 of the header on the parameters alone; *unsup is check 5's verdict
static int ptrack_params(const vvhip_pitch_track_params* p, PtrackCfg* cfg, bool* unsup) {
    const double fs = (double)p->sample_rate, lam = (double)p->lambda, jc = (double)p->jump_cost,
                 sc = (double)p->switch_cost, uc = (double)p->unvoiced_cost;
    if (p->tau_min < 1 || p->tau_min >= p->tau_max)
        return fail(ST_RANGE, "pitch_track: tau_min must be at least 1 and below tau_max");
    if (!(std::isfinite(lam) && std::isfinite(jc) && std::isfinite(sc) && std::isfinite(uc) && lam >= 0.0 &&
          jc >= 0.0 && sc >= 0.0 && uc >= 0.0))
        return fail(ST_RANGE, "pitch_track: lambda and the costs must be finite and not negative");
    if (!(std::isfinite(fs) && fs > 0.0)) return fail(ST_RANGE, "pitch_track: sample_rate must be finite and positive");
    *unsup = p->max_step > (uint32_t)PTRACK_MAX_STEP || p->tau_max - p->tau_min + 1 > (uint32_t)PTRACK_MAX_STATES;
    if (!*unsup) {
        cfg->sample_rate = fs;
        cfg->lambda = lam;
        cfg->jump = jc;
        cfg->sw = sc;
        cfg->uc = uc;
        cfg->tau_min = (int)p->tau_min;
        cfg->tau_max = (int)p->tau_max;
        cfg->B = (int)p->max_step;
    }
    return ST_OK;
}

static int ptrack_unsupported() {
    return fail(ST_UNSUP, "pitch_track: max_step above 126, more than 4096 states or 2^31 frames or channels");
}

// curves of nch channels on the device -> planes, in groups of channels
static int ptrack_run(const PtrackCfg& cfg, const float* d_q, size_t F, size_t nch, size_t row_stride,
                      size_t cmnd_ch_stride, const vvhip_pitch_track_out* o, size_t out_ch_stride, hipStream_t s) {
    const size_t per_ch = ptrack_scratch_bytes(cfg.S(), 1, (long long)F);
    size_t group = PTRACK_WORK_BYTES / per_ch;
    const long long forced = knob(KNOB_PTRACK_GROUP, 0);
    if (forced > 0) group = (size_t)forced;
    group = group < 1 ? 1 : group > nch ? nch : group;
    Scratch work(s);
    HIPCHK(work.alloc(ptrack_scratch_bytes(cfg.S(), (long long)group, (long long)F)), ST_INTERNAL);
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        PtrackArgs a;
        a.nch = (long long)(nch - c0 < group ? nch - c0 : group);
        a.F = (long long)F;
        a.q = d_q + c0 * cmnd_ch_stride;
        a.row_stride = (long long)row_stride;
        a.cmnd_ch_stride = (long long)cmnd_ch_stride;
        a.ch_stride = (long long)out_ch_stride;
        a.lag = o->lag ? o->lag + c0 * out_ch_stride : nullptr;
        a.f0 = o->f0 ? o->f0 + c0 * out_ch_stride : nullptr;
        a.aperiodicity = o->aperiodicity ? o->aperiodicity + c0 * out_ch_stride : nullptr;
        a.cost = o->cost ? o->cost + c0 : nullptr;
        a.work = (unsigned char*)work.p;
        HIPCHK(launch_pitch_track(cfg, a, s), ST_INTERNAL);
        stat_inc(STAT_PITCH_TRACK);
    }
    return ST_OK;
}

static bool ptrack_any(const vvhip_pitch_track_out* o) { return o->lag || o->f0 || o->aperiodicity || o->cost; }

extern "C" {

int vvhip_pitch_track_params_default(const vvhip_pitch_params* pitch, size_t frame_len,
                                     vvhip_pitch_track_params* track) {
    if (!pitch || !track) return ST_NULL;
    size_t lo = 0, hi = 0;
    const int st = vvhip_pitch_lag_range(pitch, frame_len, &lo, &hi, nullptr);
    if (st != ST_OK) return st;
    track->sample_rate = pitch->sample_rate;
    track->tau_min = (uint32_t)lo;
    track->tau_max = (uint32_t)hi;
    track->lambda = 4.0f;
    track->jump_cost = 0.5f;
    track->switch_cost = 0.3f;
    track->unvoiced_cost = 0.35f;
    track->max_step = 8;
    return ST_OK;
}

int vvhip_pitch_track_device(const float* d_curves, size_t frames, size_t nch, size_t row_stride,
                             size_t cmnd_ch_stride, const vvhip_pitch_track_params* params,
                             const vvhip_pitch_track_out* o, size_t out_ch_stride, void* stream) {
    if (!d_curves || !params || !o) return ST_NULL;
    if (frames == 0) return ST_OK;
    PtrackCfg cfg;
    bool unsup = false;
    if (int st = ptrack_params(params, &cfg, &unsup)) return st;
    const size_t curve = (size_t)params->tau_max + 1;
    if (row_stride < curve) return fail(ST_SIZE, "pitch_track: a row stride below tau_max + 1");
    if (nch > 1 && (cmnd_ch_stride < (frames - 1) * row_stride + curve ||
                    ((o->lag || o->f0 || o->aperiodicity) && out_ch_stride < frames)))
        return fail(ST_SIZE, "pitch_track: a channel stride shorter than its channel");
    if (unsup || frames >= ((size_t)1 << 31) || nch >= ((size_t)1 << 31)) return ptrack_unsupported();
    if (!ptrack_any(o) || nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    return ptrack_run(cfg, d_curves, frames, nch, row_stride, cmnd_ch_stride, o, out_ch_stride, (hipStream_t)stream);
}

int vvhip_pitch_track_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                                    size_t hop, size_t frames, int center, const float* d_window,
                                    const vvhip_pitch_params* pitch, const vvhip_pitch_track_params* track,
                                    const vvhip_pitch_track_out* o, size_t out_ch_stride, void* stream) {
    if (!d_signal || !pitch || !track || !o) return ST_NULL;
    if (hop == 0 || frame_len == 0) return ST_SIZE;
    size_t ptau = 0;
    if (int st = vvhip_pitch_lag_range(pitch, frame_len, nullptr, &ptau, nullptr)) return st;
    if (frames == 0) return ST_OK;
    PtrackCfg cfg;
    bool unsup = false;
    if (int st = ptrack_params(track, &cfg, &unsup)) return st;
    const size_t curve = ptau + 1;   // the row stride of the scratch curves
    if (curve < (size_t)track->tau_max + 1) return fail(ST_SIZE, "pitch_track_frames: tau_max above the curves' last lag");
    if (nch > 1 && (ch_stride < n || ((o->lag || o->f0 || o->aperiodicity) && out_ch_stride < frames)))
        return fail(ST_SIZE, "pitch_track_frames: a channel stride shorter than its channel");
    if (unsup || frames >= ((size_t)1 << 31) || nch >= ((size_t)1 << 31)) return ptrack_unsupported();
    if (!ptrack_any(o) || nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (n == 0) return ST_SIZE;
    hipStream_t s = (hipStream_t)stream;
    const size_t per_ch = frames * curve;   // floats
    size_t group = PTRACK_CURVE_BYTES / (per_ch * sizeof(float));
    const long long forced = knob(KNOB_PTRACK_GROUP, 0);
    if (forced > 0) group = (size_t)forced;
    group = group < 1 ? 1 : group > nch ? nch : group;
    Scratch curves(s);
    HIPCHK(curves.alloc(group * per_ch * sizeof(float)), ST_INTERNAL);
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const size_t g = nch - c0 < group ? nch - c0 : group;
        const vvhip_pitch_out po = {nullptr, nullptr, nullptr, (float*)curves.p};
        if (int st = vvhip_pitch_frames_device(d_signal + c0 * ch_stride, n, g, ch_stride, frame_len, hop, frames,
                                               center, d_window, pitch, &po, 0, per_ch, stream))
            return st;
        const vvhip_pitch_track_out go = {o->lag ? o->lag + c0 * out_ch_stride : nullptr,
                                          o->f0 ? o->f0 + c0 * out_ch_stride : nullptr,
                                          o->aperiodicity ? o->aperiodicity + c0 * out_ch_stride : nullptr,
                                          o->cost ? o->cost + c0 : nullptr};
        if (int st = ptrack_run(cfg, (const float*)curves.p, frames, g, curve, per_ch, &go, out_ch_stride, s)) return st;
    }
    return ST_OK;
}

// One channel of curves in host memory: the tau_max + 1 values of each row go up.
int vvhip_pitch_track_host(const float* curves, size_t frames, size_t row_stride,
                           const vvhip_pitch_track_params* params, const vvhip_pitch_track_out* o) {
    if (!curves || !params || !o) return ST_NULL;
    if (frames == 0) return ST_OK;
    PtrackCfg cfg;
    bool unsup = false;
    if (int st = ptrack_params(params, &cfg, &unsup)) return st;
    const size_t curve = (size_t)params->tau_max + 1;
    if (row_stride < curve) return fail(ST_SIZE, "pitch_track: a row stride below tau_max + 1");
    if (unsup || frames >= ((size_t)1 << 31)) return ptrack_unsupported();
    if (!ptrack_any(o)) return ST_OK;
    HostCall c("pitch_track");
    if (!c.ok()) return c.st;
    std::vector<float> packed;
    const float* up = curves;
    if (row_stride != curve) {
        packed.resize(frames * curve);
        for (size_t t = 0; t < frames; ++t)
            for (size_t i = 0; i < curve; ++i) packed[t * curve + i] = curves[t * row_stride + i];
        up = packed.data();
    }
    const float* dq = (const float*)c.in(up, sizeof(float) * frames * curve);
    // one buffer for the three planes (4 bytes a value), one for the cost
    uint32_t* planes = (uint32_t*)c.out(nullptr, sizeof(uint32_t) * 3 * frames);
    double* dcost = (double*)c.out(o->cost, sizeof(double));
    if (!c.ok()) return c.st;
    const vvhip_pitch_track_out dev = {o->lag ? planes : nullptr, o->f0 ? (float*)(planes + frames) : nullptr,
                                       o->aperiodicity ? (float*)(planes + 2 * frames) : nullptr,
                                       o->cost ? dcost : nullptr};
    int st = vvhip_pitch_track_device(dq, frames, 1, curve, frames * curve, params, &dev, frames, c.s);
    if (st == ST_OK) {
        hipError_t e = hipSuccess;
        if (o->lag) e = hipMemcpyAsync(o->lag, planes, 4 * frames, hipMemcpyDeviceToHost, c.s);
        if (e == hipSuccess && o->f0) e = hipMemcpyAsync(o->f0, planes + frames, 4 * frames, hipMemcpyDeviceToHost, c.s);
        if (e == hipSuccess && o->aperiodicity)
            e = hipMemcpyAsync(o->aperiodicity, planes + 2 * frames, 4 * frames, hipMemcpyDeviceToHost, c.s);
        if (e != hipSuccess) st = fail(ST_INTERNAL, "pitch_track: copy down", e);
    }
    return c.finish(st);
}

}  // extern "C"
