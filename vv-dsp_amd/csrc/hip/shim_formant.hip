// shim_formant.hip -- formants of LPC rows (include/vv_dsp/features/formant.h):
// the entry points over formant_kernels.hip.  Every check is made before any
// device work, in the header's order: null pointers or no output wanted; order
// < 1 or a pitch below order + 1; the parameters' ranges; order above 32; then no
// rows (OK) and no device.  STAT_FORMANT counts the launches.  The fused entry
// goes through scratch LPC rows in groups of channels as shim_lsf.hip does.
#include "shim_common.hpp"

#include <cmath>

using namespace vvh;

#pragma clang fp contract(off)

static bool formant_any(const vvhip_formant_out* o) { return o->freq || o->bw || o->count || o->flags || o->roots; }

// checks 2-4 of the header; fills cfg
static int formant_checks(size_t order, size_t pitch, size_t batch, const vvhip_formant_params* p, FormantCfg* cfg) {
    if (order < 1 || pitch < order + 1) return ST_SIZE;
    const double fs = (double)p->sample_rate, lo = (double)p->f_min, hi = (double)p->f_max, bw = (double)p->bw_max;
    if (!(std::isfinite(fs) && fs > 0.0)) return fail(ST_RANGE, "formants: sample_rate must be finite and positive");
    if (std::isnan(lo) || std::isnan(hi) || std::isnan(bw) || lo > hi)
        return fail(ST_RANGE, "formants: a NaN threshold or f_min above f_max");
    if (p->n_formants < 1 || p->n_formants > 16) return fail(ST_RANGE, "formants: n_formants outside 1..16");
    if (order > (size_t)LSF_MAX_ORDER) return fail(ST_UNSUP, "formants: order above 32");
    if (batch >= ((size_t)1 << 31) || pitch >= ((size_t)1 << 31))
        return fail(ST_SIZE, "formants: batch or pitch >= 2^31");
    cfg->sample_rate = fs;
    cfg->f_min = lo;
    cfg->f_max = hi;
    cfg->bw_max = bw;
    cfg->n_formants = (int)p->n_formants;
    for (double& v : cfg->start) v = 0.0;
    return vvhip_formant_start_points(order, cfg->start);
}

extern "C" {

int vvhip_formant_params_default(float sample_rate, vvhip_formant_params* params) {
    if (!params) return ST_NULL;
    params->sample_rate = sample_rate;
    params->f_min = 50.0f;
    params->f_max = sample_rate / 2.0f - 50.0f;
    params->bw_max = 600.0f;
    params->n_formants = 5;
    return ST_OK;
}

int vvhip_formant_start_points(size_t order, double* out) {
    if (!out) return ST_NULL;
    if (order < 1 || order > (size_t)LSF_MAX_ORDER) return fail(ST_RANGE, "formant_start_points: order outside 1..32");
    for (size_t i = 0; i < order; ++i) {
        const double t = (6.283185307179586 * (double)i) / (double)order + 0.4;
        out[2 * i] = 0.9 * std::cos(t);
        out[2 * i + 1] = 0.9 * std::sin(t);
    }
    return ST_OK;
}

int vvhip_lpc_formants_device(const float* d_a, size_t order, size_t batch, size_t a_pitch,
                              const vvhip_formant_params* params, const vvhip_formant_out* o, void* stream) {
    if (!d_a || !params || !o || !formant_any(o)) return ST_NULL;
    FormantCfg cfg;
    if (int st = formant_checks(order, a_pitch, batch, params, &cfg)) return st;
    if (batch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    FormantOut out;
    out.freq = o->freq;
    out.bw = o->bw;
    out.count = o->count;
    out.flags = o->flags;
    out.roots = o->roots;
    HIPCHK(launch_formants(d_a, (int)order, (long long)batch, (long long)a_pitch, cfg, out, (hipStream_t)stream),
           ST_INTERNAL);
    stat_inc(STAT_FORMANT);
    return ST_OK;
}

int vvhip_formants_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                                 size_t hop, size_t frames, int center, const float* d_window, size_t order,
                                 const vvhip_formant_params* params, const vvhip_formant_out* o, void* stream) {
    if (!d_signal || !params || !o || !formant_any(o)) return ST_NULL;
    if (hop == 0 || frame_len == 0 || order + 1 > frame_len) return ST_SIZE;
    FormantCfg cfg;
    if (int st = formant_checks(order, order + 1, 0, params, &cfg)) return st;
    if (frames == 0 || nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    hipStream_t s = (hipStream_t)stream;
    const size_t w = order + 1, a_ch = frames * w, nf = params->n_formants;
    const size_t group = lsf_group((a_ch + frames) * sizeof(float), nch);
    Scratch rows(s);
    HIPCHK(rows.alloc(group * (a_ch + frames) * sizeof(float)), ST_INTERNAL);
    float* sa = (float*)rows.p;
    float* serr = sa + group * a_ch;
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const size_t g = nch - c0 < group ? nch - c0 : group, r0 = c0 * frames;
        if (int st = vvhip_lpc_frames_device(d_signal + c0 * ch_stride, n, g, ch_stride, frame_len, hop, frames, center,
                                             d_window, order, sa, a_ch, serr, frames, stream))
            return st;
        const vvhip_formant_out go = {o->freq ? o->freq + r0 * nf : nullptr, o->bw ? o->bw + r0 * nf : nullptr,
                                      o->count ? o->count + r0 : nullptr, o->flags ? o->flags + r0 : nullptr,
                                      o->roots ? o->roots + r0 * order * 2 : nullptr};
        if (int st = vvhip_lpc_formants_device(sa, order, g * frames, w, params, &go, stream)) return st;
    }
    return ST_OK;
}

// One row in host memory.  One device buffer holds every plane: roots, freq, bw,
// count, flags in that order (the doubles first).
int vvhip_lpc_formants_host(const float* a, size_t order, const vvhip_formant_params* params,
                            const vvhip_formant_out* o) {
    if (!a || !params || !o || !formant_any(o)) return ST_NULL;
    FormantCfg cfg;
    if (int st = formant_checks(order, order + 1, 1, params, &cfg)) return st;
    HostCall c("lpc_formants");
    const size_t nf = params->n_formants;
    const float* da = (const float*)c.in(a, sizeof(float) * (order + 1));
    double* droots = (double*)c.out(nullptr, sizeof(double) * 2 * order + sizeof(float) * (2 * nf + 2));
    if (!c.ok()) return c.st;
    float* dfreq = (float*)(droots + 2 * order);
    float* dbw = dfreq + nf;
    int32_t* dcount = (int32_t*)(dbw + nf);
    int32_t* dflags = dcount + 1;
    const vvhip_formant_out dev = {o->freq ? dfreq : nullptr, o->bw ? dbw : nullptr, o->count ? dcount : nullptr,
                                   o->flags ? dflags : nullptr, o->roots ? droots : nullptr};
    int st = vvhip_lpc_formants_device(da, order, 1, order + 1, params, &dev, c.s);
    if (st == ST_OK) {
        hipError_t e = hipSuccess;
        if (o->roots) e = hipMemcpyAsync(o->roots, droots, sizeof(double) * 2 * order, hipMemcpyDeviceToHost, c.s);
        if (e == hipSuccess && o->freq) e = hipMemcpyAsync(o->freq, dfreq, 4 * nf, hipMemcpyDeviceToHost, c.s);
        if (e == hipSuccess && o->bw) e = hipMemcpyAsync(o->bw, dbw, 4 * nf, hipMemcpyDeviceToHost, c.s);
        if (e == hipSuccess && o->count) e = hipMemcpyAsync(o->count, dcount, 4, hipMemcpyDeviceToHost, c.s);
        if (e == hipSuccess && o->flags) e = hipMemcpyAsync(o->flags, dflags, 4, hipMemcpyDeviceToHost, c.s);
        if (e != hipSuccess) st = fail(ST_INTERNAL, "lpc_formants: copy down", e);
    }
    return c.finish(st);
}

}  // extern "C"
