// shim_shape.hip -- per-frame spectral shape descriptors
// (include/vv_dsp/features/spectral_shape.h): the entry points over
// shape_kernels.hip.  Every check is made before any device work, in this
// order: null pointers; n_fft < 2 or a row pitch below n_fft/2 + 1; the band;
// sample_rate, floor and rolloff; the kernel's limit (8193 bins); no output
// wanted (OK, nothing launched); the counts one launch takes.  One kernel, one
// wave per run of rows; STAT_SHAPE_WAVE counts its launches, STAT_SHAPE_VEC16
// those that load 16 bytes at a time.  Knob SHAPE_DWORD
// = 1 loads the rows 4 bytes at a time wherever they lie (same bits; for timing
// the two paths and for the test of equal bits).
#include "shim_common.hpp"

#include <cmath>
#include <cstring>

using namespace vvh;

// checks 2 to 5 of the header (row_pitch 0: no rows to step over)
static int shape_cfg(const vvhip_shape_params* p, size_t row_pitch, bool pitched, ShapeCfg* cfg) {
    if (p->n_fft < 2) return fail(ST_SIZE, "spectral_shape: n_fft below 2");
    const size_t K = p->n_fft / 2 + 1;
    if (pitched && row_pitch < K) return fail(ST_SIZE, "spectral_shape: row pitch below n_fft/2+1");
    if (p->k_min > p->k_max || p->k_max > p->n_fft / 2) return fail(ST_RANGE, "spectral_shape: band outside the row");
    const double fs = (double)p->sample_rate, fl = (double)p->floor, ro = (double)p->rolloff;
    if (!(std::isfinite(fs) && fs > 0.0)) return fail(ST_RANGE, "spectral_shape: sample_rate must be finite and positive");
    if (!(std::isfinite(fl) && fl > 0.0)) return fail(ST_RANGE, "spectral_shape: floor must be finite and positive");
    if (!(ro > 0.0 && ro <= 1.0)) return fail(ST_RANGE, "spectral_shape: rolloff outside (0, 1]");
    if (K > (size_t)SHAPE_MAX_BINS) return fail(ST_UNSUP, "spectral_shape: rows above 8193 bins");
    cfg->K = (int)K;
    cfg->k_min = (int)p->k_min;
    cfg->k_max = (int)p->k_max;
    cfg->magnitude = p->magnitude != 0;
    cfg->sample_rate = fs;
    cfg->n_fft = (double)p->n_fft;
    cfg->rolloff = ro;
    cfg->floor = p->floor;
    return ST_OK;
}

static ShapeOut shape_out(const vvhip_shape_out* o) {
    ShapeOut out;
    out.p[SHAPE_ENERGY] = o->energy;
    out.p[SHAPE_CENTROID] = o->centroid;
    out.p[SHAPE_SPREAD] = o->spread;
    out.p[SHAPE_SKEW] = o->skewness;
    out.p[SHAPE_KURT] = o->kurtosis;
    out.p[SHAPE_FLATNESS] = o->flatness;
    out.p[SHAPE_ROLLOFF] = o->rolloff;
    out.p[SHAPE_FLUX] = o->flux;
    out.p[SHAPE_CREST] = o->crest;
    out.p[SHAPE_PEAK] = o->peak_bin;
    return out;
}

static int shape_run(const float* d_power, size_t rows, size_t row_pitch, size_t rpg, const ShapeCfg& cfg,
                     const ShapeOut& out, hipStream_t s) {
    const bool dword = knob(KNOB_SHAPE_DWORD, 0) == 1;
    HIPCHK(launch_shape(d_power, (long long)rows, (long long)row_pitch, (long long)rpg, cfg, out, dword, s),
           ST_INTERNAL);
    stat_inc(STAT_SHAPE_WAVE);
    if (!dword && shape_rows_vec16(d_power, (long long)row_pitch)) stat_inc(STAT_SHAPE_VEC16);
    return ST_OK;
}

extern "C" {

int vvhip_shape_device(const float* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                       const vvhip_shape_params* params, const vvhip_shape_out* o, void* stream) {
    if (!params || !d_power || !o) return ST_NULL;
    ShapeCfg cfg;
    if (int st = shape_cfg(params, row_pitch, true, &cfg)) return st;
    ShapeOut out = shape_out(o);
    if (!out.mask()) return ST_OK;
    if (rows >= ((size_t)1 << 31) || row_pitch >= ((size_t)1 << 31))
        return fail(ST_SIZE, "spectral_shape: rows or pitch >= 2^31");
    if (rows == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    const size_t rpg = rows_per_group == 0 || rows_per_group > rows ? rows : rows_per_group;
    out.group_stride = (long long)rpg;
    return shape_run(d_power, rows, row_pitch, rpg, cfg, out, (hipStream_t)stream);
}

int vvhip_stft_shape_device(vvhip_stft* h, const vvhip_shape_params* params, const float* d_signal, size_t n,
                            size_t nch, size_t ch_stride, const vvhip_shape_out* o, size_t out_ch_stride,
                            void* stream) {
    if (!h || !params || !d_signal || !o) return ST_NULL;
    if (params->n_fft < 2) return fail(ST_SIZE, "spectral_shape: n_fft below 2");
    if (params->n_fft != h->nfft) return fail(ST_SIZE, "spectral_shape: n_fft differs from the stft's fft_size");
    ShapeCfg cfg;
    if (int st = shape_cfg(params, 0, false, &cfg)) return st;
    ShapeOut out = shape_out(o);
    if (!out.mask()) return ST_OK;
    const size_t frames = vvhip_stft_num_frames(n, h->nfft, h->hop);
    if (out_ch_stride < frames || (nch > 1 && ch_stride < n))
        return fail(ST_SIZE, "stft_spectral_shape: a channel stride shorter than its channel");
    if (nch >= ((size_t)1 << 31) || frames >= ((size_t)1 << 31) || nch * frames >= ((size_t)1 << 31))
        return fail(ST_SIZE, "stft_spectral_shape: too many frames for one call");
    if (nch == 0 || frames == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    const hipStream_t s = (hipStream_t)stream;
    // rows of whole 128 B lines (544 floats for n_fft 1024), as the power kernel stores them best
    const size_t pitch = ((size_t)cfg.K + 31) / 32 * 32;
    Scratch pw(s);
    HIPCHK(pw.alloc(sizeof(float) * nch * frames * pitch), ST_INTERNAL);
    if (int st = vvhip_stft_power_pitched_device(h, d_signal, n, nch, ch_stride, (float*)pw.p, frames * pitch, pitch,
                                                 stream))
        return st;
    out.group_stride = (long long)out_ch_stride;
    return shape_run((const float*)pw.p, nch * frames, pitch, frames, cfg, out, s);
}

// One row in host memory (and its predecessor, or null) through the same kernel.
int vvhip_shape_host(const float* row, const float* prev, const vvhip_shape_params* params, vvhip_shape_values* res) {
    if (!params || !row || !res) return ST_NULL;
    ShapeCfg cfg;
    if (int st = shape_cfg(params, 0, false, &cfg)) return st;
    HostCall c("spectral_shape");
    const size_t K = (size_t)cfg.K, nrows = prev ? 2 : 1;
    float vals[2 * SHAPE_NOUT];   // plane k: vals[k * nrows + r]; the peak bin's bits in the last plane
    float* drows = (float*)c.out(nullptr, sizeof(float) * K * nrows);
    float* dres = (float*)c.out(vals, sizeof(float) * SHAPE_NOUT * nrows);
    if (!c.ok()) return c.st;
    if (prev) HIPCHK(hipMemcpyAsync(drows, prev, sizeof(float) * K, hipMemcpyHostToDevice, c.s), ST_INTERNAL);
    HIPCHK(hipMemcpyAsync(drows + (nrows - 1) * K, row, sizeof(float) * K, hipMemcpyHostToDevice, c.s), ST_INTERNAL);
    vvhip_shape_out o;
    float** planes[] = {&o.energy, &o.centroid, &o.spread, &o.skewness, &o.kurtosis,
                        &o.flatness, &o.rolloff, &o.flux, &o.crest};
    for (int k = 0; k < SHAPE_PEAK; ++k) *planes[k] = dres + k * nrows;
    o.peak_bin = (uint32_t*)(dres + SHAPE_PEAK * nrows);
    const int st = c.finish(vvhip_shape_device(drows, nrows, K, nrows, params, &o, c.s));
    if (st != ST_OK) return st;
    const float* v = vals + (nrows - 1);
    res->energy = v[SHAPE_ENERGY * nrows];
    res->centroid = v[SHAPE_CENTROID * nrows];
    res->spread = v[SHAPE_SPREAD * nrows];
    res->skewness = v[SHAPE_SKEW * nrows];
    res->kurtosis = v[SHAPE_KURT * nrows];
    res->flatness = v[SHAPE_FLATNESS * nrows];
    res->rolloff = v[SHAPE_ROLLOFF * nrows];
    res->flux = v[SHAPE_FLUX * nrows];
    res->crest = v[SHAPE_CREST * nrows];
    std::memcpy(&res->peak_bin, &v[SHAPE_PEAK * nrows], sizeof(uint32_t));
    return ST_OK;
}

}  // extern "C"
