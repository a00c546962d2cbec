// shim_stats.hip -- array statistics and lagged correlations (src/core/core.c:42-108,
// src/core/stats.c:10-139): the entry points over stats_kernels.hip.  Rows or
// frames of up to STATS_WAVE_LEN (16384) samples take the wave kernel, one wave
// per row; longer ones take the long route, one wave per chunk of STATS_CHUNK
// (4096) samples through a scratch buffer; knob STATS_LONG = 1 forces it.  Both
// give the same bits.  STAT_STATS_WAVE / STAT_STATS_LONG count which ran.
#include "shim_common.hpp"

#include <cstring>

using namespace vvh;

static bool stats_long(long long len) { return knob(KNOB_STATS_LONG, 0) == 1 || len > STATS_WAVE_LEN; }

// the size rule of every requested output (core.c:67, stats.c:63, :84)
static bool stats_len_ok(unsigned mask, size_t len) {
    if (len == 0) return false;
    if ((mask & (1u << STATS_VAR)) && len < 2) return false;
    if ((mask & (1u << STATS_SKEW)) && len < 3) return false;
    if ((mask & (1u << STATS_KURT)) && len < 4) return false;
    return true;
}

static StatsOut stats_out(const vvhip_stats_out* o, size_t ch_stride) {
    StatsOut out;
    void* const p[STATS_NOUT] = {o->sum, o->mean, o->var,   o->rms,      o->min,           o->max,
                                 o->crest, o->skewness, o->kurtosis, o->zero_crossings, o->argmin, o->argmax};
    for (int k = 0; k < STATS_NOUT; ++k) out.p[k] = p[k];
    out.ch_stride = (long long)ch_stride;
    return out;
}

static int stats_run(const FrameSrc& src, const StatsOut& out, hipStream_t s) {
    if (!stats_long(src.len)) {
        HIPCHK(launch_stats_wave(src, out, s), ST_INTERNAL);
        stat_inc(STAT_STATS_WAVE);
        return ST_OK;
    }
    const size_t chunks = (size_t)((src.len + STATS_CHUNK - 1) / STATS_CHUNK);
    if ((size_t)src.rows * chunks >= ((size_t)1 << 32)) return fail(ST_SIZE, "stats: too many chunks for one call");
    Scratch parts(s), totals(s);
    HIPCHK(parts.alloc((size_t)src.rows * chunks * stats_part_bytes()), ST_INTERNAL);
    HIPCHK(totals.alloc((size_t)src.rows * stats_total_bytes()), ST_INTERNAL);
    HIPCHK(launch_stats_long(src, out, parts.p, totals.p, s), ST_INTERNAL);
    stat_inc(STAT_STATS_LONG);
    return ST_OK;
}

extern "C" {

int vvhip_stats_device(const float* d_x, size_t n, size_t batch, size_t row_stride, const vvhip_stats_out* o,
                       void* stream) {
    if (!d_x || !o) return ST_NULL;
    const StatsOut out = stats_out(o, 0);
    const unsigned mask = out.mask();
    if (mask == 0) return ST_OK;
    if (!stats_len_ok(mask, n)) return ST_SIZE;
    if (n >= ((size_t)1 << 32) || batch >= ((size_t)1 << 31)) return fail(ST_SIZE, "stats: n >= 2^32 or batch >= 2^31");
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (batch == 0) return ST_OK;
    return stats_run(rows_src(d_x, n, batch, row_stride), out, (hipStream_t)stream);
}

int vvhip_stats_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                              size_t hop, size_t frames, int center, const float* d_window, const vvhip_stats_out* o,
                              size_t out_ch_stride, void* stream) {
    if (!d_signal || !o) return ST_NULL;
    const FramesCall fc = {"stats_frames", n, nch, frame_len, hop, frames};
    if (int st = fc.shape()) return st;
    const StatsOut out = stats_out(o, out_ch_stride);
    const unsigned mask = out.mask();
    if (mask == 0) return ST_OK;
    if (!stats_len_ok(mask, frame_len)) return ST_SIZE;
    if (int st = fc.limits()) return st;
    int st;
    if (!fc.start(&st)) return st;
    return stats_run(frames_src(d_signal, n, nch, ch_stride, frame_len, hop, frames, center, d_window), out,
                     (hipStream_t)stream);
}

int vvhip_cross_correlation_device(const float* d_x, size_t nx, const float* d_y, size_t ny, size_t batch,
                                   size_t r_len, int biased, float* d_r, void* stream) {
    if (!d_x || !d_y || !d_r || nx == 0 || ny == 0) return ST_NULL;
    if (r_len == 0) return ST_SIZE;
    if (nx >= ((size_t)1 << 32) || ny >= ((size_t)1 << 32) || r_len >= ((size_t)1 << 31) ||
        batch >= ((size_t)1 << 31) || batch * r_len >= ((size_t)1 << 31))
        return fail(ST_SIZE, "correlation: n >= 2^32 or batch * r_len >= 2^31");
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (batch == 0) return ST_OK;
    HIPCHK(launch_xcorr(d_x, (long long)nx, d_y, (long long)ny, (long long)batch, (long long)r_len, biased != 0, d_r,
                        (hipStream_t)stream),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_autocorrelation_device(const float* d_x, size_t n, size_t batch, size_t r_len, int biased, float* d_r,
                                 void* stream) {
    return vvhip_cross_correlation_device(d_x, n, d_x, n, batch, r_len, biased, d_r, stream);
}

// One row in host memory: the outputs of `mask` (bit k = member k of
// vvhip_stats_out) into vals[k] (k < 9) and idx[k - 9], the others untouched.
int vvhip_stats_host(const float* x, size_t n, unsigned mask, float* vals, size_t* idx) {
    if (!x || n == 0 || (!vals && (mask & ((1u << STATS_NFLOAT) - 1))) || (!idx && (mask >> STATS_NFLOAT)))
        return ST_NULL;
    mask &= (1u << STATS_NOUT) - 1;
    if (mask == 0) return ST_OK;
    if (!stats_len_ok(mask, n)) return ST_SIZE;
    if (n >= ((size_t)1 << 32)) return fail(ST_SIZE, "stats: n >= 2^32");
    HostCall c("stats");
    uint32_t res[STATS_NOUT];   // floats [0, 9) by their bits, then the three counts
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    uint32_t* dres = (uint32_t*)c.out(res, sizeof res);
    if (!c.ok()) return c.st;
    void* p[STATS_NOUT];
    for (int k = 0; k < STATS_NOUT; ++k) p[k] = (mask >> k & 1) ? (void*)(dres + k) : nullptr;
    const vvhip_stats_out o = {(float*)p[0], (float*)p[1], (float*)p[2],    (float*)p[3],    (float*)p[4],   (float*)p[5],
                               (float*)p[6], (float*)p[7], (float*)p[8], (unsigned*)p[9], (unsigned*)p[10],
                               (unsigned*)p[11]};
    const int st = c.finish(vvhip_stats_device(dx, n, 1, n, &o, c.s));
    if (st != ST_OK) return st;
    for (int k = 0; k < STATS_NOUT; ++k) {
        if (!(mask >> k & 1)) continue;
        if (k < STATS_NFLOAT) std::memcpy(&vals[k], &res[k], sizeof(float));
        else idx[k - STATS_NFLOAT] = (size_t)res[k];
    }
    return ST_OK;
}

int vvhip_cross_correlation_host(const float* x, size_t nx, const float* y, size_t ny, float* r, size_t r_len,
                                 int biased) {
    if (!x || !y || !r || nx == 0 || ny == 0) return ST_NULL;
    if (r_len == 0) return ST_SIZE;
    HostCall c("correlation");
    const float* dx = (const float*)c.in(x, sizeof(float) * nx);
    const float* dy = y == x && ny == nx ? dx : (const float*)c.in(y, sizeof(float) * ny);
    float* dr = (float*)c.out(r, sizeof(float) * r_len);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_cross_correlation_device(dx, nx, dy, ny, 1, r_len, biased, dr, c.s));
}

}  // extern "C"
