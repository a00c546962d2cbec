// shim_lpc_filter.hip -- the LPC residual and synthesis filters
// (include/vv_dsp/envelope/lpc_filter.h): the entry points over
// lpc_filter_kernels.hip.  Every check is made before any device work, in the
// header's order: null pointers; order < 1, seg_len == 0, frames == 0, a pitch or
// stride shorter than its row; order above 32; sizes one call cannot address;
// then nothing to do (OK) and no device.
//
// Route rule of the synthesis, a function of n alone (never of the batch, the
// strides or the entry point): rows of n <= LPCF_EXACT_MAX run as one recursion
// per row; longer rows are cut into chunks of LPCF_CHUNK samples and take the
// three launches of lpc_filter_kernels.hip.  Knob LPC_SYNTH_CHUNK: 0 never
// chunks, k > 0 forces chunks of k samples; a chunk length >= n is the exact
// route.  STAT_LPC_RESIDUAL / STAT_LPC_SYNTH_EXACT / STAT_LPC_SYNTH_CHUNKED count
// the calls of each route.
//
// Scratch.  The chunked route keeps 8 p (p + 2) bytes per chunk (the transition,
// the zero-state end values, the incoming state): channels go in groups of at
// most LPCF_SCRATCH_BYTES (1 GiB), at least one channel.  The _frames_ call
// writes the LPC rows the caller does not take to scratch in the same way.  Rows
// are independent, so no value depends on the grouping; knob LPC_FILTER_GROUP =
// g > 0 forces groups of g channels, for the tests that cross a boundary.
#include "shim_common.hpp"

using namespace vvh;

static constexpr size_t LPCF_SCRATCH_BYTES = (size_t)1 << 30;
static constexpr size_t LPCF_LIMIT = (size_t)1 << 40;

// chunk length of rows of n samples; 0: one recursion per row
static long long lpcf_chunk_len(size_t n) {
    const long long k = knob(KNOB_LPC_SYNTH_CHUNK, -1);
    const long long L = k >= 0 ? k : ((long long)n <= LPCF_EXACT_MAX ? 0 : LPCF_CHUNK);
    return L >= (long long)n ? 0 : L;
}

static size_t lpcf_group(size_t per_ch, size_t nch) {
    size_t group = LPCF_SCRATCH_BYTES / (per_ch ? per_ch : 1);
    const long long forced = knob(KNOB_LPC_FILTER_GROUP, 0);
    if (forced > 0) group = (size_t)forced;
    return group < 1 ? 1 : group > nch ? nch : group;
}

// the size checks of the two filters, in the header's order
static int lpcf_sizes(size_t n, size_t nch, size_t in_stride, size_t out_stride, size_t order, size_t frames,
                      size_t a_pitch, size_t a_ch_stride, bool gain, size_t g_ch_stride, size_t seg_len,
                      long long offset) {
    if (order < 1 || seg_len == 0 || frames == 0) return ST_SIZE;
    if (a_pitch < order + 1 || in_stride < n || out_stride < n) return ST_SIZE;
    if (a_ch_stride && (a_ch_stride < order + 1 || (a_ch_stride - (order + 1)) / a_pitch < frames - 1)) return ST_SIZE;
    if (gain && g_ch_stride && g_ch_stride < frames) return ST_SIZE;
    if (order > (size_t)LPCF_MAX_ORDER) return fail(ST_UNSUP, "lpc filter: order above 32");
    if (n >= ((size_t)1 << 31) - 64 || nch >= ((size_t)1 << 31) || frames >= ((size_t)1 << 31) ||
        a_pitch >= ((size_t)1 << 31) || seg_len >= LPCF_LIMIT || offset <= -(long long)LPCF_LIMIT ||
        offset >= (long long)LPCF_LIMIT)
        return fail(ST_SIZE, "lpc filter: n, channels, frames or pitch >= 2^31, or seg_len or |offset| >= 2^40");
    return ST_OK;
}

static LpcFilt lpcf_args(const float* d_in, size_t n, size_t nch, size_t in_stride, const float* d_a, size_t order,
                         size_t frames, size_t a_pitch, size_t a_ch_stride, const float* d_gain, size_t g_ch_stride,
                         size_t seg_len, long long offset, double* d_state, float* d_out, size_t out_stride) {
    LpcFilt f;
    f.x = d_in;
    f.y = d_out;
    f.n = (long long)n;
    f.rows = (long long)nch;
    f.x_stride = (long long)in_stride;
    f.y_stride = (long long)out_stride;
    f.a = d_a;
    f.gain = d_gain;
    f.frames = (long long)frames;
    f.a_pitch = (long long)a_pitch;
    f.a_ch_stride = (long long)a_ch_stride;
    f.g_ch_stride = (long long)g_ch_stride;
    f.seg_len = (long long)seg_len;
    f.offset = offset;
    f.order = (int)order;
    f.state = d_state;
    return f;
}

// channels [c0, c0 + g) of f
static LpcFilt lpcf_channels(const LpcFilt& f, size_t c0, size_t g) {
    LpcFilt s = f;
    s.x += (long long)c0 * f.x_stride;
    s.y += (long long)c0 * f.y_stride;
    s.a += (long long)c0 * f.a_ch_stride;
    if (s.gain) s.gain += (long long)c0 * f.g_ch_stride;
    if (s.state) s.state += (long long)c0 * f.order;
    s.rows = (long long)g;
    return s;
}

extern "C" {

int vvhip_lpc_residual_device(const float* d_x, size_t n, size_t nch, size_t x_stride, const float* d_a, size_t order,
                              size_t frames, size_t a_pitch, size_t a_ch_stride, const float* d_gain,
                              size_t g_ch_stride, size_t seg_len, long long offset, double* d_state, float* d_e,
                              size_t e_stride, void* stream) {
    if (!d_x || !d_a || !d_e) return ST_NULL;
    if (int st = lpcf_sizes(n, nch, x_stride, e_stride, order, frames, a_pitch, a_ch_stride, d_gain != nullptr,
                            g_ch_stride, seg_len, offset))
        return st;
    if (n == 0 || nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    const LpcFilt f = lpcf_args(d_x, n, nch, x_stride, d_a, order, frames, a_pitch, a_ch_stride, d_gain, g_ch_stride,
                                seg_len, offset, d_state, d_e, e_stride);
    // one launch takes 2^31 - 1 tiles
    const size_t tiles = (n + LPCF_TILE - 1) / LPCF_TILE;
    const size_t group = ((size_t)0x7fffffff / tiles) < nch ? (size_t)0x7fffffff / tiles : nch;
    for (size_t c0 = 0; c0 < nch; c0 += group)
        HIPCHK(launch_lpc_residual(lpcf_channels(f, c0, nch - c0 < group ? nch - c0 : group), (hipStream_t)stream),
               ST_INTERNAL);
    stat_inc(STAT_LPC_RESIDUAL);
    return ST_OK;
}

int vvhip_lpc_synth_device(const float* d_e, size_t n, size_t nch, size_t e_stride, const float* d_a, size_t order,
                           size_t frames, size_t a_pitch, size_t a_ch_stride, const float* d_gain, size_t g_ch_stride,
                           size_t seg_len, long long offset, double* d_state, float* d_y, size_t y_stride,
                           void* stream) {
    if (!d_e || !d_a || !d_y) return ST_NULL;
    if (int st = lpcf_sizes(n, nch, e_stride, y_stride, order, frames, a_pitch, a_ch_stride, d_gain != nullptr,
                            g_ch_stride, seg_len, offset))
        return st;
    if (n == 0 || nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    hipStream_t s = (hipStream_t)stream;
    const LpcFilt f = lpcf_args(d_e, n, nch, e_stride, d_a, order, frames, a_pitch, a_ch_stride, d_gain, g_ch_stride,
                                seg_len, offset, d_state, d_y, y_stride);
    const long long L = lpcf_chunk_len(n);
    if (!L) {
        HIPCHK(launch_lpc_synth_walk(f, 1, (long long)n, nullptr, s), ST_INTERNAL);
        stat_inc(STAT_LPC_SYNTH_EXACT);
        return ST_OK;
    }
    const size_t chunks = (n + (size_t)L - 1) / (size_t)L;
    const size_t per_chunk = sizeof(double) * order * (order + 2);
    size_t group = lpcf_group(chunks * per_chunk, nch);
    if (group * chunks > (size_t)0x7fffffff) group = (size_t)0x7fffffff / chunks;
    if (group < 1) return fail(ST_SIZE, "lpc synth: too many chunks for one call");
    Scratch work(s);
    HIPCHK(work.alloc(group * chunks * per_chunk), ST_INTERNAL);
    double* phi = (double*)work.p;
    double* z = phi + group * chunks * order * order;
    double* zin = z + group * chunks * order;
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const LpcFilt g = lpcf_channels(f, c0, nch - c0 < group ? nch - c0 : group);
        HIPCHK(launch_lpc_synth_phi(g, (long long)chunks, L, phi, z, s), ST_INTERNAL);
        HIPCHK(launch_lpc_synth_scan(g, (long long)chunks, phi, z, zin, s), ST_INTERNAL);
        HIPCHK(launch_lpc_synth_walk(g, (long long)chunks, L, zin, s), ST_INTERNAL);
    }
    stat_inc(STAT_LPC_SYNTH_CHUNKED);
    return ST_OK;
}

int vvhip_lpc_residual_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                                     size_t hop, size_t frames, int center, const float* d_window, size_t order,
                                     float* d_a, size_t a_ch_stride, float* d_err, size_t err_ch_stride, float* d_e,
                                     size_t e_stride, void* stream) {
    if (!d_signal || !d_e) return ST_NULL;
    if (hop == 0 || frame_len == 0 || order < 1 || order + 1 > frame_len) return ST_SIZE;
    const size_t w = order + 1;
    if ((d_a && (a_ch_stride < w || (a_ch_stride - w) / w + 1 < frames)) || (d_err && err_ch_stride < frames) ||
        ch_stride < n || e_stride < n)
        return ST_SIZE;
    if (order > (size_t)LPCF_MAX_ORDER) return fail(ST_UNSUP, "lpc filter: order above 32");
    if (frames == 0 || nch == 0 || n == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    hipStream_t s = (hipStream_t)stream;
    const size_t a_ch = frames * w;   // floats of scratch coefficient rows per channel
    const size_t per_ch = ((d_a ? 0 : a_ch) + (d_err ? 0 : frames)) * sizeof(float);
    const size_t group = per_ch ? lpcf_group(per_ch, nch) : nch;
    Scratch rows(s);
    if (per_ch) HIPCHK(rows.alloc(group * per_ch), ST_INTERNAL);
    float* sa = (float*)rows.p;
    float* serr = sa ? sa + (d_a ? 0 : group * a_ch) : nullptr;
    const long long offset = (long long)(hop / 2) - (center ? 0 : (long long)(frame_len / 2));
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const size_t g = nch - c0 < group ? nch - c0 : group;
        float* a = d_a ? d_a + c0 * a_ch_stride : sa;
        const size_t as = d_a ? a_ch_stride : a_ch;
        if (int st = vvhip_lpc_frames_device(d_signal + c0 * ch_stride, n, g, ch_stride, frame_len, hop, frames, center,
                                             d_window, order, a, as, d_err ? d_err + c0 * err_ch_stride : serr,
                                             d_err ? err_ch_stride : frames, stream))
            return st;
        if (int st = vvhip_lpc_residual_device(d_signal + c0 * ch_stride, n, g, ch_stride, a, order, frames, w, as,
                                               nullptr, 0, hop, offset, nullptr, d_e + c0 * e_stride, e_stride, stream))
            return st;
    }
    return ST_OK;
}

int vvhip_lpc_residual_host(const float* x, size_t n, const float* a, size_t order, size_t frames, size_t seg_len,
                            long long offset, const float* gain, double* state, float* e) {
    if (!x || !a || !e) return ST_NULL;
    if (int st = lpcf_sizes(n, 1, n, n, order, frames, order + 1, 0, gain != nullptr, 0, seg_len, offset)) return st;
    if (n == 0) return ST_OK;
    HostCall c("lpc_residual");
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    const float* da = (const float*)c.in(a, sizeof(float) * frames * (order + 1));
    const float* dg = (const float*)c.in(gain, sizeof(float) * frames);
    double* ds = state ? (double*)c.inout(state, sizeof(double) * order) : nullptr;
    float* de = (float*)c.out(e, sizeof(float) * n);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_lpc_residual_device(dx, n, 1, n, da, order, frames, order + 1, 0, dg, 0, seg_len, offset, ds,
                                              de, n, c.s));
}

int vvhip_lpc_synth_host(const float* e, size_t n, const float* a, size_t order, size_t frames, size_t seg_len,
                         long long offset, const float* gain, double* state, float* y) {
    if (!e || !a || !y) return ST_NULL;
    if (int st = lpcf_sizes(n, 1, n, n, order, frames, order + 1, 0, gain != nullptr, 0, seg_len, offset)) return st;
    if (n == 0) return ST_OK;
    HostCall c("lpc_synth");
    const float* de = (const float*)c.in(e, sizeof(float) * n);
    const float* da = (const float*)c.in(a, sizeof(float) * frames * (order + 1));
    const float* dg = (const float*)c.in(gain, sizeof(float) * frames);
    double* ds = state ? (double*)c.inout(state, sizeof(double) * order) : nullptr;
    float* dy = (float*)c.out(y, sizeof(float) * n);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_lpc_synth_device(de, n, 1, n, da, order, frames, order + 1, 0, dg, 0, seg_len, offset, ds, dy,
                                           n, c.s));
}

}  // extern "C"
