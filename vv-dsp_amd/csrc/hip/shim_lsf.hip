// shim_lsf.hip -- line spectral frequencies and reflection coefficients of LPC
// rows (include/vv_dsp/envelope/lsf.h): the entry points over lsf_kernels.hip.
// Every check is made before any device work, in the header's order: null
// pointers or no output wanted; order < 1 or a pitch below order + 1; order above
// 32; then no rows (OK) and no device.  STAT_LSF counts the launches.
//
// Scratch.  The fused entry writes the LPC rows (and the err plane, when the
// caller does not want it) of a group of channels to scratch with
// vvhip_lpc_frames_device and converts them: groups of at most LSF_ROW_BYTES
// (1 GiB) of rows, at least one channel (32 channels of ten minutes at 16 kHz,
// hop 160, order 32 are 0.26 GiB: one group).  Rows are independent, so no value
// depends on the grouping; knob LSF_GROUP = g > 0 forces groups of g channels
// (here and in shim_formant.hip), for the tests that cross a boundary.
#include "shim_common.hpp"

using namespace vvh;

static constexpr size_t LSF_ROW_BYTES = (size_t)1 << 30;

static int lsf_sizes(size_t order, size_t pitch, size_t batch) {
    if (order < 1 || pitch < order + 1) return ST_SIZE;
    if (order > (size_t)LSF_MAX_ORDER) return fail(ST_UNSUP, "lsf: order above 32");
    if (batch >= ((size_t)1 << 31) || pitch >= ((size_t)1 << 31)) return fail(ST_SIZE, "lsf: batch or pitch >= 2^31");
    return ST_OK;
}

namespace vvh {
// channels per group of a _frames_ call whose scratch takes per_ch bytes a channel
size_t lsf_group(size_t per_ch, size_t nch) {
    size_t group = LSF_ROW_BYTES / (per_ch ? per_ch : 1);
    const long long forced = knob(KNOB_LSF_GROUP, 0);
    if (forced > 0) group = (size_t)forced;
    return group < 1 ? 1 : group > nch ? nch : group;
}
}  // namespace vvh

extern "C" {

int vvhip_lpc_to_lsf_device(const float* d_a, size_t order, size_t batch, size_t a_pitch, float* d_lsf, float* d_rc,
                            int32_t* d_flags, void* stream) {
    if (!d_a || (!d_lsf && !d_rc && !d_flags)) return ST_NULL;
    if (int st = lsf_sizes(order, a_pitch, batch)) return st;
    if (batch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    HIPCHK(launch_lpc_to_lsf(d_a, (int)order, (long long)batch, (long long)a_pitch, d_lsf, d_rc, d_flags,
                             (hipStream_t)stream),
           ST_INTERNAL);
    stat_inc(STAT_LSF);
    return ST_OK;
}

int vvhip_lsf_to_lpc_device(const float* d_lsf, size_t order, size_t batch, float* d_a, size_t a_pitch, void* stream) {
    if (!d_lsf || !d_a) return ST_NULL;
    if (int st = lsf_sizes(order, a_pitch, batch)) return st;
    if (batch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    HIPCHK(launch_lsf_to_lpc(d_lsf, (int)order, (long long)batch, d_a, (long long)a_pitch, (hipStream_t)stream),
           ST_INTERNAL);
    stat_inc(STAT_LSF);
    return ST_OK;
}

int vvhip_lsf_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                            size_t hop, size_t frames, int center, const float* d_window, size_t order, float* d_lsf,
                            float* d_rc, int32_t* d_flags, float* d_err, void* stream) {
    if (!d_signal || (!d_lsf && !d_rc && !d_flags && !d_err)) return ST_NULL;
    if (hop == 0 || frame_len == 0 || order + 1 > frame_len) return ST_SIZE;
    if (int st = lsf_sizes(order, order + 1, 0)) return st;
    if (frames == 0 || nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    hipStream_t s = (hipStream_t)stream;
    const size_t w = order + 1, a_ch = frames * w;   // floats of coefficient rows per channel
    const size_t group = lsf_group((a_ch + (d_err ? 0 : frames)) * sizeof(float), nch);
    Scratch rows(s);
    HIPCHK(rows.alloc(group * (a_ch + (d_err ? 0 : frames)) * sizeof(float)), ST_INTERNAL);
    float* sa = (float*)rows.p;
    float* serr = sa + group * a_ch;
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const size_t g = nch - c0 < group ? nch - c0 : group;
        if (int st = vvhip_lpc_frames_device(d_signal + c0 * ch_stride, n, g, ch_stride, frame_len, hop, frames, center,
                                             d_window, order, sa, a_ch, d_err ? d_err + c0 * frames : serr, frames,
                                             stream))
            return st;
        if (d_lsf || d_rc || d_flags)
            if (int st = vvhip_lpc_to_lsf_device(sa, order, g * frames, w, d_lsf ? d_lsf + c0 * frames * order : nullptr,
                                                 d_rc ? d_rc + c0 * frames * order : nullptr,
                                                 d_flags ? d_flags + c0 * frames : nullptr, stream))
                return st;
    }
    return ST_OK;
}

int vvhip_lpc_to_lsf_host(const float* a, size_t order, float* lsf, float* rc, int32_t* flags) {
    if (!a || (!lsf && !rc && !flags)) return ST_NULL;
    if (int st = lsf_sizes(order, order + 1, 1)) return st;
    HostCall c("lpc_to_lsf");
    const float* da = (const float*)c.in(a, sizeof(float) * (order + 1));
    float* dl = lsf ? (float*)c.out(lsf, sizeof(float) * order) : nullptr;
    float* dr = rc ? (float*)c.out(rc, sizeof(float) * order) : nullptr;
    int32_t* df = flags ? (int32_t*)c.out(flags, sizeof(int32_t)) : nullptr;
    if (!c.ok()) return c.st;
    return c.finish(vvhip_lpc_to_lsf_device(da, order, 1, order + 1, dl, dr, df, c.s));
}

int vvhip_lsf_to_lpc_host(const float* lsf, size_t order, float* a) {
    if (!lsf || !a) return ST_NULL;
    if (int st = lsf_sizes(order, order + 1, 1)) return st;
    HostCall c("lsf_to_lpc");
    const float* dl = (const float*)c.in(lsf, sizeof(float) * order);
    float* da = (float*)c.out(a, sizeof(float) * (order + 1));
    if (!c.ok()) return c.st;
    return c.finish(vvhip_lsf_to_lpc_device(dl, order, 1, da, order + 1, c.s));
}

}  // extern "C"
