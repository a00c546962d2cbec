// shim_pvoc.hip -- the phase vocoder (include/vv_dsp/spectral/phase_vocoder.h):
// the entry points over pvoc_kernels.hip.  Every check is made before any
// device work, in the header's order: null pointers; n_fft < 2 or a channel
// stride shorter than its rows; (uniform form) start, step and the last
// position; the kernel's limits.  m == 0 or no channel: OK, nothing launched.
// STAT_PVOC_ROWS counts the calls that launched the kernels.  The time-stretch
// works in groups of channels whose rows fit PVOC_GROUP_BYTES of scratch (knob
// PVOC_GROUP = k: k channels per group); every kernel it runs treats a channel
// on its own, so the grouping changes no value.
#include "shim_common.hpp"
#include "../../../include/vv_dsp/spectral/phase_vocoder.h"

#include <cmath>

using namespace vvh;

static_assert(PVOC_SEGMENT == VV_DSP_PVOC_SEGMENT && PVOC_MAX_FFT == VV_DSP_PVOC_MAX_FFT, "phase_vocoder.h");
static_assert(PVOC_NORM_FLOOR == VV_DSP_PVOC_NORM_FLOOR, "phase_vocoder.h");

static constexpr size_t PVOC_GROUP_BYTES = (size_t)1 << 30;

// checks 2 to 4 of the header (strided: the device forms' channel strides)
static int pvoc_check(size_t T, size_t n_fft, size_t nch, bool strided, size_t in_ch_stride, size_t out_ch_stride,
                      bool uniform, double start, double step, size_t m) {
    if (n_fft < 2) return fail(ST_SIZE, "phase_vocoder: n_fft below 2");
    if (strided) {
        // T n_fft or m n_fft past size_t cannot be below a stride
        if (T > SIZE_MAX / n_fft || in_ch_stride < T * n_fft)
            return fail(ST_SIZE, "phase_vocoder: input channel stride below T x n_fft");
        if (m > SIZE_MAX / n_fft || out_ch_stride < m * n_fft)
            return fail(ST_SIZE, "phase_vocoder: output channel stride below m x n_fft");
    }
    if (uniform) {
        if (!(std::isfinite(start) && std::isfinite(step))) return fail(ST_RANGE, "phase_vocoder: start or step not finite");
        if (start < 0.0 || step < 0.0) return fail(ST_RANGE, "phase_vocoder: negative start or step");
        if (m > 0) {
            volatile double q = (double)(m - 1) * step;   // rounded on its own, as the kernel's
            if (start + q > (double)T) return fail(ST_RANGE, "phase_vocoder: last position past T");
        }
    }
    const size_t lim = (size_t)1 << 31;
    if (T >= lim || m >= lim || nch >= lim || n_fft > (size_t)PVOC_MAX_FFT ||
        !pvoc_supported((long long)T, (long long)n_fft, (long long)nch, (long long)m))
        return fail(ST_UNSUP, "phase_vocoder: sizes above the kernel's limits");
    return ST_OK;
}

static int pvoc_run(const float* d_spec, size_t T, size_t n_fft, size_t nch, size_t in_ch_stride, const float* d_pos,
                    double start, double step, size_t m, float* d_out, size_t out_ch_stride, hipStream_t s) {
    PvocArgs a;
    a.in = (const float2*)d_spec;
    a.out = (float2*)d_out;
    a.T = (long long)T;
    a.n_fft = (long long)n_fft;
    a.nch = (long long)nch;
    a.m = (long long)m;
    a.in_ch_stride = (long long)in_ch_stride;
    a.out_ch_stride = (long long)out_ch_stride;
    a.pos = d_pos;
    a.start = start;
    a.step = step;
    Scratch work(s);
    HIPCHK(work.alloc(sizeof(double) * pvoc_scratch_doubles(a.n_fft, a.nch, a.m)), ST_INTERNAL);
    a.work = (double*)work.p;
    // knob PVOC_PLANE = 1: the rows' phases through an f64 plane (same bits; for timing)
    Scratch plane(s);
    if (knob(KNOB_PVOC_PLANE, 0) == 1 && pvoc_plane_supported(a.T, a.n_fft, a.nch)) {
        HIPCHK(plane.alloc(sizeof(double) * nch * T * (n_fft / 2 + 1)), ST_INTERNAL);
        a.plane = (const double*)plane.p;
    }
    HIPCHK(launch_pvoc(a, s), ST_INTERNAL);
    stat_inc(STAT_PVOC_ROWS);
    return ST_OK;
}

// m of the time-stretch: the number of j >= 0 with (double)j * rate < (double)T
static size_t stretch_rows(size_t T, double rate) {
    const double Td = (double)T;
    double g = std::ceil(Td / rate);
    if (!(g < 18446744073709549568.0)) return SIZE_MAX;   // past size_t: over every limit
    size_t m = (size_t)g;
    while (m > 0 && !((double)(m - 1) * rate < Td)) --m;
    while ((double)m * rate < Td) ++m;
    return m;
}

extern "C" {

int vvhip_pvoc_device(const float* d_spec, size_t T, size_t n_fft, size_t nch, size_t spec_ch_stride,
                      const float* d_pos, double start, double step, size_t m, float* d_out, size_t out_ch_stride,
                      void* stream) {
    if (!d_spec || !d_out) return ST_NULL;
    if (int st = pvoc_check(T, n_fft, nch, true, spec_ch_stride, out_ch_stride, d_pos == nullptr, start, step, m))
        return st;
    if (m == 0 || nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    return pvoc_run(d_spec, T, n_fft, nch, spec_ch_stride, d_pos, start, step, m, d_out, out_ch_stride,
                    (hipStream_t)stream);
}

// One channel in host memory, uniform form, through the same kernels.
int vvhip_pvoc_host(const float* spec, size_t T, size_t n_fft, double start, double step, size_t m, float* out) {
    if (!spec || !out) return ST_NULL;
    if (int st = pvoc_check(T, n_fft, 1, false, 0, 0, true, start, step, m)) return st;
    if (m == 0) return ST_OK;
    HostCall c("phase_vocoder");
    const float* dspec = (const float*)c.in(spec, 2 * sizeof(float) * T * n_fft);
    float* dout = (float*)c.out(out, 2 * sizeof(float) * m * n_fft);
    if (!c.ok()) return c.st;
    return c.finish(pvoc_run(dspec, T, n_fft, 1, T * n_fft, nullptr, start, step, m, dout, m * n_fft, c.s));
}

int vvhip_stft_stretch_length(size_t n, size_t nfft, size_t hop, double rate, size_t* rows, size_t* out_len) {
    if (nfft < 2 || hop == 0) return ST_SIZE;
    if (!(std::isfinite(rate) && rate > 0.0)) return fail(ST_RANGE, "time_stretch: rate must be finite and positive");
    const size_t m = stretch_rows(vvhip_stft_num_frames(n, nfft, hop), rate);
    if (m >= ((size_t)1 << 31)) return fail(ST_UNSUP, "time_stretch: sizes above the kernel's limits");
    if (rows) *rows = m;
    if (out_len) *out_len = (m - 1) * hop + nfft;
    return ST_OK;
}

int vvhip_stft_stretch_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch, size_t ch_stride,
                              double rate, float* d_out, size_t out_ch_stride, void* stream, size_t* out_len) {
    if (!h || !d_signal || !d_out) return ST_NULL;
    const size_t nfft = h->nfft, hop = h->hop;
    if (nfft < 2) return fail(ST_SIZE, "time_stretch: fft_size below 2");
    if (nch > 1 && ch_stride < n) return fail(ST_SIZE, "time_stretch: a channel stride shorter than its channel");
    const bool rate_ok = std::isfinite(rate) && rate > 0.0;
    const size_t T = vvhip_stft_num_frames(n, nfft, hop);
    const size_t m = rate_ok ? stretch_rows(T, rate) : 0;
    const bool m_ok = rate_ok && m < ((size_t)1 << 31);
    const size_t len = m_ok ? (m - 1) * hop + nfft : 0;
    if (m_ok && out_ch_stride < len) return fail(ST_SIZE, "time_stretch: output channel stride below out_len");
    if (!rate_ok) return fail(ST_RANGE, "time_stretch: rate must be finite and positive");
    if (!m_ok || !pvoc_supported((long long)T, (long long)nfft, (long long)(nch ? nch : 1), (long long)m))
        return fail(ST_UNSUP, "time_stretch: sizes above the kernel's limits");
    if (out_len) *out_len = len;
    if (nch == 0) return ST_OK;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");

    const hipStream_t s = (hipStream_t)stream;
    const size_t row_bytes = 2 * sizeof(float) * nfft;
    const size_t ch_bytes = (T + m) * row_bytes + sizeof(float) * len;
    const long long forced = knob(KNOB_PVOC_GROUP, 0);
    size_t group = forced > 0 ? (size_t)forced : PVOC_GROUP_BYTES / ch_bytes;
    if (group < 1) group = 1;
    if (group > nch) group = nch;
    Scratch spec(s), rows(s), norm(s);
    HIPCHK(spec.alloc(group * T * row_bytes), ST_INTERNAL);
    HIPCHK(rows.alloc(group * m * row_bytes), ST_INTERNAL);
    HIPCHK(norm.alloc(group * len * sizeof(float)), ST_INTERNAL);
    for (size_t c0 = 0; c0 < nch; c0 += group) {
        const size_t g = nch - c0 < group ? nch - c0 : group;
        float* y = d_out + c0 * out_ch_stride;
        if (int st = stft_frames_run(h, d_signal + c0 * ch_stride, n, g, ch_stride, spec.p, T * nfft, 1, s)) return st;
        if (int st = pvoc_run((const float*)spec.p, T, nfft, g, T * nfft, nullptr, 0.0, rate, m, (float*)rows.p,
                              m * nfft, s))
            return st;
        HIPCHK(hipMemsetAsync(norm.p, 0, g * len * sizeof(float), s), ST_INTERNAL);
        for (size_t c = 0; c < g; ++c) {
            HIPCHK(hipMemsetAsync(y + c * out_ch_stride, 0, len * sizeof(float), s), ST_INTERNAL);
            if (int st = vvhip_stft_reconstruct_device(h, (const float*)rows.p + 2 * c * m * nfft, m, hop,
                                                       y + c * out_ch_stride, (float*)norm.p + c * len, s))
                return st;
        }
        HIPCHK(launch_pvoc_normalize(y, (long long)out_ch_stride, (const float*)norm.p, (long long)len, (long long)g, s),
               ST_INTERNAL);
    }
    return ST_OK;
}

}  // extern "C"
