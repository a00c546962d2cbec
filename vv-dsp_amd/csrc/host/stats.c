/* stats.c -- array statistics and signal measurements on the MI355X backend (C99).
 * Semantics and argument checks of the reference's src/core/core.c:42-108 and
 * src/core/stats.c:10-139, in its order: NULL or n == 0 first, then the size
 * rule with the reference's *out = 0.  Every sum, comparison and derived value
 * runs on the GPU (vvhip_stats_*, vvhip_cross_correlation_*; stats_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/core/stats.h"
#include "vv_dsp/core/framing.h"
#include "vv_dsp_hip.h"

/* bit k of a mask = member k of vv_dsp_stats_out */
enum { B_SUM, B_MEAN, B_VAR, B_RMS, B_MIN, B_MAX, B_CREST, B_SKEW, B_KURT, B_ZC, B_ARGMIN, B_ARGMAX, NFLOAT = 9 };

static int invalid_in(const vv_dsp_real* x, size_t n) { return x == NULL || n == 0; }

/* one float output of the row */
static vv_dsp_status stat_real(const vv_dsp_real* x, size_t n, int bit, vv_dsp_real* out) {
    float vals[NFLOAT];
    const vv_dsp_status st = (vv_dsp_status)vvhip_stats_host(x, n, 1u << bit, vals, NULL);
    if (st == VV_DSP_OK) *out = vals[bit];
    return st;
}

/* one count or index */
static vv_dsp_status stat_index(const vv_dsp_real* x, size_t n, int bit, size_t* out) {
    size_t idx[3];
    const vv_dsp_status st = (vv_dsp_status)vvhip_stats_host(x, n, 1u << bit, NULL, idx);
    if (st == VV_DSP_OK) *out = idx[bit - NFLOAT];
    return st;
}

vv_dsp_status vv_dsp_sum(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_real(x, n, B_SUM, out);
}

vv_dsp_status vv_dsp_mean(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_real(x, n, B_MEAN, out);
}

vv_dsp_status vv_dsp_var(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    if (n < 2) { *out = 0; return VV_DSP_ERROR_INVALID_SIZE; }
    return stat_real(x, n, B_VAR, out);
}

vv_dsp_status vv_dsp_min(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_real(x, n, B_MIN, out);
}

vv_dsp_status vv_dsp_max(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_real(x, n, B_MAX, out);
}

vv_dsp_status vv_dsp_argmin(const vv_dsp_real* x, size_t n, size_t* idx) {
    if (!idx || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_index(x, n, B_ARGMIN, idx);
}

vv_dsp_status vv_dsp_argmax(const vv_dsp_real* x, size_t n, size_t* idx) {
    if (!idx || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_index(x, n, B_ARGMAX, idx);
}

vv_dsp_status vv_dsp_rms(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_real(x, n, B_RMS, out);
}

vv_dsp_status vv_dsp_peak(const vv_dsp_real* x, size_t n, vv_dsp_real* min_val, vv_dsp_real* max_val) {
    if (invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    const unsigned mask = (min_val ? 1u << B_MIN : 0u) | (max_val ? 1u << B_MAX : 0u);
    if (!mask) return VV_DSP_OK;
    float vals[NFLOAT];
    const vv_dsp_status st = (vv_dsp_status)vvhip_stats_host(x, n, mask, vals, NULL);
    if (st != VV_DSP_OK) return st;
    if (min_val) *min_val = vals[B_MIN];
    if (max_val) *max_val = vals[B_MAX];
    return VV_DSP_OK;
}

vv_dsp_status vv_dsp_crest_factor(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_real(x, n, B_CREST, out);
}

vv_dsp_status vv_dsp_zero_crossing_rate(const vv_dsp_real* x, size_t n, size_t* count_out) {
    if (!count_out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    return stat_index(x, n, B_ZC, count_out);
}

vv_dsp_status vv_dsp_skewness(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    if (n < 3) { *out = 0; return VV_DSP_ERROR_INVALID_SIZE; }
    return stat_real(x, n, B_SKEW, out);
}

vv_dsp_status vv_dsp_kurtosis(const vv_dsp_real* x, size_t n, vv_dsp_real* out) {
    if (!out || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    if (n < 4) { *out = 0; return VV_DSP_ERROR_INVALID_SIZE; }
    return stat_real(x, n, B_KURT, out);
}

vv_dsp_status vv_dsp_autocorrelation(const vv_dsp_real* x, size_t n, vv_dsp_real* r, size_t r_len, int biased) {
    if (!r || invalid_in(x, n)) return VV_DSP_ERROR_NULL_POINTER;
    if (r_len == 0) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_cross_correlation_host(x, n, x, n, r, r_len, biased != 0);
}

vv_dsp_status vv_dsp_cross_correlation(const vv_dsp_real* x, size_t nx, const vv_dsp_real* y, size_t ny,
                                       vv_dsp_real* r, size_t r_len) {
    if (!r || invalid_in(x, nx) || invalid_in(y, ny)) return VV_DSP_ERROR_NULL_POINTER;
    if (r_len == 0) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_cross_correlation_host(x, nx, y, ny, r, r_len, 0);
}

/* batched device rows and frames (vv_dsp_amd.h); vv_dsp_stats_out and
 * vvhip_stats_out have the same members in the same order */
vv_dsp_status vv_dsp_stats_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t row_stride,
                                  const vv_dsp_stats_out* out, void* stream) {
    if (!d_x || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_stats_device(d_x, n, batch, row_stride, (const vvhip_stats_out*)out, stream);
}

vv_dsp_status vv_dsp_stats_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                         size_t frame_len, size_t hop_len, int center, const vv_dsp_real* d_window,
                                         const vv_dsp_stats_out* out, size_t out_ch_stride, void* stream) {
    if (!d_signal || !out) return VV_DSP_ERROR_NULL_POINTER;
    if (hop_len == 0 || frame_len == 0) return VV_DSP_ERROR_INVALID_SIZE;
    const size_t frames = vv_dsp_get_num_frames(n, frame_len, hop_len, center);
    return (vv_dsp_status)vvhip_stats_frames_device(d_signal, n, nch, ch_stride, frame_len, hop_len, frames, center,
                                                    d_window, (const vvhip_stats_out*)out, out_ch_stride, stream);
}

vv_dsp_status vv_dsp_autocorrelation_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t r_len, int biased,
                                            vv_dsp_real* d_r, void* stream) {
    if (!d_r || invalid_in(d_x, n)) return VV_DSP_ERROR_NULL_POINTER;
    if (r_len == 0) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_autocorrelation_device(d_x, n, batch, r_len, biased != 0, d_r, stream);
}

vv_dsp_status vv_dsp_cross_correlation_device(const vv_dsp_real* d_x, size_t nx, const vv_dsp_real* d_y, size_t ny,
                                              size_t batch, size_t r_len, vv_dsp_real* d_r, void* stream) {
    if (!d_r || invalid_in(d_x, nx) || invalid_in(d_y, ny)) return VV_DSP_ERROR_NULL_POINTER;
    if (r_len == 0) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_cross_correlation_device(d_x, nx, d_y, ny, batch, r_len, 0, d_r, stream);
}
