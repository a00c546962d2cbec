/* stats.h -- array statistics and signal measurements (reference
 * include/vv_dsp/core.h:129-245 and :309-453; src/core/core.c:42-108,
 * src/core/stats.c:10-139), with the reference's signatures and checks:
 * a NULL pointer or n == 0 gives VV_DSP_ERROR_NULL_POINTER, and the pointer
 * checks come before the size checks.
 *
 * Numerics on this backend (every sum runs on the GPU, stats_kernels.hip):
 *   exact    min, max, peak, argmin, argmax and the crossing count are those of
 *            the reference's sequential comparisons, bit for bit: ties (+0 / -0
 *            included) resolve to the lowest index and return that element's
 *            bits, x[0] seeds the search, a later NaN never replaces the running
 *            value and a NaN at x[0] stays.  A crossing is (a > 0 && b < 0) ||
 *            (a < 0 && b > 0) on adjacent samples: +, 0, - counts none.
 *   f64      sum, rms, var, skewness, kurtosis and the correlations accumulate
 *            in f64 and round to float once, as the reference does.  The order
 *            of the f64 sums differs from the reference's loop (64 lanes per
 *            chunk of 4096 samples, an xor butterfly, chunks in order), which
 *            moves the f64 value by about n 2^-53 relative: the result is the
 *            reference's float or, rarely, its neighbour (<= 1 ulp).  var,
 *            skewness and kurtosis are moments about mean = sum / n in f64
 *            (two passes); the excess kurtosis' - 3 and skewness' pow(var, 1.5)
 *            are the reference's.  A constant row gives var == 0 exactly, hence
 *            skewness = kurtosis = 0 (the reference's var <= 0 branch).
 *   derived  mean = (float)sum / (float)n (not the running mean) and crest =
 *            max(mx, -mn) / rms, INFINITY when rms == 0, in float as the
 *            reference forms them: bit-identical whenever their inputs are.
 *   order    a value depends on the row's samples and n alone, never on the
 *            batch, the row's position or stride, the other outputs requested or
 *            the entry point (these calls, vv_dsp_stats_device and
 *            vv_dsp_stats_frames_device of vv_dsp_amd.h agree bit for bit).
 * n must be below 2^32 (VV_DSP_ERROR_INVALID_SIZE).  With no GPU every call
 * that reaches the computation returns VV_DSP_ERROR_UNSUPPORTED. */
#ifndef VV_DSP_CORE_STATS_H
#define VV_DSP_CORE_STATS_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
/* f64 sum rounded to float; mean = that float / (float)n */
vv_dsp_status vv_dsp_sum(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
vv_dsp_status vv_dsp_mean(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
/* population variance; n < 2: *out = 0 and VV_DSP_ERROR_INVALID_SIZE */
vv_dsp_status vv_dsp_var(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
vv_dsp_status vv_dsp_min(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
vv_dsp_status vv_dsp_max(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
/* index of the first minimum / maximum */
vv_dsp_status vv_dsp_argmin(const vv_dsp_real* x, size_t n, size_t* idx);
vv_dsp_status vv_dsp_argmax(const vv_dsp_real* x, size_t n, size_t* idx);
/* sqrt(mean of squares) */
vv_dsp_status vv_dsp_rms(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
/* minimum and maximum; either or both outputs may be NULL */
vv_dsp_status vv_dsp_peak(const vv_dsp_real* x, size_t n, vv_dsp_real* min_val, vv_dsp_real* max_val);
/* max |x| / rms; INFINITY when rms == 0 */
vv_dsp_status vv_dsp_crest_factor(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
/* the number of sign changes between adjacent samples (a count, not a rate) */
vv_dsp_status vv_dsp_zero_crossing_rate(const vv_dsp_real* x, size_t n, size_t* count_out);
/* m3 / var^1.5 (n < 3: *out = 0, INVALID_SIZE) and m4 / var^2 - 3 (n < 4
 * likewise), central moments over n; 0 when var <= 0 */
vv_dsp_status vv_dsp_skewness(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
vv_dsp_status vv_dsp_kurtosis(const vv_dsp_real* x, size_t n, vv_dsp_real* out);
/* r[lag] = sum_{i + lag < n} x[i] x[i + lag] over n (biased) or over the n - lag
 * terms, lag < r_len; lags with no term give 0; r_len == 0: INVALID_SIZE */
vv_dsp_status vv_dsp_autocorrelation(const vv_dsp_real* x, size_t n, vv_dsp_real* r, size_t r_len, int biased);
/* r[lag] = sum x[i] y[i + lag] over the terms with i < nx and i + lag < ny,
 * divided by their number; 0 where there is none */
vv_dsp_status vv_dsp_cross_correlation(const vv_dsp_real* x, size_t nx, const vv_dsp_real* y, size_t ny,
                                       vv_dsp_real* r, size_t r_len);
#ifdef __cplusplus
}
#endif
#endif
