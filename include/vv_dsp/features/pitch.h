/* pitch.h -- fundamental frequency of a frame by YIN (de Cheveigne & Kawahara
 * 2002, steps 2-5).  The reference library has no pitch code (its roadmap asks
 * for one), so this header is the definition; every sum and decision runs on
 * the GPU (pitch_kernels.hip), the batched and per-frame forms are in
 * vv_dsp_amd.h (vv_dsp_pitch_device, vv_dsp_pitch_frames_device).
 *
 * For a frame x[0 .. n) and parameters sample_rate (fs), fmin, fmax, threshold:
 *   lags      tau_min = max(2, floor(fs / fmax)), tau_max = ceil(fs / fmin), in
 *             double from the float parameters; W = n - tau_max, the integration
 *             length: every lag sums the same W terms.
 *   d         d(tau) = sum_{j < W} (x[j] - x[j + tau])^2, tau = 0 .. tau_max: the
 *             samples converted to f64, then subtract, square and accumulate in
 *             f64 (one accumulator per lag, ascending j; the order depends on
 *             (n, tau_max) alone, never on the batch, the stride, the outputs
 *             requested or the entry point).
 *   d'        the cumulative mean normalised difference: d'(0) = 1; with c(tau) =
 *             sum_{k = 1 .. tau} d(k) in f64, d'(tau) = d(tau) tau / c(tau), and
 *             d'(tau) = 1 exactly where c(tau) == 0.
 *   decision  the smallest tau in [tau_min, tau_max] with d'(tau) < threshold, then
 *             to the right while tau + 1 <= tau_max and d'(tau + 1) < d'(tau).
 *             voiced (there is one): lag = tau; where tau - 1 >= 1, tau + 1 <=
 *               tau_max, a = d'(tau - 1) >= b = d'(tau), c = d'(tau + 1) >= b and
 *               a - 2b + c > 0: off = (a - c) / (2 (a - 2b + c)), else off = 0;
 *               f0 = fs / (tau + off) in f64, rounded to float once;
 *               aperiodicity = (float)d'(tau).
 *             unvoiced (none): f0 = 0; lag = the first tau that attains the
 *               minimum of d' over [tau_min, tau_max] (ties go to the lower
 *               tau); aperiodicity = (float)d'(lag).  A silent or constant
 *               frame gives (0, 1.0, tau_min).
 *   non-finite  c(tau_max) (which holds every sample) not finite: f0 = 0,
 *             aperiodicity = NaN, lag = 0.
 *
 * Checks, in this order: NULL x or params -- NULL_POINTER; n == 0 --
 * INVALID_SIZE; a non-finite or non-positive sample_rate, fmin or fmax, fmin >=
 * fmax, fmax > sample_rate / 2, threshold outside (0, 1] or tau_min >= tau_max --
 * OUT_OF_RANGE; W < 1 (n <= tau_max) -- INVALID_SIZE; n > 16384 or tau_max >
 * 8191 -- UNSUPPORTED.  All before any device work; with no GPU a call that
 * reaches the computation returns VV_DSP_ERROR_UNSUPPORTED. */
#ifndef VV_DSP_FEATURES_PITCH_H
#define VV_DSP_FEATURES_PITCH_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct vv_dsp_pitch_params {
    vv_dsp_real sample_rate; /* Hz */
    vv_dsp_real fmin, fmax;  /* the search range, Hz */
    vv_dsp_real threshold;   /* on d', in (0, 1]; 0.1 .. 0.2 is usual */
} vv_dsp_pitch_params;
/* The lag range of a frame of frame_len samples (host arithmetic; each output
 * may be NULL): the curve d' has *tau_max + 1 values.  The checks above with
 * n = frame_len; nothing is written unless the result is VV_DSP_OK. */
vv_dsp_status vv_dsp_pitch_lag_range(const vv_dsp_pitch_params* params, size_t frame_len, size_t* tau_min,
                                     size_t* tau_max, size_t* integration_len);
/* One frame in host memory; f0 and aperiodicity may each be NULL. */
vv_dsp_status vv_dsp_pitch_yin(const vv_dsp_real* x, size_t n, const vv_dsp_pitch_params* params, vv_dsp_real* f0,
                               vv_dsp_real* aperiodicity);
#ifdef __cplusplus
}
#endif
#endif
