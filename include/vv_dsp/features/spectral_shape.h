/* spectral_shape.h -- per-frame spectral shape descriptors of power rows:
 * energy, centroid, spread, skewness, kurtosis, flatness, roll-off, flux, crest
 * and peak bin.  The reference library has no such code (its features/ holds
 * mel.h alone), so this header is the definition; every sum and decision runs
 * on the GPU (shape_kernels.hip), the batched forms are in vv_dsp_amd.h
 * (vv_dsp_spectral_shape_device, vv_dsp_stft_spectral_shape_device).
 *
 * A row p[0 .. K), K = n_fft / 2 + 1, holds the power of bin k at k sample_rate /
 * n_fft Hz (vv_dsp_stft_power_device's rows).  Its weights are w_k = p_k, or with
 * `magnitude` w_k = sqrtf(p_k), the correctly rounded float.  q is the row's
 * predecessor, the previous row of the same group.  Every sum runs over the band
 * k_min <= k <= k_max of B = k_max - k_min + 1 bins.
 *
 * f64 class: the weights converted to f64, accumulated in f64, rounded to float once.
 *   energy    S0 = sum w_k.
 *   centroid  c = S1 / S0 in bins, S1 = sum k w_k (k w_k is exact in f64); the output
 *             is (float)(c (double)sample_rate / (double)n_fft), in Hz; 0 when S0 == 0.
 *   spread    sigma = sqrt(m2 / S0) with m_j = sum (k - c)^j w_k, a second pass about
 *             the f64 c; scaled to Hz as the centroid; 0 when S0 == 0.
 *   skewness  (m3 / S0) / sigma^3.
 *   kurtosis  (m4 / S0) / sigma^4: the plain fourth standardised moment -- nothing
 *             is subtracted (vv_dsp/core/stats.h's kurtosis subtracts 3; this does not).
 *             Skewness and kurtosis are 0 when m2 == 0 (and when S0 == 0); a row with
 *             one non-zero bin k has c == k exactly, hence m2 == 0 exactly.
 *   flatness  with w'_k = max(w_k, floor): exp((1 / B) sum ln w'_k) / ((1 / B) sum w'_k),
 *             the geometric over the arithmetic mean.  The product of the w'_k is
 *             formed as an f64 mantissa in [0.5, 1) and an integer exponent, one log
 *             and one exp per row.  An all-zero row gives exactly 1.
 *   flux      sqrt(sum (w_k - w_k(q))^2), the difference of two floats exact in f64;
 *             0 for the first row of a group.
 *   crest     max_k w_k / (S0 / B); 0 when S0 == 0.
 * Exact class:
 *   peak_bin  (uint32) the first k that attains the maximum of w over the band, by
 *             the comparison rule of vv_dsp/core/stats.h: the running value starts
 *             at w_(k_min), a weight replaces it when strictly larger, ties go to
 *             the lowest index and a later NaN never replaces it.
 *   rolloff   with C_k = sum_{k_min <= j <= k} w_j in f64 and T = (double)rolloff S0:
 *             the smallest k with C_k >= T, or k_max when no k qualifies (C_(k_max)
 *             and S0 are the same sum in two orders and may differ in the last bit;
 *             a NaN compares false); the output is (float)(k sample_rate / n_fft), in
 *             Hz.  S0 == 0 gives k_min.
 *
 * Order.  Every f64 sum has one order, fixed by (K, k_min, k_max) alone: with t the
 * smallest odd number >= K / 64, lane l of 64 owns bins [l t, l t + t) and adds its
 * bins of the band in ascending k; the 64 partial sums combine by an xor butterfly
 * (32, 16, .. 1).  C_k is the f64 sum of the partial sums of the lanes below k's
 * (an inclusive scan by 1, 2, .. 32), to which the lane's bins up to k are added
 * one by one.  No value depends on the number of rows, the pitch, the grouping
 * (but for the flux of a group's first row), the outputs requested or the entry
 * point.
 *
 * Non-finite input.  The values are not checked and the NaN policy
 * (vv_dsp/core/nan_policy.h) is not applied.  A negative weight counts as a NaN.
 * A row holding a NaN (or a negative power) gives NaN in its f64-class outputs
 * and in the next row's flux; no other row changes.
 *
 * Checks, in this order, all before any device work:
 *   1. NULL params, rows or out struct -- NULL_POINTER;
 *   2. n_fft < 2, or (device rows) row_pitch < K -- INVALID_SIZE;
 *   3. k_min > k_max or k_max > n_fft / 2 -- OUT_OF_RANGE;
 *   4. a non-finite or non-positive sample_rate or floor, or rolloff outside
 *      (0, 1] -- OUT_OF_RANGE;
 *   5. K > 8193 (n_fft > 16385) -- UNSUPPORTED.
 * Zero rows: OK, nothing written.  No output requested: OK, nothing launched.
 * With no GPU a call that reaches the computation returns VV_DSP_ERROR_UNSUPPORTED. */
#ifndef VV_DSP_FEATURES_SPECTRAL_SHAPE_H
#define VV_DSP_FEATURES_SPECTRAL_SHAPE_H
#include <stddef.h>
#include <stdint.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct vv_dsp_spectral_shape_params {
    size_t      n_fft;        /* row has K = n_fft/2 + 1 power bins, bin k at k*sample_rate/n_fft Hz */
    vv_dsp_real sample_rate;  /* Hz */
    int         magnitude;    /* 0: weights w_k = p_k;  nonzero: w_k = sqrtf(p_k), correctly rounded float */
    size_t      k_min, k_max; /* the band, inclusive; 0 and n_fft/2 for the whole row */
    vv_dsp_real rolloff;      /* in (0, 1], e.g. 0.85 */
    vv_dsp_real floor;        /* > 0, flatness only (1e-10 is usual for power) */
} vv_dsp_spectral_shape_params;
/* the ten values of one row */
typedef struct vv_dsp_spectral_shape_values {
    vv_dsp_real energy, centroid, spread, skewness, kurtosis, flatness, rolloff, flux, crest;
    uint32_t peak_bin;
} vv_dsp_spectral_shape_values;
/* One row of n_fft/2 + 1 powers in host memory through the same kernel;
 * prev_row_or_NULL is its predecessor (NULL: the first row of a group, flux 0). */
vv_dsp_status vv_dsp_spectral_shape(const vv_dsp_real* power_row, const vv_dsp_real* prev_row_or_NULL,
                                    const vv_dsp_spectral_shape_params* params, vv_dsp_spectral_shape_values* out);
#ifdef __cplusplus
}
#endif
#endif
