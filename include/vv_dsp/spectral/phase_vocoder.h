/* phase_vocoder.h -- time-stretch of STFT rows: the textbook phase vocoder, which
 * changes duration without changing pitch.  The reference library has no such
 * code (its spectral/ holds the STFT alone), so this header is the definition;
 * every value is computed on the GPU (pvoc_kernels.hip), the batched forms are in
 * vv_dsp_amd.h (vv_dsp_phase_vocoder_uniform_device, vv_dsp_phase_vocoder_device,
 * vv_dsp_stft_time_stretch_device).
 *
 * Input.  Complex rows D[t][k], 0 <= t < T, each of n_fft vv_dsp_cpx (the layout
 * of vv_dsp_stft_spectrum_device); only bins 0 <= k <= n_fft / 2 are read,
 * K = n_fft / 2 + 1 of them.  Rows t >= T count as all zero.
 *
 * Positions.  Output row j (0 <= j < m) sits at analysis position p_j, an f64:
 *   uniform  p_j = start + (double)j * step, the product and the sum rounded
 *            separately (as vv_dsp_interpolate_uniform_device forms its positions);
 *   curve    p_j = (double)d_pos[j], a float array on the device shared by all
 *            channels, clamped into [0, T]; a NaN becomes 0.
 * t0 = floor(p_j) and a = p_j - t0.
 *
 * Per bin k, every operation in f64 and rounded on its own (nothing is fused):
 *   mag_t = sqrt((double)re^2 + (double)im^2);
 *   th_t  = atan2(im, re), and exactly 0 when re == 0 && im == 0 (whatever the
 *           signs of the zeros), and 0 for a row t >= T;
 *   m_j   = (1 - a) mag_t0 + a mag_(t0+1);
 *   d_j   = th_(t0+1) - th_t0;
 *   A_j   = sum_{i < j} d_i, A_0 = 0, in the order below;
 *   phi_j = th_(t0 of row 0) + A_j;
 *   out[j][k] = ((float)(m_j cos phi_j), (float)(m_j sin phi_j)), 0 <= k <= n_fft / 2;
 *   out[j][n_fft - k] is its conjugate for 0 < 2 k < n_fft, so that a row feeds
 *   vv_dsp_stft_reconstruct_device as it is (every one of the n_fft bins is written);
 *   m_j == 0 gives exactly (+0, +0), but for a bin that is already NaN (below).
 * exp(i (w_k hop + wrap(D))) equals exp(i (th_(t0+1) - th_t0)): the expected phase
 * advance and the wrapping of the usual recurrence drop out of the output.
 *
 * Order of the sum.  Output rows form segments of VV_DSP_PVOC_SEGMENT rows, row j
 * in segment s = j / VV_DSP_PVOC_SEGMENT.  P_j is the sum of the d_i of the rows
 * i < j of j's own segment, added in ascending i from 0.0; a segment's total is
 * the sum of all its rows' d_i formed the same way; B_s is the sum of the totals
 * of segments 0 .. s - 1, added in ascending order from 0.0.  A_j = B_s + P_j (one
 * addition), phi_j = th + A_j (one more).  The order depends on j alone: no value
 * depends on the number of channels, the strides, the entry point, or on whether
 * equal positions came as start and step or as a curve.
 *
 * Non-finite input.  The input is not checked.  A bin D[t][k] that holds a NaN or
 * an infinity has th_t = NaN and mag_t = NaN (neither atan2 nor sqrt of an infinity
 * is a NaN): both components of bin k (and of its mirror) of the output are NaN
 * from the first output row that uses row t -- as row t0 or as row t0 + 1, whatever
 * a is -- onward, also where m_j == 0.  No other bin changes.
 *
 * Checks, in this order, all before any device work:
 *   1. a NULL pointer -- NULL_POINTER;
 *   2. n_fft < 2, or (device forms) a channel stride below T n_fft on the input
 *      or m n_fft on the output -- INVALID_SIZE;
 *   3. uniform form: start or step not finite, start < 0, step < 0, or the last
 *      position start + (double)(m - 1) * step > T -- OUT_OF_RANGE;
 *   4. n_fft > VV_DSP_PVOC_MAX_FFT, or T, m or the channel count >= 2^31 -- UNSUPPORTED.
 * m == 0 or no channel: OK, nothing written.  With no GPU a call that reaches
 * the computation returns VV_DSP_ERROR_UNSUPPORTED.  On failure the outputs are
 * untouched.
 *
 * Time-stretch (vv_dsp_stft_time_stretch_device, vv_dsp_amd.h): a signal's T frames
 * through the vocoder at start = 0, step = rate, m the number of j >= 0 with
 * (double)j * rate < (double)T, overlap-added at the handle's hop to
 * out_len = (m - 1) hop + n_fft samples and divided by the summed squared window:
 * y[i] = norm[i] > VV_DSP_PVOC_NORM_FLOOR ? out[i] / norm[i] : 0, a float division. */
#ifndef VV_DSP_SPECTRAL_PHASE_VOCODER_H
#define VV_DSP_SPECTRAL_PHASE_VOCODER_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
/* output rows per segment of the phase sum (see "Order of the sum") */
#define VV_DSP_PVOC_SEGMENT 32
/* the longest row the kernel takes */
#define VV_DSP_PVOC_MAX_FFT 16777216
/* time-stretch: samples whose summed squared window is not above this are 0 */
#define VV_DSP_PVOC_NORM_FLOOR 1e-8f
/* One channel in host memory through the same kernel, uniform form:
 * spec [T][n_fft] -> out [m][n_fft]. */
vv_dsp_status vv_dsp_phase_vocoder(const vv_dsp_cpx* spec, size_t T, size_t n_fft, double start, double step,
                                   size_t m, vv_dsp_cpx* out);
#ifdef __cplusplus
}
#endif
#endif
