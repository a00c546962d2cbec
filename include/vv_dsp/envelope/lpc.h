/* lpc.h -- linear prediction: autocorrelation, Levinson-Durbin, LPC and the
 * all-pole spectrum (reference include/vv_dsp/envelope/lpc.h:11-21). */
#ifndef VV_DSP_ENVELOPE_LPC_H
#define VV_DSP_ENVELOPE_LPC_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
/* r_out[k] = sum_{i < n-k} x[i] x[i+k], k = 0..order; order + 1 <= n */
vv_dsp_status vv_dsp_autocorr(const vv_dsp_real* x, size_t n, size_t order, vv_dsp_real* r_out);
/* r[order+1] -> a_out[order+1] with A(z) = 1 + sum a[m] z^-m, *err_out the
 * prediction error; r[0] <= 0: VV_DSP_ERROR_INTERNAL, outputs untouched */
vv_dsp_status vv_dsp_levinson(const vv_dsp_real* r, size_t order, vv_dsp_real* a_out, vv_dsp_real* err_out);
/* vv_dsp_autocorr followed by vv_dsp_levinson */
vv_dsp_status vv_dsp_lpc(const vv_dsp_real* x, size_t n, size_t order, vv_dsp_real* a_out, vv_dsp_real* err_out);
/* mag_out[k] = gain / |1 - sum_{m=1..order} a[m] e^(-j 2 pi m k / nfft)|, k < nfft.
 * Note the sign: this is the envelope of coefficients with A(z) = 1 - sum a[m] z^-m,
 * not of vv_dsp_levinson's (negate a[1..order], or use vv_dsp_lpspec_device's
 * levinson_sign, vv_dsp_amd.h). */
vv_dsp_status vv_dsp_lpspec(const vv_dsp_real* a, size_t order, vv_dsp_real gain, size_t nfft, vv_dsp_real* mag_out);
#ifdef __cplusplus
}
#endif
#endif
