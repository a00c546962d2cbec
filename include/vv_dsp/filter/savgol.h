/* savgol.h -- Savitzky-Golay smoothing and differentiation (reference
 * include/vv_dsp/filter/savgol.h:16-45). */
#ifndef VV_DSP_FILTER_SAVGOL_H
#define VV_DSP_FILTER_SAVGOL_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
/* How the half-window beyond either end is filled.  REFLECT mirrors about the
 * edge sample without repeating it (x[1], x[2], .. on the left; x[N-2], x[N-3],
 * .. on the right), CONSTANT and NEAREST both repeat the edge sample, WRAP is
 * circular on the right and x[(N - (i mod N) - 1) mod N] for the i-th sample
 * to the left of x[0] -- what the reference's code does (savgol.c:164-203). */
typedef enum vv_dsp_savgol_mode {
    VV_DSP_SAVGOL_MODE_REFLECT = 0,
    VV_DSP_SAVGOL_MODE_CONSTANT = 1,
    VV_DSP_SAVGOL_MODE_NEAREST = 2,
    VV_DSP_SAVGOL_MODE_WRAP = 3
} vv_dsp_savgol_mode;

/* output[n] = sum_k h[k] y_padded[n + k], h the least-squares polynomial
 * (polyorder) window of odd window_length <= N, window_length <= 257,
 * polyorder <= 15, for the deriv-th derivative (0 <= deriv <= polyorder) at
 * sample spacing delta (> 0 when deriv > 0).  The thread's NaN policy
 * (core/nan_policy.h) is applied to the input and to the output. */
vv_dsp_status vv_dsp_savgol(const vv_dsp_real* y, size_t N, int window_length, int polyorder, int deriv,
                            vv_dsp_real delta, vv_dsp_savgol_mode mode, vv_dsp_real* output);
#ifdef __cplusplus
}
#endif
#endif
