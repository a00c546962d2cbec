/* median.h -- running median (rank filter) of float rows.  The reference library
 * has no such code (its filter/ holds the linear FIR, biquad and Savitzky-Golay
 * filters), so this header is the definition; every value is selected on the GPU
 * (median_kernels.hip), the batched form is in vv_dsp_amd.h (vv_dsp_medfilt_device).
 * vv_dsp/spectral/hpss.h uses the same rule in both directions of a spectrogram.
 *
 * The median rule.
 *   Key.     A float is ordered by its key: with b its bits as uint32, the key is
 *            b ^ 0xFFFFFFFF when the sign bit is set and b | 0x80000000 otherwise,
 *            and keys compare as unsigned integers.  So
 *            -inf < .. < -0 < +0 < .. < +inf < NaN.
 *   NaN.     Before the keys are taken every NaN input is replaced by the quiet NaN
 *            0x7FC00000, so a NaN's sign and payload never reach an output.
 *   Median.  For the odd window of L = 2h + 1 values the median is the value of rank
 *            h (0-based) under that order.  Equal keys are equal bit patterns, so
 *            ties cannot change the result, and the output is always one of the
 *            (canonicalised) inputs of its window, bit for bit.
 *   No arithmetic is done on the samples; the thread's NaN policy
 *   (vv_dsp/core/nan_policy.h) is not applied: a NaN is a value, the largest.
 *
 * y[i] is the median of x[i - h .. i + h].  An index j outside [0, n) is resolved
 * by the mode:
 *   REFLECT  mirror about the edge sample without repeating it (the REFLECT of
 *            vv_dsp/filter/savgol.h), folded with period 2n - 2, so any L is legal
 *            for any n: with m = j mod (2n - 2) in [0, 2n - 2), the index is m when
 *            m < n and 2n - 2 - m otherwise; n == 1 gives x[0];
 *   NEAREST  the index clamped to [0, n - 1];
 *   ZERO     the value +0.0f (what scipy.signal.medfilt does).
 * window_length == 1 is a copy (NaNs still canonicalised).
 *
 * Checks, in this order, all before any device work:
 *   1. a NULL pointer -- NULL_POINTER;
 *   2. n == 0, or (device form) batch > 1 and a stride below n -- INVALID_SIZE;
 *   3. an even or non-positive window_length, or an unknown mode -- OUT_OF_RANGE;
 *   4. window_length > VV_DSP_MEDFILT_MAX_WINDOW, or batch * ceil(n / 256) >= 2^31
 *      (more than one launch takes) -- UNSUPPORTED.
 * batch == 0: OK, nothing written.  With no GPU a call that passes its checks
 * returns VV_DSP_ERROR_UNSUPPORTED.  y must not overlap x; this is not checked. */
#ifndef VV_DSP_FILTER_MEDIAN_H
#define VV_DSP_FILTER_MEDIAN_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the longest window the kernel takes */
#define VV_DSP_MEDFILT_MAX_WINDOW 127
typedef enum vv_dsp_medfilt_mode {
    VV_DSP_MEDFILT_MODE_REFLECT = 0,
    VV_DSP_MEDFILT_MODE_NEAREST = 1,
    VV_DSP_MEDFILT_MODE_ZERO = 2
} vv_dsp_medfilt_mode;
/* One row of n samples in host memory through the same kernel. */
vv_dsp_status vv_dsp_medfilt(const vv_dsp_real* x, size_t n, int window_length, vv_dsp_medfilt_mode mode,
                             vv_dsp_real* y);
#ifdef __cplusplus
}
#endif
#endif
