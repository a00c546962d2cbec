/* hpss.h -- harmonic-percussive separation of power rows by median filtering
 * (Fitzgerald 2010): a running median along time (the harmonic estimate H), one
 * along frequency (the percussive estimate P), and masks from the two.  The
 * reference library has no such code, so this header is the definition; every
 * value is computed on the GPU (median_kernels.hip), the batched forms are in
 * vv_dsp_amd.h (vv_dsp_hpss_device, vv_dsp_stft_hpss_device).
 *
 * Rows and weights.  A row p[0 .. K), K = n_fft / 2 + 1, holds the power of bin k
 * (vv_dsp_stft_power_device's rows, packed or pitched).  Its weights are w = p, or
 * with `magnitude` w = sqrtf(p), the correctly rounded float (as in
 * vv_dsp/features/spectral_shape.h).  A NaN weight is replaced by the quiet NaN
 * 0x7FC00000 (vv_dsp/filter/median.h, "The median rule", which both medians
 * follow: keys, rank h of L = 2h + 1, no arithmetic on the weights); a negative
 * power under `magnitude` is therefore that NaN.
 *
 * Groups.  Rows form groups of rows_per_group consecutive rows (the frames of one
 * channel); 0 means one group, and the last group may be short -- the meaning of
 * vv_dsp_spectral_shape_device's rows_per_group.  The time median never crosses a
 * group.
 *
 * The two medians, row t of a group of G rows, bin k:
 *   H[t][k]  the median of w[t - h .. t + h][k], h = win_harm / 2, rows outside
 *            [0, G) by REFLECT over the group's rows (median.h);
 *   P[t][k]  the median of w[t][k - h .. k + h], h = win_perc / 2, bins outside
 *            [0, K) by REFLECT.
 *
 * Masks.  With a = (double)H and b = (double)margin_harm * (double)P (the product
 * of two floats, exact), each line one IEEE f64 operation, nothing fused:
 *   HARD    a > b ? 1 : 0 (a NaN on either side gives 0);
 *   SOFT    d = a + b;                        q = a / d;
 *   WIENER  a2 = a * a; b2 = b * b; d = a2 + b2; q = a2 / d;
 * d == 0 gives q = 0.5.  mask_harm is q rounded to float once; a NaN result is
 * stored as the quiet NaN 0x7FC00000.  mask_perc is the same with H and P
 * exchanged and margin_perc.  harm is H and perc is P themselves.
 *
 * No value depends on the number of rows, the pitches, the outputs requested or
 * the entry point; an output that is not requested costs no store.
 *
 * Checks, in this order, all before any device work:
 *   1. NULL params, rows or out struct -- NULL_POINTER;
 *   2. n_fft < 2, or (device rows) row_pitch or out_pitch < K -- INVALID_SIZE;
 *   3. an even or non-positive win_harm or win_perc, an unknown mask, or a margin
 *      that is not finite or is below 1 -- OUT_OF_RANGE;
 *   4. a window > 127, K > VV_DSP_HPSS_MAX_BINS, a group of 2^31 rows or more, or
 *      rows * ceil(K / 64) >= 2^31 (more than one launch takes) -- UNSUPPORTED.
 * Zero rows or no output requested: OK, nothing launched.  With no GPU a call that
 * reaches the computation returns VV_DSP_ERROR_UNSUPPORTED.  An output plane must
 * not overlap the input or another plane; this is not checked. */
#ifndef VV_DSP_SPECTRAL_HPSS_H
#define VV_DSP_SPECTRAL_HPSS_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the widest row the kernels take (n_fft 16384 or 16385) */
#define VV_DSP_HPSS_MAX_BINS 8193
#define VV_DSP_HPSS_HARD 0
#define VV_DSP_HPSS_SOFT 1
#define VV_DSP_HPSS_WIENER 2
typedef struct vv_dsp_hpss_params {
    size_t      n_fft;        /* a row has K = n_fft/2 + 1 power bins */
    int         magnitude;    /* 0: weights w = p;  nonzero: w = sqrtf(p), correctly rounded */
    int         win_harm;     /* odd, rows: median along time, per bin (librosa: 31) */
    int         win_perc;     /* odd, bins: median along frequency, per row (librosa: 31) */
    vv_dsp_real margin_harm, margin_perc;   /* finite, >= 1 */
    int         mask;         /* VV_DSP_HPSS_HARD, _SOFT or _WIENER */
} vv_dsp_hpss_params;
typedef struct vv_dsp_hpss_out {   /* each NULL (not wanted) or [rows][out_pitch], K values of a row written */
    vv_dsp_real *harm, *perc, *mask_harm, *mask_perc;
} vv_dsp_hpss_out;
/* One group of `rows` packed rows (K floats each) in host memory through the same
 * kernels; the planes of `out` are host memory, [rows][K]. */
vv_dsp_status vv_dsp_hpss(const vv_dsp_real* power_rows, size_t rows, const vv_dsp_hpss_params* params,
                          const vv_dsp_hpss_out* out);
#ifdef __cplusplus
}
#endif
#endif
