/* denoise.h -- spectral noise suppression of power rows by minimum statistics
 * (Martin 2001, in its windowed form): a short running mean of each bin's power
 * along time, the minimum of that mean over a window of rows as the noise floor,
 * and a gain per cell from the power and the floor.  The reference library has
 * no such code, so this header is the definition; every value is computed on
 * the GPU (denoise_kernels.hip), the batched forms are in vv_dsp_amd.h
 * (vv_dsp_denoise_device, vv_dsp_stft_denoise_device).
 *
 * Rows and groups, as in vv_dsp/spectral/hpss.h.  A row p[0 .. K), K = n_fft / 2
 * + 1, holds the power of bin k (vv_dsp_stft_power_device's rows, packed or
 * pitched).  Rows form groups of rows_per_group consecutive rows (the frames of
 * one channel); 0 means one group, and the last group may be short.  Nothing
 * crosses a group.
 *
 * The values, row t of a group of G rows, bin k, W = smooth_len:
 *   1. Smoothed power S[t][k]:
 *        acc = 0.0;
 *        for j = W - 1 down to 0:  acc = acc + (double)p[max(t - j, 0)][k];
 *        S = (float)(acc / (double)W);
 *      oldest row first, one f64 add each, rows before the group's first taken
 *      as its first; one f64 divide, rounded to float once.
 *   2. Floor M[t][k]: the minimum of S[u][k] over u in [max(t - back, 0),
 *      min(t + ahead, G - 1)] under the total order of vv_dsp/filter/median.h,
 *      -inf < .. < -0 < +0 < .. < +inf < NaN: a NaN is ignored unless the whole
 *      window is NaN, and the result does not depend on how the minimum is
 *      evaluated.  ahead = 0 is the causal tracker; the default window is
 *      centred, for offline batches.
 *   3. Noise r = (double)bias * (double)M, the exact product of two floats; the
 *      plane `noise` is r rounded to float once.
 *   4. Gain.  a = (double)p[t][k]; d = a - r; q = d / a; each one IEEE f64
 *      operation, nothing fused, every comparison as written (a NaN takes the
 *      "else" side), F = (double)floor:
 *        GATE      g = a > r ? 1 : F;
 *        WIENER    g = q > F ? q : F;
 *        SUBTRACT  f2 = F * F;  q = q > f2 ? q : f2;  g = sqrt(q), correctly rounded;
 *      then g = g > 1 ? 1 : g.  The plane `gain` is g rounded to float once.  It
 *      lies in [floor, 1] and is never NaN, whatever the powers (a = 0, r = 0,
 *      NaN and +-inf included).
 * A NaN in `smooth` or `noise` is stored as the quiet NaN 0x7FC00000.
 *
 * No value depends on the number of rows, the pitches, the outputs requested,
 * the entry point or any internal tiling; an output that is not requested costs
 * no store.
 *
 * Checks, in this order, all before any device work:
 *   1. NULL params, rows or out struct -- NULL_POINTER;
 *   2. n_fft < 2, or (device rows) row_pitch or out_pitch < K -- INVALID_SIZE;
 *   3. smooth_len < 1, a negative back or ahead, an unknown mode, a bias that is
 *      not finite or is <= 0, a floor outside [0, 1] or NaN -- OUT_OF_RANGE;
 *   4. smooth_len > VV_DSP_DENOISE_MAX_SMOOTH, back or ahead >
 *      VV_DSP_DENOISE_MAX_REACH, K > VV_DSP_HPSS_MAX_BINS, a group of 2^31 rows
 *      or more, or rows * ceil(K / 16) >= 2^30 (more than one launch takes) --
 *      UNSUPPORTED.
 * Zero rows or no output requested: OK, nothing launched.  With no GPU a call that
 * reaches the computation returns VV_DSP_ERROR_UNSUPPORTED.  An output plane must
 * not overlap the input or another plane; this is not checked. */
#ifndef VV_DSP_SPECTRAL_DENOISE_H
#define VV_DSP_SPECTRAL_DENOISE_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#include "vv_dsp/spectral/hpss.h"
#ifdef __cplusplus
extern "C" {
#endif
#define VV_DSP_DENOISE_MAX_SMOOTH 64
#define VV_DSP_DENOISE_MAX_REACH 511
#define VV_DSP_DENOISE_GATE 0
#define VV_DSP_DENOISE_WIENER 1
#define VV_DSP_DENOISE_SUBTRACT 2
typedef struct vv_dsp_denoise_params {
    size_t      n_fft;        /* a row has K = n_fft/2 + 1 power bins */
    int         smooth_len;   /* W: rows of the running mean, 1 .. VV_DSP_DENOISE_MAX_SMOOTH */
    int         back, ahead;  /* rows of the minimum's window before and after t, 0 .. VV_DSP_DENOISE_MAX_REACH */
    vv_dsp_real bias;         /* finite, > 0: noise = bias x floor (the minimum of a mean of W lies below the mean) */
    vv_dsp_real floor;        /* in [0, 1]: the least gain */
    int         mode;         /* VV_DSP_DENOISE_GATE, _WIENER or _SUBTRACT */
} vv_dsp_denoise_params;
typedef struct vv_dsp_denoise_out {   /* each NULL (not wanted) or [rows][out_pitch], K values of a row written */
    vv_dsp_real *smooth, *noise, *gain;
} vv_dsp_denoise_out;
/* smooth_len 8, back 48, ahead 48, bias 4.0f, floor 0.1f, WIENER.  NULL params: NULL_POINTER. */
vv_dsp_status vv_dsp_denoise_params_default(size_t n_fft, vv_dsp_denoise_params* params);
/* One group of `rows` packed rows (K floats each) in host memory through the same
 * kernel; the planes of `out` are host memory, [rows][K]. */
vv_dsp_status vv_dsp_denoise(const vv_dsp_real* power_rows, size_t rows, const vv_dsp_denoise_params* params,
                             const vv_dsp_denoise_out* out);
#ifdef __cplusplus
}
#endif
#endif
