/* formant.h -- the poles of 1/A(z) of an LPC row as formant frequencies and
 * bandwidths.  The reference has no such code: this header is the definition,
 * and tests/formant_util.py is its numpy model.  Formant analysis usually
 * pre-emphasises the signal first (y[n] = x[n] - 0.97 x[n-1] or so); the caller
 * does that with the direct-form FIR (vv_dsp/filter/fir.h).
 *
 * Input: a row a[0..p], p = order, 1 <= p <= VV_DSP_FORMANT_MAX_ORDER, A(z) =
 * 1 + sum a[m] z^-m (vv_dsp_levinson's convention); a[0] is ignored, every
 * value is (double)a[m], every operation is one IEEE f64 operation, nothing
 * fused.
 *
 * Roots of z^p + a[1] z^(p-1) + ... + a[p] by Aberth-Ehrlich, all p updated
 * together (Jacobi).  Complex arithmetic in real operations:
 *   product  (ar + i ai)(br + i bi) = (ar*br - ai*bi, ar*bi + ai*br);
 *   quotient (x + i y)/(u + i v): n = u*u + v*v, ((x*u + y*v)/n, (y*u - x*v)/n);
 *   a reciprocal is the quotient with x = 1, y = 0, spelled out in full.
 * Start points z_i = 0.9 (cos t_i, sin t_i), t_i = (6.283185307179586*i)/p +
 * 0.4, host f64 arithmetic exported as vv_dsp_formant_start_points (needs no
 * device); the kernels read that table.
 *
 * One iteration, for every root i of the row from the same old iterate:
 *   Horner with b = (1, 0), d = (0, 0); for m = 1..p: d = d*z + b (product,
 *     then both parts added), then b = b*z with a[m] added to the real part;
 *   w = b/d;
 *   s = (0, 0); for j = 0..p-1, j != i, ascending: s += 1/(z_i - z_j);
 *   t = w*s; delta = w / (1 - t.re, -t.im);
 *   z_i = z_i - delta.
 * A row has converged after the first iteration in which delta.re^2 +
 * delta.im^2 < 1e-26 for every i; from then on it is frozen whatever its
 * neighbours in a wave do.  A row stops unconverged after
 * VV_DSP_FORMANT_MAX_ITER iterations, or after the first iteration in which a
 * part of some delta is not finite; in that second case its roots plane is the
 * quiet NaN 0x7FF8000000000000 throughout.  A silent row, every a[m] == 0 for m
 * >= 1, is converged with no candidates and is not iterated: its roots are the
 * start points.
 *
 * Candidates.  For each root with im > 0: c = (double)sample_rate /
 * 6.283185307179586, f = atan2(im, re) * c, r2 = re*re + im*im, bw =
 * -(log(r2) * c).  Kept when f >= f_min, f <= f_max, bw > 0 and bw <= bw_max (a
 * NaN fails every test).  Kept candidates are sorted by f ascending, ties by
 * root index, and the first n_formants are written as floats.
 *
 * Outputs, each may be NULL: freq and bw [rows][n_formants], entries past the
 * count the quiet NaN 0x7FC00000; count [rows] int32, the number written (at
 * most n_formants); flags [rows] int32 with VV_DSP_FORMANT_CONVERGED; roots
 * [rows][order][2] double, the final iterate in root-index order.  A row that
 * has not converged has count 0 and NaN freq / bw.
 *
 * No value depends on the batch, the pitch, the outputs requested, the entry
 * point or how rows share a wave.  freq and bw go through the device's atan2 /
 * log and may differ from another library's by the last f64 bit before
 * rounding to float.
 *
 * Checks, in this order and before any device work: a NULL required pointer or
 * an all-NULL output set: NULL_POINTER; order < 1 or a pitch below order + 1:
 * INVALID_SIZE; a non-finite or non-positive sample_rate, f_min > f_max, a NaN
 * threshold, n_formants outside 1..VV_DSP_FORMANT_MAX_FORMANTS: OUT_OF_RANGE;
 * order > VV_DSP_FORMANT_MAX_ORDER: UNSUPPORTED.  No GPU: UNSUPPORTED.  The
 * batched device entry points are in vv_dsp_amd.h. */
#ifndef VV_DSP_FEATURES_FORMANT_H
#define VV_DSP_FEATURES_FORMANT_H
#include <stddef.h>
#include <stdint.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
#define VV_DSP_FORMANT_MAX_ORDER 32
#define VV_DSP_FORMANT_MAX_FORMANTS 16
#define VV_DSP_FORMANT_MAX_ITER 48
/* the bit of the flags word of a row */
#define VV_DSP_FORMANT_CONVERGED 1

typedef struct vv_dsp_formant_params {
    vv_dsp_real sample_rate; /* Hz */
    vv_dsp_real f_min;       /* candidates with f_min <= f <= f_max ... */
    vv_dsp_real f_max;
    vv_dsp_real bw_max;      /* ... and 0 < bw <= bw_max are kept */
    uint32_t n_formants;     /* 1..VV_DSP_FORMANT_MAX_FORMANTS */
} vv_dsp_formant_params;

/* one device (or, for vv_dsp_lpc_formants, host) pointer per output, NULL = not wanted */
typedef struct vv_dsp_formant_out {
    vv_dsp_real* freq;
    vv_dsp_real* bw;
    int32_t* count;
    int32_t* flags;
    double* roots;
} vv_dsp_formant_out;

/* f_min 50 Hz, f_max sample_rate/2 - 50, bw_max 600 Hz, 5 formants */
vv_dsp_status vv_dsp_formant_params_default(vv_dsp_real sample_rate, vv_dsp_formant_params* params);
/* out[2*i], out[2*i+1] = the start point z_i, i < order; order 1..VV_DSP_FORMANT_MAX_ORDER,
 * else OUT_OF_RANGE.  Host arithmetic, needs no device. */
vv_dsp_status vv_dsp_formant_start_points(size_t order, double* out);
/* one host row a[order+1] */
vv_dsp_status vv_dsp_lpc_formants(const vv_dsp_real* a, size_t order, const vv_dsp_formant_params* params,
                                  const vv_dsp_formant_out* out);
#ifdef __cplusplus
}
#endif
#endif
