/* lsf.h -- LPC rows as line spectral frequencies and reflection coefficients,
 * and back.  The reference has no such code: this header is the definition,
 * and tests/lsf_util.py is its numpy model.
 *
 * Input: a row a[0..p], p = order, 1 <= p <= VV_DSP_LSF_MAX_ORDER, in
 * vv_dsp_levinson's convention A(z) = 1 + sum a[m] z^-m.  a[0] is ignored and
 * taken as 1.  Every value is (double)a[m]; every operation below is one IEEE
 * f64 operation, nothing fused.
 *
 * Reflection coefficients rc[0..p) and VV_DSP_LSF_STABLE, by the step-down
 * recursion.  c = a; for m = p down to 1: k = c[m], rc[m-1] = (float)k,
 * den = 1 - k*k, c'[i] = (c[i] - k*c[m-i]) / den for i = 1..m-1.  If
 * !(fabs(k) < 1) at some m: STABLE is clear, rc[m-1] keeps k, every lower
 * entry is the quiet NaN 0x7FC00000 and the recursion stops.  A NaN k is stored
 * as that quiet NaN too, whatever its sign and payload.
 *
 * LSF lsf[0..p) in radians in (0, pi), ascending, and VV_DSP_LSF_COMPLETE, by
 * the Kabal-Ramachandran scan.  With a[p+1] = 0: P[k] = a[k] + a[p+1-k],
 * Q[k] = a[k] - a[p+1-k].  The trivial roots are removed:
 *   even p: f1[k] = P[k] - f1[k-1], f2[k] = Q[k] + f2[k-1], k = 0..p/2;
 *   odd p:  f1[k] = P[k], k = 0..(p+1)/2, f2[k] = Q[k] + f2[k-2], k = 0..(p-1)/2;
 * a term with a negative index is not added or subtracted at all (f1[0] = P[0],
 * f2[0] = Q[0], odd p: f2[1] = Q[1]).  A half-polynomial of M+1 entries is the
 * Chebyshev series c[0] = f[M], c[n] = 2*f[M-n], evaluated by Clenshaw: b1 =
 * b2 = 0; for n = M..1: b = ((2*x)*b1 - b2) + c[n], b2 = b1, b1 = b; then
 * S = (x*b1 - b2) + c[0].
 *
 * The grid has G = VV_DSP_LSF_GRID cells and is defined by arithmetic alone:
 * x[0] = 1, x[1] = VV_DSP_LSF_CG (the double nearest cos(pi/256)), x[i] =
 * (2*CG)*x[i-1] - x[i-2] for i = 2..G-1, x[G] = -1.  It is within 5.6e-13 of
 * cos(pi i/G) and strictly decreasing.
 *
 * Cell i brackets a root of S when (S(x[i]) < 0) != (S(x[i+1]) < 0); a zero or
 * a NaN counts as not negative.  A bracket [lo, hi] = [x[i], x[i+1]] is
 * bisected 32 times: mid = 0.5*(lo+hi); the endpoint whose sign class equals
 * mid's is replaced (lo when (S(mid) < 0) == (S(lo) < 0) of the cell's first
 * grid point, else hi); the root is 0.5*(lo+hi) of the last interval.
 *
 * COMPLETE is set when the scan of f1 finds exactly M1 brackets and the scan of
 * f2 exactly M2 (the degrees above) and the roots, u[k] of f1 and v[k] of f2 in
 * cell order, interlace strictly: u[k] > v[k] for every k < M2 and v[k] >
 * u[k+1] for every k+1 < M1.  Then lsf[2k] = (float)acos(u[k]) and lsf[2k+1] =
 * (float)acos(v[k]), f64 acos.  Otherwise the row's lsf is the quiet NaN
 * throughout.
 *
 * LSF -> LPC.  ck is the cosine of w = (double)lsf[k] by arithmetic alone, so
 * that no math library stands between an LSF row and its coefficients (a last
 * bit of a library cosine moves a coefficient that cancels to near zero by many
 * float ulps): t = (w - PIO2_HI) - PIO2_LO with PIO2_HI = VV_DSP_LSF_PIO2_HI,
 * the double nearest pi/2, and PIO2_LO = VV_DSP_LSF_PIO2_LO, the double nearest
 * the rest; s = t*t; q = C[11], then q = q*s + C[i] for i = 10..0, with C[0] = 1
 * and C[i] = -C[i-1] / (double)((2i)*(2i+1)); ck = -(t*q).  That is -sin(t) by
 * its Taylor series to t^23, within 4e-16 of cos(w) for 0 <= w <= pi; outside
 * that range the arithmetic decides.  F1 and F2 are arrays of p+2
 * entries, {1, 0, ...}.  For k ascending, F1 for even k and F2 for odd k takes
 * the factor (1 - 2ck z^-1 + z^-2): new[i] = (old[i] - (2*ck)*old[i-1]) +
 * old[i-2] for every i = 0..p+1, an entry with a negative index being +0.0 and
 * the arithmetic still done.  Then, entries with a negative index again +0.0,
 *   even p: P[i] = F1[i] + F1[i-1], Q[i] = F2[i] - F2[i-1];
 *   odd p:  P[i] = F1[i],           Q[i] = F2[i] - F2[i-2];
 * a[0] = 1 and a[m] = (float)(0.5*(P[m] + Q[m])), m = 1..p, a NaN stored as the
 * quiet NaN 0x7FC00000.  The input is not checked for order or range: the
 * arithmetic decides.
 *
 * No value depends on the batch, the pitch, the outputs requested, the entry
 * point or how rows share a wave.  lsf goes through the device's acos and may
 * differ from another library's by the last f64 bit before rounding to float.
 *
 * Checks, in this order and before any device work: a NULL required pointer or
 * an all-NULL output set: NULL_POINTER; order < 1 or a pitch below order + 1:
 * INVALID_SIZE; order > VV_DSP_LSF_MAX_ORDER: UNSUPPORTED.  No GPU: UNSUPPORTED.
 * The batched device entry points are in vv_dsp_amd.h. */
#ifndef VV_DSP_ENVELOPE_LSF_H
#define VV_DSP_ENVELOPE_LSF_H
#include <stddef.h>
#include <stdint.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
#define VV_DSP_LSF_MAX_ORDER 32
#define VV_DSP_LSF_GRID 256
/* the double nearest cos(pi/256) */
#define VV_DSP_LSF_CG 0x1.fff62169b92dbp-1
#define VV_DSP_LSF_BISECTIONS 32
/* pi/2 as the nearest double and the double nearest the rest */
#define VV_DSP_LSF_PIO2_HI 0x1.921fb54442d18p+0
#define VV_DSP_LSF_PIO2_LO 0x1.1a62633145c07p-54
#define VV_DSP_LSF_COS_TERMS 12
/* bits of the flags word of a row */
#define VV_DSP_LSF_STABLE 1
#define VV_DSP_LSF_COMPLETE 2

/* one host row a[order+1] -> lsf_out[order], rc_out[order], *flags_out; any
 * output may be NULL, not all of them */
vv_dsp_status vv_dsp_lpc_to_lsf(const vv_dsp_real* a, size_t order, vv_dsp_real* lsf_out, vv_dsp_real* rc_out,
                                int32_t* flags_out);
/* one host row lsf[order] -> a_out[order+1] */
vv_dsp_status vv_dsp_lsf_to_lpc(const vv_dsp_real* lsf, size_t order, vv_dsp_real* a_out);
#ifdef __cplusplus
}
#endif
#endif
