/* lpc_filter.h -- LPC rows applied to a signal: the time-varying inverse filter
 * A(z) (the residual) and the time-varying all-pole filter g / A(z) (synthesis).
 * The reference has no such code: this header is the definition, and
 * tests/lpc_filter_util.py is its numpy model.
 *
 * Coefficients: `frames` >= 1 rows a[f][0..p], p = order, 1 <= p <=
 * VV_DSP_LPC_FILTER_MAX_ORDER, in vv_dsp_levinson's convention A(z) = 1 + sum
 * a[m] z^-m.  a[0] is ignored and taken as 1.
 *
 * Which row governs a sample.  Sample t of a call (0-based) is governed by row
 *   f(t) = clamp(floor((t + offset) / seg_len), 0, frames - 1),
 * seg_len >= 1, offset signed: t + offset < 0 gives row 0 and the last row holds
 * to the end of the signal.  The rows are piecewise constant on purpose; smooth
 * envelopes are made by interpolating LSF rows (lsf.h) to a shorter seg_len and
 * converting back.  An optional gain plane g[f] (NULL: 1) is indexed by the same
 * f(t).
 *
 * Arithmetic.  Every value is widened to f64; every operation below is one IEEE
 * f64 operation, nothing fused, k ascending.
 *   Residual:  acc = (double)x[t]; for k = 1..p: acc = acc + (double)a[f][k] *
 *     X[t-k]; with a gain plane acc = acc / (double)g[f]; e[t] = (float)acc.
 *   Synthesis: acc = (double)e[t], or (double)g[f] * (double)e[t] with a gain
 *     plane; for k = 1..p: acc = acc - (double)a[f][k] * Y[t-k]; Y[t] = acc, kept
 *     in f64; y[t] = (float)acc.
 * The synthesis history is the f64 value, not the rounded output: cutting the
 * recursion into chunks then changes a float of the output almost never.
 *
 * History and state.  X (the inputs as doubles) and Y before sample 0 come from
 * state[0..p), doubles, newest first: state[k-1] is the value at t = -k.  NULL:
 * zeros.  A state that is given is overwritten with the last p values (when
 * n < p the older entries shift), so one call equals the same signal fed in any
 * two pieces with offset advanced by the first piece's length.
 *
 * A NaN output is stored as the quiet NaN 0x7FC00000.  Rows are not checked for
 * stability: the arithmetic decides.  y may be e (synthesis in place); the
 * residual's output may not overlap its input.
 *
 * The residual is fully parallel and always these bits.  Synthesis of rows of
 * n <= VV_DSP_LPC_SYNTH_EXACT_MAX samples is one recursion per row and always
 * these bits.  Longer rows are cut into chunks of VV_DSP_LPC_SYNTH_CHUNK samples
 * (independent of seg_len): each chunk's zero-state end values and its p x p
 * state transition are computed in f64, a scan carries the states over the
 * chunks, and every chunk is walked again from its state by the recursion above.
 * The chunks' incoming states then differ from the sequential ones by f64
 * rounding only.  No value depends on the batch, the strides or the entry point.
 *
 * Checks, in this order and before any device work: a NULL required pointer:
 * NULL_POINTER; order < 1, seg_len == 0, frames == 0, or a pitch or stride
 * shorter than its row: INVALID_SIZE; order > VV_DSP_LPC_FILTER_MAX_ORDER:
 * UNSUPPORTED; what one call cannot address -- n >= 2^31 - 64, 2^31 or more
 * channels, rows or floats of pitch, seg_len >= 2^40 or |offset| >= 2^40:
 * INVALID_SIZE; n == 0 (or no channels): OK, nothing written; no GPU:
 * UNSUPPORTED.  The batched device entry points are in vv_dsp_amd.h. */
#ifndef VV_DSP_ENVELOPE_LPC_FILTER_H
#define VV_DSP_ENVELOPE_LPC_FILTER_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
#define VV_DSP_LPC_FILTER_MAX_ORDER 32
/* synthesis rows up to here run as one recursion */
#define VV_DSP_LPC_SYNTH_EXACT_MAX 8192
/* chunk length of longer rows */
#define VV_DSP_LPC_SYNTH_CHUNK 1024

/* one host channel x[n] through host rows a[frames][order + 1] -> e[n];
 * gain [frames] and state [order] may be NULL */
vv_dsp_status vv_dsp_lpc_residual(const vv_dsp_real* x, size_t n, const vv_dsp_real* a, size_t order, size_t frames,
                                  size_t seg_len, long long offset, const vv_dsp_real* gain, double* state,
                                  vv_dsp_real* e);
/* one host channel e[n] -> y[n]; y may be e */
vv_dsp_status vv_dsp_lpc_synth(const vv_dsp_real* e, size_t n, const vv_dsp_real* a, size_t order, size_t frames,
                               size_t seg_len, long long offset, const vv_dsp_real* gain, double* state,
                               vv_dsp_real* y);
#ifdef __cplusplus
}
#endif
#endif
