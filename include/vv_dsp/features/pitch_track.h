/* pitch_track.h -- one f0 contour from the YIN curves of consecutive frames: a
 * Viterbi path over (lag, frame) with an unvoiced state.  pitch.h decides every
 * frame on its own (the first lag under the threshold), which puts a frame with
 * a weak fundamental an octave high and lets a noisy frame flip between voiced
 * and unvoiced; the path below pays for every change of lag and of voicing, so
 * it stays on the contour.  The reference library has no pitch code, so this
 * header is the definition.  Every operation below is an f64 add, multiply,
 * divide or strict comparison in a stated order, each rounded once (no fused
 * multiply-add) and no sum whose order is free: an implementation equals the
 * definition bit for bit, ties included.  The forward pass and the backtrace run
 * on the GPU (pitch_track_kernels.hip); the device forms are in vv_dsp_amd.h
 * (vv_dsp_pitch_track_device, vv_dsp_pitch_track_frames_device).
 *
 * Input: one channel's curves q[t][0 .. tau_max], float32, t = 0 .. F - 1, as
 * vv_dsp_pitch_device / vv_dsp_pitch_frames_device export them (cmnd).  Values
 * are expected in [0, +inf] or NaN (d' is never negative; -inf is outside the
 * definition).
 *
 * States: the S = tau_max - tau_min + 1 lags tau_min .. tau_max and the unvoiced
 * state U.  lambda, jump_cost, switch_cost, unvoiced_cost are converted to
 * double once; B = max_step.
 *
 * Costs (all f64):
 *   O(t, tau) = (double)q[t][tau], +inf where that is NaN;  O(t, U) = unvoiced_cost
 *   r(tau)    = lambda / (double)tau
 *   D(0, tau) = O(0, tau);  D(0, U) = unvoiced_cost
 *
 * Step t >= 1.  s* = the lowest lag that attains min over tau of D(t-1, tau).
 *   A voiced state tau examines, in this order, a candidate replacing the best so
 *   far only where it is strictly smaller:
 *     1. U:     D(t-1, U) + switch_cost
 *     2. jump:  D(t-1, s*) + jump_cost
 *     3. tau' = max(tau_min, tau - B) .. min(tau_max, tau + B), ascending:
 *               D(t-1, tau') + p,  p = fl((double)|tau - tau'| * r(tau)), the
 *               product rounded before the add
 *   D(t, tau) = best + O(t, tau), and the winning candidate is the predecessor.
 *   The unvoiced state examines  1. U: D(t-1, U)   2. D(t-1, s*) + switch_cost
 *   and D(t, U) = best + unvoiced_cost.
 *
 * End.  The end state is U, or the lowest lag that attains min over tau of
 * D(F-1, tau) where that minimum is strictly smaller than D(F-1, U).  The path
 * is the end state's chain of predecessors back to t = 0.
 *
 * Outputs, each pointer NULL (not wanted) or one value per frame (cost: one per
 * channel):
 *   lag          uint32, the path's lag at the frame, 0 = unvoiced
 *   f0           0 for an unvoiced frame; else with tau = lag, b = (double)q[t][tau]
 *                and, where tau - 1 >= 1 and tau + 1 <= tau_max, a = (double)
 *                q[t][tau-1], c = (double)q[t][tau+1]: off = (a - c) / (2 ((a - 2b)
 *                + c)) where a >= b, c >= b and (a - 2b) + c > 0, else off = 0 (pitch.h's
 *                parabola rule); f0 = fs / ((double)tau + off) in f64, rounded to
 *                float once
 *   aperiodicity q[t][lag] for a voiced frame; for an unvoiced frame the first
 *                minimum of q[t][tau_min .. tau_max], NaN values skipped (NaN where
 *                every value is NaN)
 *   cost         double, D(F-1, end state)
 * A value never depends on the number of channels, the strides, the outputs
 * requested or the entry point.
 *
 * Checks, in this order, all before any device work:
 *   1. NULL curves, params or out -- NULL_POINTER;
 *   2. F == 0 -- OK, nothing written;
 *   3. tau_min < 1, tau_min >= tau_max, a non-finite or negative lambda, jump_cost,
 *      switch_cost or unvoiced_cost, a non-finite or non-positive sample_rate --
 *      OUT_OF_RANGE;
 *   4. a row stride below tau_max + 1 (or a channel stride shorter than its
 *      channel) -- INVALID_SIZE;
 *   5. max_step > VV_DSP_PITCH_TRACK_MAX_STEP, S > VV_DSP_PITCH_TRACK_MAX_STATES
 *      or F >= 2^31 -- UNSUPPORTED;
 *   6. no output wanted (or, device forms, no channel) -- OK, nothing launched;
 *   7. no GPU -- UNSUPPORTED. */
#ifndef VV_DSP_FEATURES_PITCH_TRACK_H
#define VV_DSP_FEATURES_PITCH_TRACK_H
#include <stddef.h>
#include <stdint.h>
#include "vv_dsp/vv_dsp_types.h"
#include "vv_dsp/features/pitch.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the kernel's limits: a predecessor is one byte (U, jump or one of 2 B + 1 band
 * offsets), and the two D vectors of a channel sit in one CU's LDS */
#define VV_DSP_PITCH_TRACK_MAX_STEP 126
#define VV_DSP_PITCH_TRACK_MAX_STATES 4096
typedef struct vv_dsp_pitch_track_params {
    vv_dsp_real sample_rate;      /* Hz, for f0 */
    uint32_t tau_min, tau_max;    /* the lags that are states; the curves have tau_max + 1 values */
    vv_dsp_real lambda;           /* a step of k lags from tau costs k * lambda / tau */
    vv_dsp_real jump_cost;        /* to any lag from the best lag of the frame before */
    vv_dsp_real switch_cost;      /* between voiced and unvoiced */
    vv_dsp_real unvoiced_cost;    /* of one unvoiced frame (a voiced one costs its d') */
    uint32_t max_step;            /* B: the lags a step may move without a jump */
} vv_dsp_pitch_track_params;
typedef struct vv_dsp_pitch_track_out {   /* each NULL (not wanted) or per frame; cost per channel */
    uint32_t* lag;
    vv_dsp_real *f0, *aperiodicity;
    double* cost;
} vv_dsp_pitch_track_out;
/* The tracker's parameters for the curves of `pitch` on frames of frame_len
 * samples: sample_rate, the lag range of vv_dsp_pitch_lag_range (and its checks
 * and statuses), lambda 4, max_step 8, jump_cost 0.5, switch_cost 0.3,
 * unvoiced_cost 0.35.  Nothing is written unless the result is VV_DSP_OK. */
vv_dsp_status vv_dsp_pitch_track_params_default(const vv_dsp_pitch_params* pitch, size_t frame_len,
                                                vv_dsp_pitch_track_params* track);
/* One channel of curves in host memory, rows row_stride floats apart; only the
 * tau_max + 1 values of each row go to the device. */
vv_dsp_status vv_dsp_pitch_track(const vv_dsp_real* curves, size_t frames, size_t row_stride,
                                 const vv_dsp_pitch_track_params* params, const vv_dsp_pitch_track_out* out);
#ifdef __cplusplus
}
#endif
#endif
