/* iir.h -- biquad cascades, Direct Form II Transposed (reference
 * include/vv_dsp/filter/iir.h:14-35). */
#ifndef VV_DSP_FILTER_IIR_H
#define VV_DSP_FILTER_IIR_H
#include <stddef.h>
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif
/* one second-order section, a0 = 1; the field order is ABI */
typedef struct {
    vv_dsp_real a1, a2, b0, b1, b2;
    vv_dsp_real z1, z2; /* state */
} vv_dsp_biquad;

/* sets the coefficients and clears the state */
vv_dsp_status vv_dsp_biquad_init(vv_dsp_biquad* biquad, vv_dsp_real b0, vv_dsp_real b1, vv_dsp_real b2,
                                 vv_dsp_real a1, vv_dsp_real a2);
void vv_dsp_biquad_reset(vv_dsp_biquad* biquad);
/* y = b0 x + z1; z1 = b1 x - a1 y + z2; z2 = b2 x - a2 y.  One sample through
 * the device (vv_dsp_iir_apply on one stage): a launch per sample, kept for
 * link compatibility and the state protocol.  With no device: NaN, state
 * untouched, vvhip_last_error() set. */
vv_dsp_real vv_dsp_biquad_process(vv_dsp_biquad* biquad, vv_dsp_real input_sample);
/* the cascade over num_samples samples, continuing from and updating each
 * stage's z1, z2; output may be input; num_stages = 0 copies */
vv_dsp_status vv_dsp_iir_apply(vv_dsp_biquad* biquads, size_t num_stages, const vv_dsp_real* input,
                               vv_dsp_real* output, size_t num_samples);
#ifdef __cplusplus
}
#endif
#endif
