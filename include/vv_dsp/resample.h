/* resample.h -- the resample module: interpolation at fractional positions and
 * the fixed-ratio resampler (reference include/vv_dsp/resample.h). */
#ifndef VV_DSP_RESAMPLE_H
#define VV_DSP_RESAMPLE_H
#include "vv_dsp/resample/interpolate.h"
#include "vv_dsp/resample/resampler.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the module's link check: returns 3 */
int vv_dsp_resample_dummy(void);
#ifdef __cplusplus
}
#endif
#endif
