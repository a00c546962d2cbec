/* filter.h -- the filter module: FIR, filtfilt, biquad IIR, Savitzky-Golay
 * (reference include/vv_dsp/filter.h). */
#ifndef VV_DSP_FILTER_H
#define VV_DSP_FILTER_H
#include "vv_dsp/filter/common.h"
#include "vv_dsp/filter/fir.h"
#include "vv_dsp/filter/iir.h"
#include "vv_dsp/filter/savgol.h"
#include "vv_dsp/filter/median.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the module's link check: returns 7 */
int vv_dsp_filter_dummy(void);
#ifdef __cplusplus
}
#endif
#endif
