/* envelope.h -- the envelope module: real cepstrum, minimum phase, LPC, LSF,
 * the LPC residual and synthesis filters
 * (reference include/vv_dsp/envelope.h). */
#ifndef VV_DSP_ENVELOPE_H
#define VV_DSP_ENVELOPE_H
#include "vv_dsp/envelope/cepstrum.h"
#include "vv_dsp/envelope/minphase.h"
#include "vv_dsp/envelope/lpc.h"
#include "vv_dsp/envelope/lsf.h"
#include "vv_dsp/envelope/lpc_filter.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the module's link check: returns 5 */
int vv_dsp_envelope_dummy(void);
#ifdef __cplusplus
}
#endif
#endif
