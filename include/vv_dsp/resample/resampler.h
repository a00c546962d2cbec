/* resampler.h -- fixed-ratio resampler API (reference
 * include/vv_dsp/resample/resampler.h:10-37; semantics of
 * src/resample/resampler.c:16-119).  Linear interpolation is bit-identical to
 * the reference; the windowed-sinc path follows its arithmetic (f64 centre,
 * sinc rounded to f32, Hann indexed by tap, row normalised by its sum) through
 * a polyphase table and agrees within the harness tolerance.  The batched
 * device form is in vv_dsp/vv_dsp_amd.h. */
#ifndef VV_DSP_RESAMPLE_RESAMPLER_H
#define VV_DSP_RESAMPLE_RESAMPLER_H
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vv_dsp_resampler vv_dsp_resampler; /* opaque */

/* out_rate / in_rate = ratio_num / ratio_den, both > 0; NULL on a zero or no memory */
vv_dsp_resampler* vv_dsp_resampler_create(unsigned int ratio_num, unsigned int ratio_den);
void vv_dsp_resampler_destroy(vv_dsp_resampler* rs);
/* VV_DSP_ERROR_OUT_OF_RANGE for a zero numerator or denominator */
int vv_dsp_resampler_set_ratio(vv_dsp_resampler* rs, unsigned int ratio_num, unsigned int ratio_den);
/* use_sinc 0: linear interpolation, else windowed sinc with `taps` taps
 * (clamped to 4..128; an odd count is raised by one when processing) */
int vv_dsp_resampler_set_quality(vv_dsp_resampler* rs, int use_sinc, unsigned int taps);
/* A whole contiguous buffer per call: floor((in_n - 1) * ratio) + 1 outputs.
 * Checks in the reference's order: null pointers; in_n == 0 -> *out_n = 0, OK;
 * more outputs than out_cap -> VV_DSP_ERROR_INVALID_SIZE.  Runs on the device
 * (host pointers are staged through it); VV_DSP_ERROR_UNSUPPORTED with none. */
int vv_dsp_resampler_process_real(vv_dsp_resampler* rs, const vv_dsp_real* in, size_t in_n, vv_dsp_real* out,
                                  size_t out_cap, size_t* out_n);

#ifdef __cplusplus
}
#endif
#endif
