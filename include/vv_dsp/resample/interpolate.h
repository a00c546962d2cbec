/* interpolate.h -- single-position interpolation API (reference
 * include/vv_dsp/resample/interpolate.h:17-29; semantics of
 * src/resample/interpolate.c:4-64), bit-identical to the reference.
 *
 * These two functions exist for source compatibility: each call stages the row
 * and one position through the device for one value.  The product is the
 * batched forms in vv_dsp/vv_dsp_amd.h (vv_dsp_interpolate_device,
 * vv_dsp_interpolate_uniform_device, vv_dsp_interpolate_real_batch), which read
 * whole rows along a curve of positions in one launch.  No value is computed on
 * the CPU: with no device they return VV_DSP_ERROR_UNSUPPORTED and leave *out
 * untouched. */
#ifndef VV_DSP_RESAMPLE_INTERPOLATE_H
#define VV_DSP_RESAMPLE_INTERPOLATE_H
#include "vv_dsp/vv_dsp_types.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Checks in the reference's order: x or out NULL -> VV_DSP_ERROR_NULL_POINTER;
 * n == 0 -> VV_DSP_ERROR_INVALID_SIZE.  pos <= 0 gives x[0], pos >= (float)(n - 1)
 * gives x[n - 1]; a NaN pos (undefined in the reference) gives NaN.
 * Linear: (1 - t) x[i] + t x[i + 1] with i = floor(pos), t = pos - i. */
vv_dsp_status vv_dsp_interpolate_linear_real(const vv_dsp_real* x, size_t n, vv_dsp_real pos, vv_dsp_real* out);
/* Cubic: Catmull-Rom through x[i - 1], x[i], x[i + 1], x[i + 2] with the indices
 * clamped into the row; x[0] when n < 2, whatever pos. */
vv_dsp_status vv_dsp_interpolate_cubic_real(const vv_dsp_real* x, size_t n, vv_dsp_real pos, vv_dsp_real* out);

#ifdef __cplusplus
}
#endif
#endif
