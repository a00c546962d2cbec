/* iir.c -- biquad cascades on the MI355X backend (C99).
 * Semantics and argument checks of the reference's src/filter/iir.c:3-43, in
 * its order.  init and reset are plain setters; every sample runs on the GPU
 * (vvhip_iir_*; iir_kernels.hip) -- vv_dsp_biquad_process too, one launch per
 * sample: it exists for link compatibility and the state protocol, not speed. */
#include <math.h>
#include <stdlib.h>

#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/filter.h"
#include "vv_dsp_hip.h"

int vv_dsp_filter_dummy(void) { return 7; }

vv_dsp_status vv_dsp_biquad_init(vv_dsp_biquad* bq, vv_dsp_real b0, vv_dsp_real b1, vv_dsp_real b2, vv_dsp_real a1,
                                 vv_dsp_real a2) {
    if (!bq) return VV_DSP_ERROR_NULL_POINTER;
    bq->a1 = a1;
    bq->a2 = a2;
    bq->b0 = b0;
    bq->b1 = b1;
    bq->b2 = b2;
    vv_dsp_biquad_reset(bq);
    return VV_DSP_OK;
}

void vv_dsp_biquad_reset(vv_dsp_biquad* bq) {
    if (bq) bq->z1 = bq->z2 = 0;
}

vv_dsp_status vv_dsp_iir_apply(vv_dsp_biquad* biquads, size_t num_stages, const vv_dsp_real* input,
                               vv_dsp_real* output, size_t n) {
    if (!input || !output || (!biquads && num_stages > 0)) return VV_DSP_ERROR_NULL_POINTER;
    if (n == 0) return VV_DSP_OK;
    /* the shim's layout: coef [stages][5] = b0 b1 b2 a1 a2, then state [stages][2] = z1 z2 */
    float* packed = NULL;
    if (num_stages > 0) {
        if (num_stages > ((size_t)-1) / (7 * sizeof(float))) return VV_DSP_ERROR_INVALID_SIZE;
        packed = (float*)malloc(7 * sizeof(float) * num_stages);
        if (!packed) return VV_DSP_ERROR_INTERNAL;
    }
    float* state = packed ? packed + 5 * num_stages : NULL;
    for (size_t s = 0; s < num_stages; ++s) {
        packed[5 * s + 0] = biquads[s].b0;
        packed[5 * s + 1] = biquads[s].b1;
        packed[5 * s + 2] = biquads[s].b2;
        packed[5 * s + 3] = biquads[s].a1;
        packed[5 * s + 4] = biquads[s].a2;
        state[2 * s + 0] = biquads[s].z1;
        state[2 * s + 1] = biquads[s].z2;
    }
    const vv_dsp_status st = (vv_dsp_status)vvhip_iir_host(packed, num_stages, state, input, output, n);
    if (st == VV_DSP_OK) {
        for (size_t s = 0; s < num_stages; ++s) {
            biquads[s].z1 = state[2 * s + 0];
            biquads[s].z2 = state[2 * s + 1];
        }
    }
    free(packed);
    return st;
}

vv_dsp_real vv_dsp_biquad_process(vv_dsp_biquad* bq, vv_dsp_real x) {
    vv_dsp_real y = (vv_dsp_real)NAN;
    if (!bq) {
        vvhip_set_error("vv_dsp_biquad_process: NULL biquad");
        return y;
    }
    if (vv_dsp_iir_apply(bq, 1, &x, &y, 1) != VV_DSP_OK) return (vv_dsp_real)NAN;   /* state untouched, error text set */
    return y;
}

vv_dsp_status vv_dsp_iir_apply_device(const vv_dsp_real* d_coef, size_t num_stages, vv_dsp_real* d_state,
                                      const vv_dsp_real* d_x, vv_dsp_real* d_y, size_t n, size_t batch,
                                      size_t x_stride, size_t y_stride, void* stream) {
    if (!d_x || !d_y || (!d_coef && num_stages > 0)) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_iir_device(d_coef, num_stages, d_state, d_x, d_y, n, batch, x_stride, y_stride, stream);
}
