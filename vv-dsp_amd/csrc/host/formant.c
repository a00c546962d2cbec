/* formant.c -- formants of LPC rows on the MI355X backend (C99).
 * include/vv_dsp/features/formant.h defines the values and the order of the
 * argument checks, all made before any device work by the shim; the root finder
 * and the candidate sort run on the GPU (vvhip_lpc_formants_*, vvhip_formants_*;
 * formant_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/features/formant.h"
#include "vv_dsp/core/framing.h"
#include "vv_dsp_hip.h"

/* vv_dsp_formant_params / _out and vvhip_formant_params / _out have the same
 * members in the same order */
vv_dsp_status vv_dsp_formant_params_default(vv_dsp_real sample_rate, vv_dsp_formant_params* params) {
    if (!params) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_formant_params_default(sample_rate, (vvhip_formant_params*)params);
}

vv_dsp_status vv_dsp_formant_start_points(size_t order, double* out) {
    if (!out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_formant_start_points(order, out);
}

vv_dsp_status vv_dsp_lpc_formants(const vv_dsp_real* a, size_t order, const vv_dsp_formant_params* params,
                                  const vv_dsp_formant_out* out) {
    if (!a || !params || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_formants_host(a, order, (const vvhip_formant_params*)params,
                                                  (const vvhip_formant_out*)out);
}

vv_dsp_status vv_dsp_lpc_formants_device(const vv_dsp_real* d_a, size_t order, size_t batch, size_t a_pitch,
                                         const vv_dsp_formant_params* params, const vv_dsp_formant_out* out,
                                         void* stream) {
    if (!d_a || !params || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_formants_device(d_a, order, batch, a_pitch, (const vvhip_formant_params*)params,
                                                    (const vvhip_formant_out*)out, stream);
}

vv_dsp_status vv_dsp_formants_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                            size_t frame_len, size_t hop_len, int center,
                                            const vv_dsp_real* d_window, size_t order,
                                            const vv_dsp_formant_params* params, const vv_dsp_formant_out* out,
                                            void* stream) {
    if (!d_signal || !params || !out || !(out->freq || out->bw || out->count || out->flags || out->roots))
        return VV_DSP_ERROR_NULL_POINTER;
    if (hop_len == 0 || frame_len == 0 || order < 1 || order + 1 > frame_len) return VV_DSP_ERROR_INVALID_SIZE;
    const size_t frames = vv_dsp_get_num_frames(n, frame_len, hop_len, center);
    return (vv_dsp_status)vvhip_formants_frames_device(d_signal, n, nch, ch_stride, frame_len, hop_len, frames, center,
                                                       d_window, order, (const vvhip_formant_params*)params,
                                                       (const vvhip_formant_out*)out, stream);
}
