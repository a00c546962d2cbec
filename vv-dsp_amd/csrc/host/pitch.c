/* pitch.c -- fundamental frequency by YIN on the MI355X backend (C99).
 * include/vv_dsp/features/pitch.h defines the algorithm and the order of the
 * argument checks (NULL pointers, n == 0, the parameters' ranges, the
 * integration length, the kernel's limits), all made before any device work by
 * the shim; every sum and decision runs on the GPU (vvhip_pitch_*;
 * pitch_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/features/pitch.h"
#include "vv_dsp/core/framing.h"
#include "vv_dsp_hip.h"

/* vv_dsp_pitch_params / vv_dsp_pitch_out and vvhip_pitch_params / vvhip_pitch_out
 * have the same members in the same order */
vv_dsp_status vv_dsp_pitch_lag_range(const vv_dsp_pitch_params* params, size_t frame_len, size_t* tau_min,
                                     size_t* tau_max, size_t* integration_len) {
    if (!params) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pitch_lag_range((const vvhip_pitch_params*)params, frame_len, tau_min, tau_max,
                                                integration_len);
}

vv_dsp_status vv_dsp_pitch_yin(const vv_dsp_real* x, size_t n, const vv_dsp_pitch_params* params, vv_dsp_real* f0,
                               vv_dsp_real* aperiodicity) {
    if (!x || !params) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pitch_host(x, n, (const vvhip_pitch_params*)params, f0, aperiodicity);
}

vv_dsp_status vv_dsp_pitch_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t row_stride,
                                  const vv_dsp_pitch_params* params, const vv_dsp_pitch_out* out,
                                  size_t cmnd_row_stride, void* stream) {
    if (!d_x || !params || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pitch_device(d_x, n, batch, row_stride, (const vvhip_pitch_params*)params,
                                             (const vvhip_pitch_out*)out, cmnd_row_stride, stream);
}

vv_dsp_status vv_dsp_pitch_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                         size_t frame_len, size_t hop_len, int center, const vv_dsp_real* d_window,
                                         const vv_dsp_pitch_params* params, const vv_dsp_pitch_out* out,
                                         size_t out_ch_stride, size_t cmnd_ch_stride, void* stream) {
    if (!d_signal || !params || !out) return VV_DSP_ERROR_NULL_POINTER;
    if (hop_len == 0 || frame_len == 0) return VV_DSP_ERROR_INVALID_SIZE;
    const size_t frames = vv_dsp_get_num_frames(n, frame_len, hop_len, center);
    return (vv_dsp_status)vvhip_pitch_frames_device(d_signal, n, nch, ch_stride, frame_len, hop_len, frames, center,
                                                    d_window, (const vvhip_pitch_params*)params,
                                                    (const vvhip_pitch_out*)out, out_ch_stride, cmnd_ch_stride, stream);
}
