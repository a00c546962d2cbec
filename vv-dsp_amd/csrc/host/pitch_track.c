/* pitch_track.c -- f0 tracking over the YIN curves on the MI355X backend (C99).
 * include/vv_dsp/features/pitch_track.h defines the path and the order of the
 * argument checks, all made before any device work by the shim; the forward
 * pass and the backtrace run on the GPU (vvhip_pitch_track_*;
 * pitch_track_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/features/pitch_track.h"
#include "vv_dsp/core/framing.h"
#include "vv_dsp_hip.h"

/* vv_dsp_pitch_track_params / _out and vvhip_pitch_track_params / _out have the
 * same members in the same order */
vv_dsp_status vv_dsp_pitch_track_params_default(const vv_dsp_pitch_params* pitch, size_t frame_len,
                                                vv_dsp_pitch_track_params* track) {
    if (!pitch || !track) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pitch_track_params_default((const vvhip_pitch_params*)pitch, frame_len,
                                                           (vvhip_pitch_track_params*)track);
}

vv_dsp_status vv_dsp_pitch_track(const vv_dsp_real* curves, size_t frames, size_t row_stride,
                                 const vv_dsp_pitch_track_params* params, const vv_dsp_pitch_track_out* out) {
    if (!curves || !params || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pitch_track_host(curves, frames, row_stride, (const vvhip_pitch_track_params*)params,
                                                 (const vvhip_pitch_track_out*)out);
}

vv_dsp_status vv_dsp_pitch_track_device(const vv_dsp_real* d_curves, size_t frames, size_t nch, size_t row_stride,
                                        size_t cmnd_ch_stride, const vv_dsp_pitch_track_params* params,
                                        const vv_dsp_pitch_track_out* out, size_t out_ch_stride, void* stream) {
    if (!d_curves || !params || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pitch_track_device(d_curves, frames, nch, row_stride, cmnd_ch_stride,
                                                   (const vvhip_pitch_track_params*)params,
                                                   (const vvhip_pitch_track_out*)out, out_ch_stride, stream);
}

vv_dsp_status vv_dsp_pitch_track_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                               size_t frame_len, size_t hop_len, int center,
                                               const vv_dsp_real* d_window, const vv_dsp_pitch_params* pitch,
                                               const vv_dsp_pitch_track_params* track,
                                               const vv_dsp_pitch_track_out* out, size_t out_ch_stride, void* stream) {
    if (!d_signal || !pitch || !track || !out) return VV_DSP_ERROR_NULL_POINTER;
    if (hop_len == 0 || frame_len == 0) return VV_DSP_ERROR_INVALID_SIZE;
    const size_t frames = vv_dsp_get_num_frames(n, frame_len, hop_len, center);
    return (vv_dsp_status)vvhip_pitch_track_frames_device(d_signal, n, nch, ch_stride, frame_len, hop_len, frames,
                                                          center, d_window, (const vvhip_pitch_params*)pitch,
                                                          (const vvhip_pitch_track_params*)track,
                                                          (const vvhip_pitch_track_out*)out, out_ch_stride, stream);
}
