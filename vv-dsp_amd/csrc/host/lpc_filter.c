/* lpc_filter.c -- the LPC residual and synthesis filters on the MI355X backend
 * (C99).  include/vv_dsp/envelope/lpc_filter.h defines the values and the order
 * of the argument checks, all made before any device work; the filters run on
 * the GPU (vvhip_lpc_residual_*, vvhip_lpc_synth_*; lpc_filter_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/envelope/lpc_filter.h"
#include "vv_dsp/core/framing.h"
#include "vv_dsp_hip.h"

vv_dsp_status vv_dsp_lpc_residual(const vv_dsp_real* x, size_t n, const vv_dsp_real* a, size_t order, size_t frames,
                                  size_t seg_len, long long offset, const vv_dsp_real* gain, double* state,
                                  vv_dsp_real* e) {
    if (!x || !a || !e) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_residual_host(x, n, a, order, frames, seg_len, offset, gain, state, e);
}

vv_dsp_status vv_dsp_lpc_synth(const vv_dsp_real* e, size_t n, const vv_dsp_real* a, size_t order, size_t frames,
                               size_t seg_len, long long offset, const vv_dsp_real* gain, double* state,
                               vv_dsp_real* y) {
    if (!e || !a || !y) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_synth_host(e, n, a, order, frames, seg_len, offset, gain, state, y);
}

vv_dsp_status vv_dsp_lpc_residual_device(const vv_dsp_real* d_x, size_t n, size_t nch, size_t x_stride,
                                         const vv_dsp_real* d_a, size_t order, size_t frames, size_t a_pitch,
                                         size_t a_ch_stride, const vv_dsp_real* d_gain, size_t g_ch_stride,
                                         size_t seg_len, long long offset, double* d_state, vv_dsp_real* d_e,
                                         size_t e_stride, void* stream) {
    if (!d_x || !d_a || !d_e) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_residual_device(d_x, n, nch, x_stride, d_a, order, frames, a_pitch, a_ch_stride,
                                                    d_gain, g_ch_stride, seg_len, offset, d_state, d_e, e_stride,
                                                    stream);
}

vv_dsp_status vv_dsp_lpc_synth_device(const vv_dsp_real* d_e, size_t n, size_t nch, size_t e_stride,
                                      const vv_dsp_real* d_a, size_t order, size_t frames, size_t a_pitch,
                                      size_t a_ch_stride, const vv_dsp_real* d_gain, size_t g_ch_stride,
                                      size_t seg_len, long long offset, double* d_state, vv_dsp_real* d_y,
                                      size_t y_stride, void* stream) {
    if (!d_e || !d_a || !d_y) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_synth_device(d_e, n, nch, e_stride, d_a, order, frames, a_pitch, a_ch_stride,
                                                 d_gain, g_ch_stride, seg_len, offset, d_state, d_y, y_stride, stream);
}

vv_dsp_status vv_dsp_lpc_residual_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                                size_t frame_len, size_t hop_len, int center,
                                                const vv_dsp_real* d_window, size_t order, vv_dsp_real* d_a,
                                                size_t a_ch_stride, vv_dsp_real* d_err, size_t err_ch_stride,
                                                vv_dsp_real* d_e, size_t e_stride, void* stream) {
    if (!d_signal || !d_e) return VV_DSP_ERROR_NULL_POINTER;
    if (hop_len == 0 || frame_len == 0 || order < 1 || order + 1 > frame_len) return VV_DSP_ERROR_INVALID_SIZE;
    const size_t frames = vv_dsp_get_num_frames(n, frame_len, hop_len, center);
    return (vv_dsp_status)vvhip_lpc_residual_frames_device(d_signal, n, nch, ch_stride, frame_len, hop_len, frames,
                                                           center, d_window, order, d_a, a_ch_stride, d_err,
                                                           err_ch_stride, d_e, e_stride, stream);
}
