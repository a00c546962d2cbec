/* lsf.c -- line spectral frequencies and reflection coefficients of LPC rows on
 * the MI355X backend (C99).  include/vv_dsp/envelope/lsf.h defines the values
 * and the order of the argument checks, all made before any device work; the
 * recursion, the scan and the bisection run on the GPU (vvhip_lpc_to_lsf_*,
 * vvhip_lsf_*; lsf_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/envelope/lsf.h"
#include "vv_dsp/core/framing.h"
#include "vv_dsp_hip.h"

vv_dsp_status vv_dsp_lpc_to_lsf(const vv_dsp_real* a, size_t order, vv_dsp_real* lsf_out, vv_dsp_real* rc_out,
                                int32_t* flags_out) {
    if (!a || (!lsf_out && !rc_out && !flags_out)) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_to_lsf_host(a, order, lsf_out, rc_out, flags_out);
}

vv_dsp_status vv_dsp_lsf_to_lpc(const vv_dsp_real* lsf, size_t order, vv_dsp_real* a_out) {
    if (!lsf || !a_out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lsf_to_lpc_host(lsf, order, a_out);
}

vv_dsp_status vv_dsp_lpc_to_lsf_device(const vv_dsp_real* d_a, size_t order, size_t batch, size_t a_pitch,
                                       vv_dsp_real* d_lsf, vv_dsp_real* d_rc, int32_t* d_flags, void* stream) {
    if (!d_a || (!d_lsf && !d_rc && !d_flags)) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpc_to_lsf_device(d_a, order, batch, a_pitch, d_lsf, d_rc, d_flags, stream);
}

vv_dsp_status vv_dsp_lsf_to_lpc_device(const vv_dsp_real* d_lsf, size_t order, size_t batch, vv_dsp_real* d_a,
                                       size_t a_pitch, void* stream) {
    if (!d_lsf || !d_a) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lsf_to_lpc_device(d_lsf, order, batch, d_a, a_pitch, stream);
}

vv_dsp_status vv_dsp_lsf_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                       size_t frame_len, size_t hop_len, int center, const vv_dsp_real* d_window,
                                       size_t order, vv_dsp_real* d_lsf, vv_dsp_real* d_rc, int32_t* d_flags,
                                       vv_dsp_real* d_err, void* stream) {
    if (!d_signal || (!d_lsf && !d_rc && !d_flags && !d_err)) return VV_DSP_ERROR_NULL_POINTER;
    if (hop_len == 0 || frame_len == 0 || order < 1 || order + 1 > frame_len) return VV_DSP_ERROR_INVALID_SIZE;
    const size_t frames = vv_dsp_get_num_frames(n, frame_len, hop_len, center);
    return (vv_dsp_status)vvhip_lsf_frames_device(d_signal, n, nch, ch_stride, frame_len, hop_len, frames, center,
                                                  d_window, order, d_lsf, d_rc, d_flags, d_err, stream);
}
