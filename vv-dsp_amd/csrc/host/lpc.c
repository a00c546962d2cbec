/* lpc.c -- linear prediction on the MI355X backend (C99).
 * Semantics and argument checks of the reference's src/envelope/lpc.c:7-72, in
 * its order; every sum, recursion and spectrum runs on the GPU (vvhip_autocorr_*,
 * _levinson_*, _lpc_*, _lpspec_*; lpc_kernels.hip).  The one host comparison is
 * vv_dsp_levinson's r[0] <= 0 on the caller's own value (lpc.c:25). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/envelope.h"
#include "vv_dsp/core/framing.h"
#include "vv_dsp_hip.h"

int vv_dsp_envelope_dummy(void) { return 5; }

vv_dsp_status vv_dsp_autocorr(const vv_dsp_real* x, size_t n, size_t order, vv_dsp_real* r_out) {
    if (!x || !r_out) return VV_DSP_ERROR_NULL_POINTER;
    if (order + 1 > n) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_autocorr_host(x, n, order, r_out);
}

vv_dsp_status vv_dsp_levinson(const vv_dsp_real* r, size_t order, vv_dsp_real* a_out, vv_dsp_real* err_out) {
    if (!r || !a_out || !err_out) return VV_DSP_ERROR_NULL_POINTER;
    if (r[0] <= 0) return VV_DSP_ERROR_INTERNAL;   /* a NaN passes, as in the reference */
    return (vv_dsp_status)vvhip_levinson_host(r, order, a_out, err_out);
}

vv_dsp_status vv_dsp_lpc(const vv_dsp_real* x, size_t n, size_t order, vv_dsp_real* a_out, vv_dsp_real* err_out) {
    if (!x || !a_out || !err_out) return VV_DSP_ERROR_NULL_POINTER;
    if (order + 1 > n) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_lpc_host(x, n, order, a_out, err_out);
}

vv_dsp_status vv_dsp_lpspec(const vv_dsp_real* a, size_t order, vv_dsp_real gain, size_t nfft, vv_dsp_real* mag_out) {
    if (!a || !mag_out) return VV_DSP_ERROR_NULL_POINTER;
    if (nfft == 0) return VV_DSP_OK;
    return (vv_dsp_status)vvhip_lpspec_host(a, order, gain, nfft, mag_out);
}

/* batched device rows (vv_dsp_amd.h) */
vv_dsp_status vv_dsp_autocorr_device(const vv_dsp_real* d_x, size_t n, size_t order, size_t batch, vv_dsp_real* d_r,
                                     void* stream) {
    if (!d_x || !d_r) return VV_DSP_ERROR_NULL_POINTER;
    if (order + 1 > n) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_autocorr_device(d_x, n, order, batch, d_r, stream);
}

vv_dsp_status vv_dsp_levinson_device(const vv_dsp_real* d_r, size_t order, size_t batch, vv_dsp_real* d_a,
                                     vv_dsp_real* d_err, void* stream) {
    if (!d_r || !d_a || !d_err) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_levinson_device(d_r, order, batch, d_a, d_err, NULL, stream);
}

vv_dsp_status vv_dsp_lpc_device(const vv_dsp_real* d_x, size_t n, size_t order, size_t batch, vv_dsp_real* d_a,
                                vv_dsp_real* d_err, void* stream) {
    if (!d_x || !d_a || !d_err) return VV_DSP_ERROR_NULL_POINTER;
    if (order + 1 > n) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_lpc_device(d_x, n, order, batch, d_a, d_err, NULL, stream);
}

vv_dsp_status vv_dsp_lpc_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                       size_t frame_len, size_t hop_len, int center, const vv_dsp_real* d_window,
                                       size_t order, vv_dsp_real* d_a, size_t a_ch_stride, vv_dsp_real* d_err,
                                       size_t err_ch_stride, void* stream) {
    if (!d_signal || !d_a || !d_err) return VV_DSP_ERROR_NULL_POINTER;
    if (hop_len == 0 || frame_len == 0 || order + 1 > frame_len) return VV_DSP_ERROR_INVALID_SIZE;
    const size_t frames = vv_dsp_get_num_frames(n, frame_len, hop_len, center);
    if (frames == 0) return VV_DSP_OK;
    return (vv_dsp_status)vvhip_lpc_frames_device(d_signal, n, nch, ch_stride, frame_len, hop_len, frames, center,
                                                  d_window, order, d_a, a_ch_stride, d_err, err_ch_stride, stream);
}

vv_dsp_status vv_dsp_lpspec_device(const vv_dsp_real* d_a, size_t order, const vv_dsp_real* d_gain, size_t nfft,
                                   size_t batch, int levinson_sign, vv_dsp_real* d_mag, void* stream) {
    if (!d_a || !d_mag) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_lpspec_device(d_a, order, d_gain, 1.0f, nfft, batch, levinson_sign, d_mag, stream);
}
