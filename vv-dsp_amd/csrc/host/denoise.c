/* denoise.c -- spectral noise suppression on the MI355X backend (C99).
 * include/vv_dsp/spectral/denoise.h defines every value and the order of the
 * argument checks (NULL pointers; n_fft < 2 or a pitch below n_fft/2 + 1; the
 * lengths, the mode, the bias and the floor; the kernel's limits), all made
 * before any device work, here and by the shim; every value is computed on the
 * GPU (vvhip_denoise_*, vvhip_stft_denoise_device; denoise_kernels.hip).
 * vv_dsp_denoise_params and _out have the layouts of vvhip_denoise_params and _out. */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/spectral/denoise.h"
#include "vv_dsp_hip.h"

/* stft.c: the handle's device side */
__attribute__((visibility("hidden"))) vvhip_stft* vv_amd_stft_device_handle(const vv_dsp_stft* h);

vv_dsp_status vv_dsp_denoise_params_default(size_t n_fft, vv_dsp_denoise_params* params) {
    if (!params) return VV_DSP_ERROR_NULL_POINTER;
    params->n_fft = n_fft;
    params->smooth_len = 8;
    params->back = 48;
    params->ahead = 48;
    params->bias = 4.0f;
    params->floor = 0.1f;
    params->mode = VV_DSP_DENOISE_WIENER;
    return VV_DSP_OK;
}

vv_dsp_status vv_dsp_denoise(const vv_dsp_real* power_rows, size_t rows, const vv_dsp_denoise_params* params,
                             const vv_dsp_denoise_out* out) {
    if (!params || !power_rows || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_denoise_host(power_rows, rows, (const vvhip_denoise_params*)params,
                                             (const vvhip_denoise_out*)out);
}

vv_dsp_status vv_dsp_denoise_device(const vv_dsp_real* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                                    const vv_dsp_denoise_params* params, const vv_dsp_denoise_out* out,
                                    size_t out_pitch, void* stream) {
    if (!params || !d_power || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_denoise_device(d_power, rows, row_pitch, rows_per_group,
                                               (const vvhip_denoise_params*)params, (const vvhip_denoise_out*)out,
                                               out_pitch, stream);
}

vv_dsp_status vv_dsp_stft_denoise_device(vv_dsp_stft* h, const vv_dsp_denoise_params* params,
                                         const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                         vv_dsp_real* d_out, size_t out_ch_stride, void* stream, size_t* out_len) {
    if (!h || !params || !d_signal || !d_out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_stft_denoise_device(vv_amd_stft_device_handle(h), (const vvhip_denoise_params*)params,
                                                    d_signal, n, nch, ch_stride, d_out, out_ch_stride, stream,
                                                    out_len);
}
