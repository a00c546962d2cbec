/* hpss.c -- harmonic-percussive separation on the MI355X backend (C99).
 * include/vv_dsp/spectral/hpss.h defines every value and the order of the
 * argument checks (NULL pointers; n_fft < 2 or a pitch below n_fft/2 + 1; the
 * windows, the mask and the margins; the kernels' limits), all made before any
 * device work, here and by the shim; every value is computed on the GPU
 * (vvhip_hpss_*, vvhip_stft_hpss_device; median_kernels.hip).
 * vv_dsp_hpss_params and _out have the layouts of vvhip_hpss_params and _out. */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/spectral/hpss.h"
#include "vv_dsp_hip.h"

/* stft.c: the handle's device side */
__attribute__((visibility("hidden"))) vvhip_stft* vv_amd_stft_device_handle(const vv_dsp_stft* h);

vv_dsp_status vv_dsp_hpss(const vv_dsp_real* power_rows, size_t rows, const vv_dsp_hpss_params* params,
                          const vv_dsp_hpss_out* out) {
    if (!params || !power_rows || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_hpss_host(power_rows, rows, (const vvhip_hpss_params*)params,
                                          (const vvhip_hpss_out*)out);
}

vv_dsp_status vv_dsp_hpss_device(const vv_dsp_real* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                                 const vv_dsp_hpss_params* params, const vv_dsp_hpss_out* out, size_t out_pitch,
                                 void* stream) {
    if (!params || !d_power || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_hpss_device(d_power, rows, row_pitch, rows_per_group,
                                            (const vvhip_hpss_params*)params, (const vvhip_hpss_out*)out, out_pitch,
                                            stream);
}

vv_dsp_status vv_dsp_stft_hpss_device(vv_dsp_stft* h, const vv_dsp_hpss_params* params, const vv_dsp_real* d_signal,
                                      size_t n, size_t nch, size_t ch_stride, vv_dsp_real* d_out_harm,
                                      vv_dsp_real* d_out_perc, size_t out_ch_stride, void* stream, size_t* out_len) {
    if (!h || !params || !d_signal || (!d_out_harm && !d_out_perc)) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_stft_hpss_device(vv_amd_stft_device_handle(h), (const vvhip_hpss_params*)params,
                                                 d_signal, n, nch, ch_stride, d_out_harm, d_out_perc, out_ch_stride,
                                                 stream, out_len);
}
