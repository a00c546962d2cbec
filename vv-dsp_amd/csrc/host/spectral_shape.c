/* spectral_shape.c -- per-frame spectral shape descriptors on the MI355X backend
 * (C99).  include/vv_dsp/features/spectral_shape.h defines every value and the
 * order of the argument checks (NULL pointers; n_fft < 2 or a row pitch below
 * n_fft/2 + 1; the band; sample_rate, floor and rolloff; the kernel's limit), all
 * made before any device work, here and by the shim; every sum and decision runs
 * on the GPU (vvhip_shape_*; shape_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/features/spectral_shape.h"
#include "vv_dsp_hip.h"

/* vv_dsp_spectral_shape_params / _out / _values and vvhip_shape_params / _out /
 * _values have the same members in the same order */
typedef char shape_params_same[sizeof(vv_dsp_spectral_shape_params) == sizeof(vvhip_shape_params) ? 1 : -1];
typedef char shape_out_same[sizeof(vv_dsp_spectral_shape_out) == sizeof(vvhip_shape_out) ? 1 : -1];
typedef char shape_values_same[sizeof(vv_dsp_spectral_shape_values) == sizeof(vvhip_shape_values) ? 1 : -1];

/* stft.c: the handle's device side and its fft_size */
__attribute__((visibility("hidden"))) vvhip_stft* vv_amd_stft_device_handle(const vv_dsp_stft* h);

vv_dsp_status vv_dsp_spectral_shape(const vv_dsp_real* power_row, const vv_dsp_real* prev_row_or_NULL,
                                    const vv_dsp_spectral_shape_params* params, vv_dsp_spectral_shape_values* out) {
    if (!params || !power_row || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_shape_host(power_row, prev_row_or_NULL, (const vvhip_shape_params*)params,
                                           (vvhip_shape_values*)out);
}

vv_dsp_status vv_dsp_spectral_shape_device(const vv_dsp_real* d_power, size_t rows, size_t row_pitch,
                                           size_t rows_per_group, const vv_dsp_spectral_shape_params* params,
                                           const vv_dsp_spectral_shape_out* out, void* stream) {
    if (!params || !d_power || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_shape_device(d_power, rows, row_pitch, rows_per_group,
                                             (const vvhip_shape_params*)params, (const vvhip_shape_out*)out, stream);
}

vv_dsp_status vv_dsp_stft_spectral_shape_device(vv_dsp_stft* h, const vv_dsp_spectral_shape_params* params,
                                                const vv_dsp_real* d_signal, size_t n, size_t nch, size_t ch_stride,
                                                const vv_dsp_spectral_shape_out* out, size_t out_ch_stride,
                                                void* stream, size_t* out_frames) {
    if (!h || !params || !d_signal || !out) return VV_DSP_ERROR_NULL_POINTER;
    size_t nfft = 0, hop = 0;
    vv_dsp_status st = vv_dsp_stft_get_sizes(h, &nfft, &hop);
    if (st != VV_DSP_OK) return st;
    if (out_frames) *out_frames = vvhip_stft_num_frames(n, nfft, hop);
    return (vv_dsp_status)vvhip_stft_shape_device(vv_amd_stft_device_handle(h), (const vvhip_shape_params*)params,
                                                  d_signal, n, nch, ch_stride, (const vvhip_shape_out*)out,
                                                  out_ch_stride, stream);
}
