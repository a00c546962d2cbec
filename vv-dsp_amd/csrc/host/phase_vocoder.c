/* phase_vocoder.c -- the phase vocoder on the MI355X backend (C99).
 * include/vv_dsp/spectral/phase_vocoder.h defines every value and the order of
 * the argument checks (NULL pointers; n_fft < 2 or a channel stride shorter than
 * its rows; start, step and the last position of the uniform form; the kernel's
 * limits), all made before any device work, here and by the shim; every value
 * is computed on the GPU (vvhip_pvoc_*, vvhip_stft_stretch_*; pvoc_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/spectral/phase_vocoder.h"
#include "vv_dsp_hip.h"

/* stft.c: the handle's device side */
__attribute__((visibility("hidden"))) vvhip_stft* vv_amd_stft_device_handle(const vv_dsp_stft* h);

vv_dsp_status vv_dsp_phase_vocoder(const vv_dsp_cpx* spec, size_t T, size_t n_fft, double start, double step,
                                   size_t m, vv_dsp_cpx* out) {
    if (!spec || !out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pvoc_host((const float*)spec, T, n_fft, start, step, m, (float*)out);
}

vv_dsp_status vv_dsp_phase_vocoder_uniform_device(const vv_dsp_cpx* d_spec, size_t T, size_t n_fft, size_t nch,
                                                  size_t spec_ch_stride, double start, double step, size_t m,
                                                  vv_dsp_cpx* d_out, size_t out_ch_stride, void* stream) {
    if (!d_spec || !d_out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pvoc_device((const float*)d_spec, T, n_fft, nch, spec_ch_stride, NULL, start, step, m,
                                            (float*)d_out, out_ch_stride, stream);
}

vv_dsp_status vv_dsp_phase_vocoder_device(const vv_dsp_cpx* d_spec, size_t T, size_t n_fft, size_t nch,
                                          size_t spec_ch_stride, const vv_dsp_real* d_pos, size_t m, vv_dsp_cpx* d_out,
                                          size_t out_ch_stride, void* stream) {
    if (!d_spec || !d_pos || !d_out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_pvoc_device((const float*)d_spec, T, n_fft, nch, spec_ch_stride, d_pos, 0.0, 0.0, m,
                                            (float*)d_out, out_ch_stride, stream);
}

vv_dsp_status vv_dsp_stft_time_stretch_length(const vv_dsp_stft* h, size_t n, double rate, size_t* out_rows,
                                              size_t* out_len) {
    if (!h) return VV_DSP_ERROR_NULL_POINTER;
    size_t nfft = 0, hop = 0;
    vv_dsp_status st = vv_dsp_stft_get_sizes(h, &nfft, &hop);
    if (st != VV_DSP_OK) return st;
    return (vv_dsp_status)vvhip_stft_stretch_length(n, nfft, hop, rate, out_rows, out_len);
}

vv_dsp_status vv_dsp_stft_time_stretch_device(vv_dsp_stft* h, const vv_dsp_real* d_signal, size_t n, size_t nch,
                                              size_t ch_stride, double rate, vv_dsp_real* d_out, size_t out_ch_stride,
                                              void* stream, size_t* out_len) {
    if (!h || !d_signal || !d_out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_stft_stretch_device(vv_amd_stft_device_handle(h), d_signal, n, nch, ch_stride, rate,
                                                    d_out, out_ch_stride, stream, out_len);
}
