/* interpolate.c -- interpolation at fractional positions on the MI355X backend (C99).
 * Semantics and argument checks of the reference's src/resample/interpolate.c:4-64
 * and src/resample/resample.c, in its order: NULL pointers, then n == 0.  Every
 * value runs on the GPU (vvhip_interp_*; interp_kernels.hip) -- the two
 * single-position functions too, one staged launch per value: they exist for
 * source compatibility, the batched forms of vv_dsp_amd.h are the product. */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/resample.h"
#include "vv_dsp_hip.h"

int vv_dsp_resample_dummy(void) { return 3; }

vv_dsp_status vv_dsp_interpolate_real_batch(const vv_dsp_real* x, size_t n, const vv_dsp_real* pos, size_t m,
                                            vv_dsp_interp_method method, vv_dsp_real* out) {
    if (!x || !pos || !out) return VV_DSP_ERROR_NULL_POINTER;
    if (n == 0) return VV_DSP_ERROR_INVALID_SIZE;
    return (vv_dsp_status)vvhip_interp_host(x, n, pos, m, (int)method, out);
}

vv_dsp_status vv_dsp_interpolate_linear_real(const vv_dsp_real* x, size_t n, vv_dsp_real pos, vv_dsp_real* out) {
    if (!x || !out) return VV_DSP_ERROR_NULL_POINTER;
    return vv_dsp_interpolate_real_batch(x, n, &pos, 1, VV_DSP_INTERP_LINEAR, out);
}

vv_dsp_status vv_dsp_interpolate_cubic_real(const vv_dsp_real* x, size_t n, vv_dsp_real pos, vv_dsp_real* out) {
    if (!x || !out) return VV_DSP_ERROR_NULL_POINTER;
    return vv_dsp_interpolate_real_batch(x, n, &pos, 1, VV_DSP_INTERP_CUBIC, out);
}

vv_dsp_status vv_dsp_interpolate_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t x_stride,
                                        const vv_dsp_real* d_pos, size_t m, size_t pos_stride,
                                        vv_dsp_interp_method method, vv_dsp_real* d_out, size_t out_stride,
                                        void* stream) {
    if (!d_x || !d_pos || !d_out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_interp_device(d_x, n, batch, x_stride, d_pos, m, pos_stride, (int)method, d_out,
                                              out_stride, stream);
}

vv_dsp_status vv_dsp_interpolate_uniform_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t x_stride,
                                                double start, double step, size_t m, vv_dsp_interp_method method,
                                                vv_dsp_real* d_out, size_t out_stride, void* stream) {
    if (!d_x || !d_out) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_interp_uniform_device(d_x, n, batch, x_stride, start, step, m, (int)method, d_out,
                                                      out_stride, stream);
}
