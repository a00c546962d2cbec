/* medfilt.c -- the running median on the MI355X backend (C99).
 * include/vv_dsp/filter/median.h defines the order, the boundary modes and the
 * order of the argument checks (NULL pointers; n == 0 or a stride below n; the
 * window and the mode; the kernel's limits), all made before any device work,
 * here and by the shim; every value is selected on the GPU (vvhip_medfilt_*;
 * median_kernels.hip). */
#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/filter/median.h"
#include "vv_dsp_hip.h"

vv_dsp_status vv_dsp_medfilt(const vv_dsp_real* x, size_t n, int window_length, vv_dsp_medfilt_mode mode,
                             vv_dsp_real* y) {
    if (!x || !y) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_medfilt_host(x, n, window_length, (int)mode, y);
}

vv_dsp_status vv_dsp_medfilt_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t x_stride,
                                    int window_length, vv_dsp_medfilt_mode mode, vv_dsp_real* d_y, size_t y_stride,
                                    void* stream) {
    if (!d_x || !d_y) return VV_DSP_ERROR_NULL_POINTER;
    return (vv_dsp_status)vvhip_medfilt_device(d_x, n, batch, x_stride, window_length, (int)mode, d_y, y_stride,
                                               stream);
}
