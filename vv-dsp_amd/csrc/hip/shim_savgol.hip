// shim_savgol.hip -- Savitzky-Golay rows (src/filter/savgol.c:164-217): the
// entry points over savgol_kernels.hip.  The window's coefficients are designed
// on the host (csrc/host/savgol.c) and arrive here in host memory.
#include "shim_common.hpp"

using namespace vvh;

extern "C" {

int vvhip_savgol_device(const float* d_x, size_t n, size_t batch, size_t x_stride, const float* h, int m, int mode,
                        int nan_policy, float* d_y, size_t y_stride, void* stream) {
    if (!d_x || !d_y || !h) return ST_NULL;
    if (n == 0) return ST_SIZE;
    if (m <= 0 || m % 2 == 0) return ST_RANGE;
    if ((size_t)m > n) return ST_SIZE;
    if (m > SAVGOL_MAX_WINDOW) return ST_RANGE;
    if (mode < 0 || mode > 3) return fail(ST_RANGE, "savgol: mode is not one of vv_dsp_savgol_mode");
    if (nan_policy < 0 || nan_policy > 3) nan_policy = 0;   // nan_policy.c:79-81: unknown is PROPAGATE
    if (n >= ((size_t)1 << 31) || batch >= ((size_t)1 << 31)) return fail(ST_SIZE, "savgol: n or batch >= 2^31");
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (batch == 0) return ST_OK;
    hipStream_t s = (hipStream_t)stream;
    // rows that overlap the output are staged: a workgroup reads its neighbours' spans
    Scratch copy(s), flag(s);
    const float* x_end = d_x + (batch - 1) * x_stride + n;
    const float* y_end = d_y + (batch - 1) * y_stride + n;
    if (d_x < y_end && d_y < x_end) {
        HIPCHK(copy.alloc(sizeof(float) * n * batch), ST_INTERNAL);
        HIPCHK(hipMemcpy2DAsync(copy.p, sizeof(float) * n, d_x, sizeof(float) * x_stride, sizeof(float) * n, batch,
                                hipMemcpyDeviceToDevice, s),
               ST_INTERNAL);
        d_x = (const float*)copy.p;
        x_stride = n;
    }
    int* dflag = nullptr;
    if (nan_policy == 2) {
        HIPCHK(flag.alloc(sizeof(int)), ST_INTERNAL);
        dflag = (int*)flag.p;
        HIPCHK(hipMemsetAsync(dflag, 0, sizeof(int), s), ST_INTERNAL);
    }
    HIPCHK(launch_savgol(d_x, (long long)n, (long long)batch, (long long)x_stride, h, m, mode, nan_policy, d_y,
                         (long long)y_stride, dflag, s),
           ST_INTERNAL);
    if (nan_policy == 2) {
        int hflag = 0;
        HIPCHK(hipMemcpyAsync(&hflag, dflag, sizeof(int), hipMemcpyDeviceToHost, s), ST_INTERNAL);
        HIPCHK(hipStreamSynchronize(s), ST_INTERNAL);
        if (hflag) return ST_NAN;
    }
    return ST_OK;
}

int vvhip_savgol_host(const float* x, size_t n, const float* h, int m, int mode, int nan_policy, float* y) {
    if (!x || !y || !h) return ST_NULL;
    if (n == 0) return ST_SIZE;
    HostCall c("savgol");
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    float* dy = (float*)c.out(y, sizeof(float) * n);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_savgol_device(dx, n, 1, n, h, m, mode, nan_policy, dy, n, c.s));
}

}  // extern "C"
