// shim_core.hip -- the extern "C" HIP shim (include/vv_dsp_hip.h): availability,
// version, the error text, device memory, streams and devices, half-row packing.
//
// The shim owns the device-side objects behind the C99 front-end and dispatches
// to the kernel launchers of the *_kernels.hip files; each module has its own
// translation unit (shim_fft, shim_stft, shim_fir, shim_resample,
// shim_analytic, shim_mel, shim_spectral) over shim_common.hpp.  There is no
// CPU compute path: every transform runs on the GPU, and every entry point
// reports UNSUPPORTED/INTERNAL when no device is present or a launch fails.
#include "shim_common.hpp"

using namespace vvh;

extern "C" {

int vvhip_available(void) { return device_count(); }

const char* vvhip_last_error(void) { return g_err.c_str(); }

const char* vvhip_version(void) { return "vvhip gfx950 (CDNA4) ROCm 7.2"; }

void* vvhip_malloc(size_t bytes) {
    void* p = nullptr;
    if (device_count() <= 0 || hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    return p;
}
void vvhip_free(void* p) {
    if (p) (void)hipFree(p);
}
int vvhip_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), ST_INTERNAL);
    return ST_OK;
}
int vvhip_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), ST_INTERNAL);
    return ST_OK;
}
// stream-ordered scratch (hipMallocAsync pool of the stream's device) and copies,
// for the C host code (dist.c); errors land in vvhip_last_error
int vvhip_malloc_async(void** p, size_t bytes, void* stream) {
    if (!p) return ST_NULL;
    *p = nullptr;
    HIPCHK(hipMallocAsync(p, bytes ? bytes : 16, (hipStream_t)stream), ST_INTERNAL);
    return ST_OK;
}
int vvhip_free_async(void* p, void* stream) {
    if (p) HIPCHK(hipFreeAsync(p, (hipStream_t)stream), ST_INTERNAL);
    return ST_OK;
}
int vvhip_memcpy_d2d_async(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0 || dst == src) return ST_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), ST_INTERNAL);
    return ST_OK;
}
// the device a stream belongs to (the null stream: the current device's)
int vvhip_stream_device(void* stream, int* device) {
    if (!device) return ST_NULL;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    HIPCHK(hipStreamGetDevice((hipStream_t)stream, device), ST_INTERNAL);
    return ST_OK;
}
// `waiter` waits (on the device) for the work enqueued on `producer` so far:
// an event recorded on the producer's device, waited on by the waiter; the
// event is released once it has completed (hipEventDestroy defers)
int vvhip_stream_wait(void* waiter, void* producer) {
    if (waiter == producer) return ST_OK;
    int prev = 0, pdev = 0;
    HIPCHK(hipGetDevice(&prev), ST_INTERNAL);
    HIPCHK(hipStreamGetDevice((hipStream_t)producer, &pdev), ST_INTERNAL);
    hipEvent_t ev = nullptr;
    hipError_t e = hipSetDevice(pdev);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, (hipStream_t)producer);
    (void)hipSetDevice(prev);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)waiter, ev, 0);
    if (ev) (void)hipEventDestroy(ev);
    HIPCHK(e, ST_INTERNAL);
    return ST_OK;
}
void vvhip_set_error(const char* what) { g_err = what ? what : ""; }

int vvhip_memset(void* dst, int value, size_t bytes) {
    HIPCHK(hipMemset(dst, value, bytes), ST_INTERNAL);
    return ST_OK;
}
int vvhip_stream_sync(void* stream) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream), ST_INTERNAL);
    return ST_OK;
}
int vvhip_device_sync(void) {
    HIPCHK(hipDeviceSynchronize(), ST_INTERNAL);
    return ST_OK;
}

int vvhip_set_device(int device) {
    const int nd = device_count();
    if (nd <= 0) return fail(ST_UNSUP, "no HIP device");
    if (device < 0 || device >= nd) return fail(ST_RANGE, "device index");
    HIPCHK(hipSetDevice(device), ST_INTERNAL);
    return ST_OK;
}

int vvhip_get_device(int* device) {
    if (!device) return ST_NULL;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    HIPCHK(hipGetDevice(device), ST_INTERNAL);
    return ST_OK;
}

int vvhip_rows_half_device(const float* d_in, float* d_out, size_t rows, size_t n, int unpack, void* stream) {
    if (!d_in || !d_out) return ST_NULL;
    if (n == 0) return ST_SIZE;
    {   // the kernel reads rows while writing others: any overlap of the byte ranges races
        const size_t h = n / 2 + 1, in_w = unpack ? h : n, out_w = unpack ? n : h;
        const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + sizeof(float) * rows * in_w;
        const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + sizeof(float) * rows * out_w;
        if (rows > 0 && a0 < b1 && b0 < a1) return fail(ST_RANGE, "half-row pack/unpack: in and out overlap");
    }
    HIPCHK(launch_rows_half(d_in, d_out, (long long)rows, (long long)n, unpack ? 1 : 0, (hipStream_t)stream),
           ST_INTERNAL);
    return ST_OK;
}

}  // extern "C"
