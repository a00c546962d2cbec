// shim_resample.hip -- the rational resampler's entry points over
// resample_kernels.hip (the plan and its table live in csrc/host/resampler.c).
#include "shim_common.hpp"

#include <cstring>

using namespace vvh;

static unsigned resample_gcd(unsigned a, unsigned b) {
    while (b) {
        const unsigned t = a % b;
        a = b;
        b = t;
    }
    return a;
}

extern "C" {

size_t vvhip_resample_run_length(unsigned num, unsigned den, unsigned taps) {
    if (num == 0 || den == 0) return 0;
    if (taps < 4) taps = 4;
    if (taps & 1) taps += 1;
    const unsigned g = resample_gcd(num, den);
    return (size_t)resample_run((long long)(num / g) + 1, (int)taps, (double)num / (double)den);
}

// the packed host table [phases][taps] -> a device table with rows
// resample_row_stride(taps) floats apart (the pad floats 0), as the kernel reads it
int vvhip_resample_table_upload(const float* table, size_t phases, unsigned taps, float** d_table) {
    if (!table || !d_table) return ST_NULL;
    *d_table = nullptr;
    if (phases == 0 || taps == 0) return ST_SIZE;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    const size_t S = (size_t)resample_row_stride((int)taps);
    std::vector<float> padded(phases * S, 0.0f);
    for (size_t r = 0; r < phases; ++r) std::memcpy(&padded[r * S], table + r * taps, sizeof(float) * taps);
    float* d = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(float) * padded.size()), ST_INTERNAL);
    hipError_t e = hipMemcpy(d, padded.data(), sizeof(float) * padded.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(ST_INTERNAL, "resampler table upload", e);
    }
    *d_table = d;
    return ST_OK;
}

int vvhip_resample_linear_device(const float* d_in, size_t in_n, size_t nch, size_t in_stride, float* d_out,
                                 size_t out_n, size_t out_stride, double ratio, void* stream) {
    if (!d_in || !d_out) return ST_NULL;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (in_n == 0 || out_n == 0 || nch == 0) return ST_OK;
    if (in_n >= ((size_t)1 << 31) || !(ratio > 0.0)) return fail(ST_SIZE, "resampler: in_n >= 2^31 or a bad ratio");
    HIPCHK(launch_resample_linear(d_in, (long long)in_n, (long long)nch, (long long)in_stride, d_out, (long long)out_n,
                                  (long long)out_stride, ratio, (hipStream_t)stream),
           ST_INTERNAL);
    return ST_OK;
}

int vvhip_resample_sinc_device(const float* d_in, size_t in_n, size_t nch, size_t in_stride, float* d_out,
                               size_t out_n, size_t out_stride, double ratio, double cutoff, unsigned taps,
                               const float* d_table, size_t phases, void* stream) {
    if (!d_in || !d_out) return ST_NULL;
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    if (in_n == 0 || out_n == 0 || nch == 0) return ST_OK;
    if (in_n >= ((size_t)1 << 31) || !(ratio > 0.0)) return fail(ST_SIZE, "resampler: in_n >= 2^31 or a bad ratio");
    if (taps < 4 || taps > 128 || (taps & 1)) return fail(ST_SIZE, "resampler: taps must be even, 4..128");
    hipStream_t s = (hipStream_t)stream;
    if (d_table && knob(KNOB_RESAMPLE_GENERIC, 0) != 1) {
        if (resample_run((long long)phases, (int)taps, ratio) == 0)
            return fail(ST_SIZE, "resampler: this table does not fit the table kernel");
        HIPCHK(launch_resample_table(d_in, (long long)in_n, (long long)nch, (long long)in_stride, d_out,
                                     (long long)out_n, (long long)out_stride, ratio, cutoff, (long long)phases,
                                     (int)taps, d_table, s),
               ST_INTERNAL);
        stat_inc(STAT_RESAMPLE_TABLE);
        return ST_OK;
    }
    HIPCHK(launch_resample_generic(d_in, (long long)in_n, (long long)nch, (long long)in_stride, d_out, (long long)out_n,
                                   (long long)out_stride, ratio, cutoff, (int)taps, s),
           ST_INTERNAL);
    stat_inc(STAT_RESAMPLE_GENERIC);
    return ST_OK;
}

}  // extern "C"
