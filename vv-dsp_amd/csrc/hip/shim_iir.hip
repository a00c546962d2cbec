// shim_iir.hip -- biquad cascades (src/filter/iir.c:21-43): the entry points
// over iir_kernels.hip.
//
// Route rule, a function of n alone (never of the batch, the strides or the
// entry point, so a row's output is the same wherever it is computed): rows of
// n <= IIR_EXACT_MAX run as one recurrence per row, bit-identical to the
// reference; longer rows are cut into chunks of IIR_CHUNK_LEN samples and take
// the three launches of iir_kernels.hip.  Knob IIR_CHUNK: 0 never chunks, k > 0
// forces chunks of k samples; a chunk length >= n is the exact route.
// STAT_IIR_EXACT / STAT_IIR_CHUNKED count the calls of either route.
//
// Cascades longer than IIR_MAX_STAGES run as successive groups of stages, the
// later groups in place on the output rows.  The reference rounds to float
// between stages too, so the split changes no bit.
#include "shim_common.hpp"

using namespace vvh;

// chunk length of rows of n samples; 0: one recurrence per row
static long long iir_chunk_len(size_t n) {
    const long long k = knob(KNOB_IIR_CHUNK, -1);
    const long long L = k >= 0 ? k : ((long long)n <= IIR_EXACT_MAX ? 0 : IIR_CHUNK_LEN);
    return L >= (long long)n ? 0 : L;
}

extern "C" {

int vvhip_iir_device(const float* d_coef, size_t stages, float* d_state, const float* d_x, float* d_y, size_t n,
                     size_t batch, size_t x_stride, size_t y_stride, void* stream) {
    if (!d_x || !d_y || (!d_coef && stages > 0)) return ST_NULL;
    if (n == 0 || batch == 0) return ST_OK;
    if (n >= ((size_t)1 << 31) - 64 || batch >= ((size_t)1 << 31) || stages >= ((size_t)1 << 24))
        return fail(ST_SIZE, "iir: n or batch >= 2^31, or stages >= 2^24");
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    hipStream_t s = (hipStream_t)stream;
    if (stages == 0) {
        if (d_y != d_x)
            HIPCHK(hipMemcpy2DAsync(d_y, sizeof(float) * y_stride, d_x, sizeof(float) * x_stride, sizeof(float) * n,
                                    batch, hipMemcpyDeviceToDevice, s),
                   ST_INTERNAL);
        return ST_OK;
    }
    const long long L = iir_chunk_len(n);
    const long long chunks = L ? ((long long)n + L - 1) / L : 1;
    if (chunks * (long long)batch >= (1LL << 37)) return fail(ST_SIZE, "iir: too many chunks for one call");
    Scratch zs(s), zin(s), phi(s);
    if (L) {
        const size_t states = (size_t)chunks * batch * 2 * IIR_MAX_STAGES;
        HIPCHK(zs.alloc(sizeof(float) * states), ST_INTERNAL);
        HIPCHK(zin.alloc(sizeof(float) * states), ST_INTERNAL);
        HIPCHK(phi.alloc(sizeof(double) * 4 * IIR_MAX_STAGES * IIR_MAX_STAGES), ST_INTERNAL);
    }
    for (size_t g0 = 0; g0 < stages; g0 += IIR_MAX_STAGES) {
        const int sg = (int)(stages - g0 < (size_t)IIR_MAX_STAGES ? stages - g0 : (size_t)IIR_MAX_STAGES);
        float* state = d_state ? d_state + 2 * g0 : nullptr;
        IirWalk w;
        w.x = g0 == 0 ? d_x : d_y;
        w.x_stride = (long long)(g0 == 0 ? x_stride : y_stride);
        w.y = d_y;
        w.y_stride = (long long)y_stride;
        w.n = (long long)n;
        w.rows = (long long)batch;
        w.coef = d_coef + 5 * g0;
        if (!L) {
            w.L = (long long)n;
            w.zin = w.zout = state;
            w.zin_stride = w.zout_stride = (long long)(2 * stages);
            HIPCHK(launch_iir_walk(w, sg, 1, s), ST_INTERNAL);
            continue;
        }
        const long long D = 2 * sg;
        w.L = L;
        w.chunks = chunks;
        HIPCHK(launch_iir_phi(w.coef, sg, L, (double*)phi.p, s), ST_INTERNAL);
        w.zout = (float*)zs.p;
        w.zout_stride = D;
        HIPCHK(launch_iir_walk(w, sg, 0, s), ST_INTERNAL);
        HIPCHK(launch_iir_scan((const double*)phi.p, sg, (const float*)zs.p, state, (long long)(2 * stages),
                               (long long)batch, chunks, (float*)zin.p, s),
               ST_INTERNAL);
        w.zin = (const float*)zin.p;
        w.zin_stride = D;
        w.zout = state;
        w.zout_stride = (long long)(2 * stages);
        HIPCHK(launch_iir_walk(w, sg, 1, s), ST_INTERNAL);
    }
    stat_inc(L ? STAT_IIR_CHUNKED : STAT_IIR_EXACT);
    return ST_OK;
}

int vvhip_iir_host(const float* coef, size_t stages, float* state, const float* x, float* y, size_t n) {
    if (!x || !y || ((!coef || !state) && stages > 0)) return ST_NULL;
    if (n == 0) return ST_OK;
    HostCall c("iir");
    const float* dc = (const float*)c.in(stages ? coef : nullptr, sizeof(float) * 5 * stages);
    float* dz = stages ? (float*)c.inout(state, sizeof(float) * 2 * stages) : nullptr;
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    float* dy = (float*)c.out(y, sizeof(float) * n);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_iir_device(dc, stages, dz, dx, dy, n, 1, n, n, c.s));
}

}  // extern "C"
