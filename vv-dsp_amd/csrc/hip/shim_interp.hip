// shim_interp.hip -- interpolation at arbitrary positions (src/resample/interpolate.c:4-64):
// the entry points over interp_kernels.hip.  Every check is made before any
// device work, in this order: null pointers; n == 0 (the reference's order); m == 0
// or batch == 0 (OK, nothing written); a non-zero stride shorter than its row, or
// an output stride of 0 with more than one row; an unknown method; n >= 2^31.
#include "shim_common.hpp"

using namespace vvh;

// the checks of both device forms; ST_OK with *empty set: nothing to do
static int interp_check(const void* d_x, size_t n, size_t batch, size_t x_stride, size_t m, size_t pos_stride, int method,
                        const void* d_out, size_t out_stride, bool* empty) {
    *empty = false;
    if (!d_x || !d_out) return ST_NULL;
    if (n == 0) return ST_SIZE;
    if (m == 0 || batch == 0) {
        *empty = true;
        return ST_OK;
    }
    if ((x_stride != 0 && x_stride < n) || (pos_stride != 0 && pos_stride < m) || (out_stride != 0 && out_stride < m) ||
        (out_stride == 0 && batch > 1))
        return fail(ST_SIZE, "interpolate: a stride shorter than its row");
    if (method != INTERP_LINEAR && method != INTERP_CUBIC) return fail(ST_RANGE, "interpolate: unknown method");
    if (n >= ((size_t)1 << 31) || m >= ((size_t)1 << 40) || batch >= ((size_t)1 << 31))
        return fail(ST_SIZE, "interpolate: n >= 2^31, m >= 2^40 or batch >= 2^31");
    return ST_OK;
}

// Signal rows one workgroup takes its run of positions through.  Where one
// position array serves every row, a workgroup takes INTERP_SHARED_ROWS rows: the
// positions are read once for them, and what a position decides (clamps, floor,
// fraction, weights) serves them all -- measured faster than one row per workgroup
// (DESIGN.md section 4).  Knob INTERP_ROWS = 1 forces one row; the bits are the
// same.  Computed (uniform) positions measured no faster that way and always take
// one row.
static int interp_rows(const InterpArgs& a) {
    if (!a.pos || a.pos_stride != 0 || a.batch < 2) return 1;
    return knob(KNOB_INTERP_ROWS, 0) == 1 ? 1 : INTERP_SHARED_ROWS;
}

static int interp_run(const InterpArgs& a, int method, hipStream_t s) {
    if (device_count() <= 0) return fail(ST_UNSUP, "no HIP device");
    const int rows = interp_rows(a);
    HIPCHK(launch_interp(a, method, rows, s), ST_INTERNAL);
    stat_inc(rows > 1 ? STAT_INTERP_ROWS : STAT_INTERP_ONE);
    return ST_OK;
}

extern "C" {

size_t vvhip_interp_run_length(void) { return (size_t)INTERP_RUN; }

int vvhip_interp_device(const float* d_x, size_t n, size_t batch, size_t x_stride, const float* d_pos, size_t m,
                        size_t pos_stride, int method, float* d_out, size_t out_stride, void* stream) {
    if (!d_pos) return ST_NULL;
    bool empty;
    const int st = interp_check(d_x, n, batch, x_stride, m, pos_stride, method, d_out, out_stride, &empty);
    if (st != ST_OK || empty) return st;
    InterpArgs a;
    a.x = d_x;
    a.n = (long long)n;
    a.batch = (long long)batch;
    a.x_stride = (long long)x_stride;
    a.pos = d_pos;
    a.m = (long long)m;
    a.pos_stride = (long long)pos_stride;
    a.out = d_out;
    a.out_stride = (long long)out_stride;
    return interp_run(a, method, (hipStream_t)stream);
}

int vvhip_interp_uniform_device(const float* d_x, size_t n, size_t batch, size_t x_stride, double start, double step,
                                size_t m, int method, float* d_out, size_t out_stride, void* stream) {
    bool empty;
    const int st = interp_check(d_x, n, batch, x_stride, m, 0, method, d_out, out_stride, &empty);
    if (st != ST_OK || empty) return st;
    InterpArgs a;
    a.x = d_x;
    a.n = (long long)n;
    a.batch = (long long)batch;
    a.x_stride = (long long)x_stride;
    a.m = (long long)m;
    a.start = start;
    a.step = step;
    a.out = d_out;
    a.out_stride = (long long)out_stride;
    return interp_run(a, method, (hipStream_t)stream);
}

// One row and m positions in host memory, staged once.
int vvhip_interp_host(const float* x, size_t n, const float* pos, size_t m, int method, float* out) {
    if (!pos) return ST_NULL;
    bool empty;
    const int st = interp_check(x, n, 1, n, m, 0, method, out, m, &empty);
    if (st != ST_OK || empty) return st;
    HostCall c("interpolate");
    const float* dx = (const float*)c.in(x, sizeof(float) * n);
    const float* dp = (const float*)c.in(pos, sizeof(float) * m);
    float* dout = (float*)c.out(out, sizeof(float) * m);
    if (!c.ok()) return c.st;
    return c.finish(vvhip_interp_device(dx, n, 1, n, dp, m, 0, method, dout, m, c.s));
}

}  // extern "C"
