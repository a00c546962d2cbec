/* resampler.c -- fixed-ratio resampler on the MI355X backend (C99).
 *
 * The plan keeps the reference's state (src/resample/resampler.c:7-52: ratio,
 * quality, cutoff) plus the ratio reduced by its gcd and a lazily built device
 * table.  Processing runs on the GPU (csrc/hip/resample_kernels.hip):
 *   linear (:77-86)  -> bit-identical to vv_dsp_interpolate_linear_real per output;
 *   sinc   (:88-119) -> the polyphase table kernel, or the per-output f64 kernel
 *                       when the table of the reduced ratio does not fit in LDS.
 *
 * The table.  The ratio is rational, so in_pos = k / ratio has only P = num / gcd
 * distinct fractional parts p / P, and the reference's weights
 *   sinc_fn(t * cutoff) * hann(m, taps),  t = (m - taps/2) - frac
 * depend on frac and the tap number m alone (the Hann window is indexed by the
 * tap, not by t).  Row p < P holds them for frac = p / P, row P for frac = 1:
 * where k den / num is an integer, the reference's f64 quotient (double)k / ratio
 * can land one ulp below it; it then centres one sample lower with frac ~ 1,
 * which is a different filter from frac = 0 one sample higher.  The sinc is
 * rounded to f32 before the product (sinc_fn returns vv_dsp_real); window,
 * product, sum and the division by the sum are f64, rounded to f32 once. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/resample/resampler.h"
#include "vv_dsp_hip.h"

static const double kPiD = 3.141592653589793238462643383279502884;

struct vv_dsp_resampler {
    unsigned int ratio_num, ratio_den; /* as given */
    unsigned int num_r, den_r;         /* reduced by the gcd: the same ratio and cutoff doubles */
    int use_sinc;
    unsigned int taps;
    double cutoff;
    /* device table of (num_r, den_r, table_taps) on device table_dev; NULL: not built */
    float* d_table;
    size_t phases;
    unsigned int table_taps;
    int table_dev;
};

static unsigned int gcd_u(unsigned int a, unsigned int b) {
    while (b) {
        const unsigned int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

static unsigned int effective_taps(unsigned int taps) { /* resampler.c:89-91 after the 4..128 clamp of :48-49 */
    if (taps < 4) taps = 4;
    if (taps > 128) taps = 128;
    if (taps % 2 == 1) taps += 1;
    return taps;
}

static vv_dsp_real sinc_fn(double x) { /* resampler.c:54-58 */
    if (x == 0.0) return (vv_dsp_real)1.0;
    const double pix = kPiD * x;
    return (vv_dsp_real)(sin(pix) / pix);
}

static double hann_window(unsigned int m, unsigned int N) { /* resampler.c:60-63 */
    if (N <= 1) return 1.0;
    return 0.5 - 0.5 * cos((2.0 * kPiD * (double)m) / (double)(N - 1));
}

int vvhip_resample_table_host(unsigned num, unsigned den, unsigned taps, float* out, size_t* phases,
                              unsigned* taps_eff) {
    if (!phases || !taps_eff) return VV_DSP_ERROR_NULL_POINTER;
    if (num == 0 || den == 0) return VV_DSP_ERROR_OUT_OF_RANGE;
    taps = effective_taps(taps);
    const unsigned int P = num / gcd_u(num, den);
    *phases = (size_t)P + 1;
    *taps_eff = taps;
    if (!out) return VV_DSP_OK;
    const double cutoff = fmin(1.0, (double)num / (double)den);
    const int half = (int)(taps / 2);
    double weight[128];
    for (size_t p = 0; p <= P; ++p) {
        const double frac = p == P ? 1.0 : (double)p / (double)P;
        double wsum = 0.0;
        for (unsigned int m = 0; m < taps; ++m) {
            const double t = (double)((int)m - half) - frac;
            weight[m] = (double)sinc_fn(t * cutoff) * hann_window(m, taps);
            wsum += weight[m];
        }
        for (unsigned int m = 0; m < taps; ++m)
            out[p * taps + m] = (float)(wsum != 0.0 ? weight[m] / wsum : weight[m]);
    }
    return VV_DSP_OK;
}

static void set_ratio(vv_dsp_resampler* rs, unsigned int num, unsigned int den) {
    const unsigned int g = gcd_u(num, den);
    rs->ratio_num = num;
    rs->ratio_den = den;
    rs->num_r = num / g;
    rs->den_r = den / g;
    rs->cutoff = fmin(1.0, (double)num / (double)den);
}

static void drop_table(vv_dsp_resampler* rs) {
    if (rs->d_table) vvhip_free(rs->d_table);
    rs->d_table = NULL;
    rs->phases = 0;
}

vv_dsp_resampler* vv_dsp_resampler_create(unsigned int ratio_num, unsigned int ratio_den) {
    if (ratio_num == 0 || ratio_den == 0) return NULL;
    vv_dsp_resampler* rs = (vv_dsp_resampler*)calloc(1, sizeof(*rs));
    if (!rs) return NULL;
    set_ratio(rs, ratio_num, ratio_den);
    rs->use_sinc = 0;
    rs->taps = 32;
    return rs;
}

void vv_dsp_resampler_destroy(vv_dsp_resampler* rs) {
    if (!rs) return;
    drop_table(rs);
    free(rs);
}

int vv_dsp_resampler_set_ratio(vv_dsp_resampler* rs, unsigned int ratio_num, unsigned int ratio_den) {
    if (!rs) return VV_DSP_ERROR_NULL_POINTER;
    if (ratio_num == 0 || ratio_den == 0) return VV_DSP_ERROR_OUT_OF_RANGE;
    const unsigned int pn = rs->num_r, pd = rs->den_r;
    set_ratio(rs, ratio_num, ratio_den);
    if (rs->num_r != pn || rs->den_r != pd) drop_table(rs);
    return VV_DSP_OK;
}

int vv_dsp_resampler_set_quality(vv_dsp_resampler* rs, int use_sinc, unsigned int taps) {
    if (!rs) return VV_DSP_ERROR_NULL_POINTER;
    rs->use_sinc = use_sinc ? 1 : 0;
    if (taps < 4) taps = 4;
    if (taps > 128) taps = 128;
    rs->taps = taps; /* the table is keyed by the effective taps: rebuilt at the next call if they changed */
    return VV_DSP_OK;
}

size_t vv_dsp_resampler_output_length(const vv_dsp_resampler* rs, size_t in_n) {
    if (!rs || in_n == 0) return 0;
    const double ratio = (double)rs->ratio_num / (double)rs->ratio_den;
    return (size_t)floor((in_n - 1) * ratio) + 1; /* resampler.c:72-73 */
}

/* the device table for (reduced ratio, taps) on the stream's device */
static int ensure_table(vv_dsp_resampler* rs, unsigned int taps, void* stream) {
    int dev = 0;
    int st = vvhip_stream_device(stream, &dev);
    if (st != VV_DSP_OK) return st;
    if (rs->d_table && rs->table_taps == taps && rs->table_dev == dev) return VV_DSP_OK;
    drop_table(rs);
    size_t phases = 0;
    unsigned int te = 0;
    st = vvhip_resample_table_host(rs->num_r, rs->den_r, taps, NULL, &phases, &te);
    if (st != VV_DSP_OK) return st;
    float* host = (float*)malloc(phases * te * sizeof(float));
    if (!host) return VV_DSP_ERROR_INTERNAL;
    st = vvhip_resample_table_host(rs->num_r, rs->den_r, taps, host, &phases, &te);
    int prev = 0;
    if (st == VV_DSP_OK) st = vvhip_get_device(&prev);
    if (st == VV_DSP_OK && prev != dev) st = vvhip_set_device(dev);
    if (st == VV_DSP_OK) {
        st = vvhip_resample_table_upload(host, phases, te, &rs->d_table);
        if (prev != dev) (void)vvhip_set_device(prev);
    }
    free(host);
    if (st != VV_DSP_OK) return st;
    rs->phases = phases;
    rs->table_taps = te;
    rs->table_dev = dev;
    return VV_DSP_OK;
}

vv_dsp_status vv_dsp_resampler_process_device(vv_dsp_resampler* rs, const vv_dsp_real* d_in, size_t in_n, size_t nch,
                                              size_t in_stride, vv_dsp_real* d_out, size_t out_cap,
                                              size_t out_stride, void* stream, size_t* out_n) {
    if (!rs || !d_in || !d_out) return VV_DSP_ERROR_NULL_POINTER;
    if (in_n == 0) {
        if (out_n) *out_n = 0;
        return VV_DSP_OK;
    }
    const size_t expect = vv_dsp_resampler_output_length(rs, in_n);
    if (expect > out_cap) return VV_DSP_ERROR_INVALID_SIZE;
    if (in_n >= ((size_t)1 << 31)) return VV_DSP_ERROR_INVALID_SIZE; /* the reference's centre index is an int */
    if (out_n) *out_n = expect;
    const double ratio = (double)rs->ratio_num / (double)rs->ratio_den;
    if (!rs->use_sinc)
        return (vv_dsp_status)vvhip_resample_linear_device(d_in, in_n, nch, in_stride, d_out, expect, out_stride,
                                                           ratio, stream);
    const unsigned int taps = effective_taps(rs->taps);
    const float* table = NULL;
    if (vvhip_resample_run_length(rs->num_r, rs->den_r, taps) != 0) { /* routing: the table fits the table kernel */
        int st = ensure_table(rs, taps, stream);
        if (st != VV_DSP_OK) return (vv_dsp_status)st;
        table = rs->d_table;
    }
    return (vv_dsp_status)vvhip_resample_sinc_device(d_in, in_n, nch, in_stride, d_out, expect, out_stride, ratio,
                                                     rs->cutoff, taps, table, rs->phases, stream);
}

int vv_dsp_resampler_process_real(vv_dsp_resampler* rs, const vv_dsp_real* in, size_t in_n, vv_dsp_real* out,
                                  size_t out_cap, size_t* out_n) {
    if (!rs || !in || !out || !out_n) return VV_DSP_ERROR_NULL_POINTER;
    if (in_n == 0) {
        *out_n = 0;
        return VV_DSP_OK;
    }
    const size_t expect = vv_dsp_resampler_output_length(rs, in_n);
    if (expect > out_cap) return VV_DSP_ERROR_INVALID_SIZE;
    if (in_n >= ((size_t)1 << 31)) return VV_DSP_ERROR_INVALID_SIZE;
    *out_n = expect;
    if (vvhip_available() <= 0) { /* no CPU compute path */
        vvhip_set_error("no HIP device");
        return VV_DSP_ERROR_UNSUPPORTED;
    }
    float* d_in = (float*)vvhip_malloc(in_n * sizeof(float));
    float* d_out = (float*)vvhip_malloc(expect * sizeof(float));
    int st = (d_in && d_out) ? VV_DSP_OK : VV_DSP_ERROR_INTERNAL;
    if (st == VV_DSP_OK) st = vvhip_memcpy_h2d(d_in, in, in_n * sizeof(float));
    if (st == VV_DSP_OK)
        st = vv_dsp_resampler_process_device(rs, d_in, in_n, 1, in_n, d_out, expect, expect, NULL, NULL);
    if (st == VV_DSP_OK) st = vvhip_stream_sync(NULL);
    if (st == VV_DSP_OK) st = vvhip_memcpy_d2h(out, d_out, expect * sizeof(float));
    vvhip_free(d_in);
    vvhip_free(d_out);
    return st;
}
