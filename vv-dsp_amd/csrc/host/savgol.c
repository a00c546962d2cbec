/* savgol.c -- Savitzky-Golay on the MI355X backend (C99).
 * Argument checks of the reference's src/filter/savgol.c:219-262 in its order.
 * The window's coefficients are one-time host setup in f64 with the reference's
 * operations in its order (savgol.c:28-162: the normal matrix, Gauss-Jordan
 * with partial pivoting, one solve per sample and the sum-to-one step for
 * smoothing, one solve and the delta scaling for derivatives), so the float
 * coefficients are bit-identical to its; this file is compiled with
 * -ffp-contract=off.  Padding and convolution run on the GPU (vvhip_savgol_*;
 * savgol_kernels.hip).
 *
 * One difference in order: the reference applies the NaN policy to the input
 * before it rejects window_length > 257 or polyorder > 15, so under the ERROR
 * policy a NaN in the input wins over those two; here every check that needs
 * no data comes first. */
#include <math.h>

#include "vv_dsp/vv_dsp_amd.h"
#include "vv_dsp/filter/savgol.h"
#include "vv_dsp/core/nan_policy.h"
#include "vv_dsp_hip.h"

enum { SG_MAX_WINDOW = 257, SG_MAX_COLS = 16 };

/* A^T A of the m x cols Vandermonde matrix on t = -half .. half, row by row */
static void sg_normal_matrix(int m, int cols, double* ata) {
    const int half = m / 2;
    for (int i = 0; i < cols * cols; ++i) ata[i] = 0.0;
    for (int row = 0; row < m; ++row) {
        double pw[SG_MAX_COLS];
        pw[0] = 1.0;
        for (int j = 1; j < cols; ++j) pw[j] = pw[j - 1] * (double)(row - half);
        for (int i = 0; i < cols; ++i)
            for (int j = 0; j < cols; ++j) ata[i * cols + j] += pw[i] * pw[j];
    }
}

/* ata x = rhs by Gauss-Jordan elimination with partial pivoting on the augmented
 * matrix; 0, or -1 for a zero pivot */
static int sg_solve(const double* ata, const double* rhs, int cols, double* x) {
    double aug[SG_MAX_COLS * (SG_MAX_COLS + 1)];
    const int w = cols + 1;
    for (int i = 0; i < cols; ++i) {
        for (int j = 0; j < cols; ++j) aug[i * w + j] = ata[i * cols + j];
        aug[i * w + cols] = rhs[i];
    }
    for (int k = 0; k < cols; ++k) {
        int piv = k;
        double best = fabs(aug[k * w + k]);
        for (int r = k + 1; r < cols; ++r) {
            const double v = fabs(aug[r * w + k]);
            if (v > best) {
                piv = r;
                best = v;
            }
        }
        if (best == 0.0) return -1;
        if (piv != k) {
            for (int j = k; j <= cols; ++j) {
                const double t = aug[k * w + j];
                aug[k * w + j] = aug[piv * w + j];
                aug[piv * w + j] = t;
            }
        }
        const double diag = aug[k * w + k];
        for (int j = k; j <= cols; ++j) aug[k * w + j] /= diag;
        for (int r = 0; r < cols; ++r) {
            if (r == k) continue;
            const double f = aug[r * w + k];
            for (int j = k; j <= cols; ++j) aug[r * w + j] -= f * aug[k * w + j];
        }
    }
    for (int i = 0; i < cols; ++i) x[i] = aug[i * w + cols];
    return 0;
}

/* deriv == 0: h[r] = the constant term of the fit to a unit sample at r, then
 * the row is scaled to sum 1 */
static vv_dsp_status sg_smoothing(int m, int cols, const double* ata, vv_dsp_real* h) {
    const int half = m / 2;
    for (int r = 0; r < m; ++r) {
        double col[SG_MAX_COLS], sol[SG_MAX_COLS];
        col[0] = 1.0;
        for (int j = 1; j < cols; ++j) col[j] = col[j - 1] * (double)(r - half);
        if (sg_solve(ata, col, cols, sol) != 0) return VV_DSP_ERROR_INTERNAL;
        h[r] = (vv_dsp_real)sol[0];
    }
    double sum = 0.0;
    for (int r = 0; r < m; ++r) sum += (double)h[r];
    if (sum != 0.0) {
        const double inv = 1.0 / sum;
        for (int r = 0; r < m; ++r) h[r] = (vv_dsp_real)((double)h[r] * inv);
    }
    return VV_DSP_OK;
}

/* deriv > 0: c solves ata c = deriv! e_deriv, h[r] = sum_j c[j] t^j, over delta^deriv */
static vv_dsp_status sg_derivative(int m, int cols, const double* ata, int deriv, vv_dsp_real delta, vv_dsp_real* h) {
    const int half = m / 2;
    double rhs[SG_MAX_COLS], c[SG_MAX_COLS];
    double fact = 1.0;
    for (int i = 1; i <= deriv; ++i) fact *= (double)i;
    for (int i = 0; i < cols; ++i) rhs[i] = 0.0;
    rhs[deriv] = fact;
    if (sg_solve(ata, rhs, cols, c) != 0) return VV_DSP_ERROR_INTERNAL;
    for (int r = 0; r < m; ++r) {
        double tp = 1.0, acc = 0.0;
        for (int j = 0; j < cols; ++j) {
            if (j > 0) tp *= (double)(r - half);
            acc += c[j] * tp;
        }
        h[r] = (vv_dsp_real)acc;
    }
    const double scale = pow((double)delta, (double)deriv);
    if (scale == 0.0) return VV_DSP_ERROR_OUT_OF_RANGE;
    const double inv = 1.0 / scale;
    for (int r = 0; r < m; ++r) h[r] = (vv_dsp_real)((double)h[r] * inv);
    return VV_DSP_OK;
}

/* savgol.c:230-235 without the data-dependent window_length > N */
static vv_dsp_status sg_check_shape(int window_length, int polyorder, int deriv) {
    if (window_length <= 0 || (window_length & 1) == 0) return VV_DSP_ERROR_OUT_OF_RANGE;
    if (polyorder < 0 || deriv < 0 || deriv > polyorder) return VV_DSP_ERROR_OUT_OF_RANGE;
    return VV_DSP_OK;
}

/* savgol.c:252-258 and the kernels' own limits (:39, :147) */
static vv_dsp_status sg_design(int m, int polyorder, int deriv, vv_dsp_real delta, vv_dsp_real* h) {
    if (m > SG_MAX_WINDOW) return VV_DSP_ERROR_OUT_OF_RANGE;
    const int cols = polyorder + 1;
    if (cols > SG_MAX_COLS) return VV_DSP_ERROR_OUT_OF_RANGE;
    double ata[SG_MAX_COLS * SG_MAX_COLS];
    sg_normal_matrix(m, cols, ata);
    return deriv == 0 ? sg_smoothing(m, cols, ata, h) : sg_derivative(m, cols, ata, deriv, delta, h);
}

vv_dsp_status vv_dsp_savgol_coeffs(int window_length, int polyorder, int deriv, vv_dsp_real delta, vv_dsp_real* h) {
    if (!h) return VV_DSP_ERROR_NULL_POINTER;
    vv_dsp_status st = sg_check_shape(window_length, polyorder, deriv);
    if (st != VV_DSP_OK) return st;
    if (deriv > 0 && !(delta > (vv_dsp_real)0)) return VV_DSP_ERROR_OUT_OF_RANGE;
    return sg_design(window_length, polyorder, deriv, delta, h);
}

/* the checks and the design shared by the host and the device entry */
static vv_dsp_status sg_prepare(size_t n, int window_length, int polyorder, int deriv, vv_dsp_real delta,
                                vv_dsp_real* h) {
    if (n == 0) return VV_DSP_ERROR_INVALID_SIZE;
    vv_dsp_status st = sg_check_shape(window_length, polyorder, deriv);
    if (st != VV_DSP_OK) return st;
    if ((size_t)window_length > n) return VV_DSP_ERROR_INVALID_SIZE;
    if (deriv > 0 && !(delta > (vv_dsp_real)0)) return VV_DSP_ERROR_OUT_OF_RANGE;
    return sg_design(window_length, polyorder, deriv, delta, h);
}

vv_dsp_status vv_dsp_savgol(const vv_dsp_real* y, size_t N, int window_length, int polyorder, int deriv,
                            vv_dsp_real delta, vv_dsp_savgol_mode mode, vv_dsp_real* output) {
    if (!y || !output) return VV_DSP_ERROR_NULL_POINTER;
    vv_dsp_real h[SG_MAX_WINDOW];
    const vv_dsp_status st = sg_prepare(N, window_length, polyorder, deriv, delta, h);
    if (st != VV_DSP_OK) return st;
    return (vv_dsp_status)vvhip_savgol_host(y, N, h, window_length, (int)mode, (int)vv_dsp_get_nan_policy(), output);
}

vv_dsp_status vv_dsp_savgol_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t x_stride, int window_length,
                                   int polyorder, int deriv, vv_dsp_real delta, vv_dsp_savgol_mode mode,
                                   vv_dsp_real* d_y, size_t y_stride, void* stream) {
    if (!d_x || !d_y) return VV_DSP_ERROR_NULL_POINTER;
    vv_dsp_real h[SG_MAX_WINDOW];
    const vv_dsp_status st = sg_prepare(n, window_length, polyorder, deriv, delta, h);
    if (st != VV_DSP_OK) return st;
    return (vv_dsp_status)vvhip_savgol_device(d_x, n, batch, x_stride, h, window_length, (int)mode,
                                              (int)vv_dsp_get_nan_policy(), d_y, y_stride, stream);
}
