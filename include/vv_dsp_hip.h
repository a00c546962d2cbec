/*
 * vv_dsp_hip.h -- the thin extern "C" HIP shim of the MI355X (gfx950) backend.
 *
 * Plain C ABI: opaque handles, raw pointers, sizes, int status codes with the
 * values of the reference's vv_dsp_status (include/vv_dsp/vv_dsp_types.h:120-128:
 * 0 OK, 1 NULL_POINTER, 2 INVALID_SIZE, 3 OUT_OF_RANGE, 4 INTERNAL,
 * 5 NAN_INF, 6 UNSUPPORTED).  No HIP or torch types appear here: streams are
 * passed as `void*` (a hipStream_t; NULL = the handle's own stream).
 *
 * Two calling conventions per operation:
 *   *_host   : host pointers, synchronous (what the reference's C API needs);
 *   *_device : device pointers, asynchronous on the given stream (the batched
 *              entry points; inputs already resident in HBM).
 *
 * The C99 front-end in vv-dsp_amd/csrc/host/ (the reference's vv_dsp_* API) is
 * the only intended caller of the *_host functions; the *_device functions are
 * also reachable through include/vv_dsp/vv_dsp_amd.h.
 *
 * Reference interfaces each group replaces:
 *   vvhip_fft_*  : the FFT backend vtable slot, src/spectral/fft_backend.h:32-38
 *                  (make_plan / execute / free_plan / is_available)
 *   vvhip_stft_* : src/spectral/stft.c:30-144 (create, process, reconstruct, spectrogram)
 *   vvhip_fir_*  : src/filter/fir.c:75-196 (apply_fft, apply), filter/common.c:23-80 (filtfilt)
 *   vvhip_hilbert_*: src/spectral/hilbert.c:14-75
 *   vvhip_dct_*  : src/spectral/dct.c:86-136
 *   vvhip_czt_*  : src/spectral/czt.c:44-178 (exec_cpx, exec_real)
 *   vvhip_fftshift_* / _phase_wrap_* / _phase_unwrap_*: src/spectral/utils.c:5-73
 *   vvhip_cepstrum_* / _icepstrum_minphase_* / _minphase_from_cepstrum_*:
 *                  src/envelope/cepstrum.c:7-78, src/envelope/minphase.c:7-31
 *   vvhip_autocorr_* / _levinson_* / _lpc_* / _lpspec_*: src/envelope/lpc.c:7-72
 *   vvhip_iir_*  : src/filter/iir.c:21-43;  vvhip_savgol_*: src/filter/savgol.c:164-217
 *   vvhip_stats_* / _autocorrelation_* / _cross_correlation_*: src/core/core.c:42-108,
 *                  src/core/stats.c:10-139
 *   vvhip_pitch_*: no reference source; include/vv_dsp/features/pitch.h defines it
 *   vvhip_shape_* / _stft_shape_*: no reference source;
 *                  include/vv_dsp/features/spectral_shape.h defines them
 *   vvhip_pvoc_* / _stft_stretch_*: no reference source;
 *                  include/vv_dsp/spectral/phase_vocoder.h defines them
 *   vvhip_medfilt_* / _hpss_* / _stft_hpss_*: no reference source;
 *                  include/vv_dsp/filter/median.h and spectral/hpss.h define them
 *   vvhip_denoise_* / _stft_denoise_*: no reference source;
 *                  include/vv_dsp/spectral/denoise.h defines them
 */
#ifndef VV_DSP_HIP_H
#define VV_DSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct vvhip_fft vvhip_fft;
typedef struct vvhip_stft vvhip_stft;
typedef struct vvhip_fir vvhip_fir;
typedef struct vvhip_mel vvhip_mel;
typedef struct vvhip_czt vvhip_czt;

/* Number of usable HIP devices (0 when none: every other call then fails). */
int vvhip_available(void);
/* Text of the last error seen by this thread ("" if none). */
const char* vvhip_last_error(void);

/* A/B switches and path counters (csrc/hip/debug.hip), for tests and the
 * scripts/kbench.py timing harness; the defaults are the adopted kernels.
 *   vvhip_debug_set("STFT_DYN", 0)  selects a launcher alternative (the names
 *       are the VVHIP_* switches of DESIGN.md, with or without the prefix);
 *       0 on success, -1 for an unknown name or a negative value;
 *   vvhip_debug_clear(name)  back to the default (NULL: every knob, and every
 *       path counter to 0);
 *   vvhip_debug_get(name)  a knob's value (-1 unset) or a path counter
 *       ("STAT_STFT_DYN", "STAT_FIR_DYN", "STAT_FIR_STATIC", "STAT_MEL_FUSED",
 *       "STAT_MEL_SPLIT", "STAT_RESAMPLE_TABLE", "STAT_RESAMPLE_GENERIC",
 *       "STAT_LPC_WAVE", "STAT_LPC_GENERIC", "STAT_IIR_EXACT",
 *       "STAT_IIR_CHUNKED", "STAT_STATS_WAVE", "STAT_STATS_LONG",
 *       "STAT_INTERP_ONE", "STAT_INTERP_ROWS", "STAT_PITCH_WAVE",
 *       "STAT_PVOC_ROWS", "STAT_PITCH_TRACK": launches of that path since the
 *       last clear);
 *       -2 unknown.
 * The environment is read once per process, and only with VVHIP_AB=1 set. */
int vvhip_debug_set(const char* name, long long value);
int vvhip_debug_clear(const char* name);
long long vvhip_debug_get(const char* name);
/* Build identification, e.g. "vvhip gfx950 ROCm 7.2". */
const char* vvhip_version(void);

/* ---- device memory helpers (tests / host front-end) ---- */
void* vvhip_malloc(size_t bytes);
void vvhip_free(void* p);
int vvhip_memcpy_h2d(void* dst, const void* src, size_t bytes);
int vvhip_memcpy_d2h(void* dst, const void* src, size_t bytes);
int vvhip_memset(void* dst, int value, size_t bytes);
/* stream-ordered scratch on the stream's device (hipMallocAsync / hipFreeAsync)
 * and a device-to-device copy on a stream */
int vvhip_malloc_async(void** p, size_t bytes, void* stream);
int vvhip_free_async(void* p, void* stream);
int vvhip_memcpy_d2d_async(void* dst, const void* src, size_t bytes, void* stream);
/* the device of a stream (NULL: the current device's null stream), and a
 * device-side wait of `waiter` for everything enqueued on `producer` so far
 * (an event on the producer's device; no host synchronisation) */
int vvhip_stream_device(void* stream, int* device);
int vvhip_stream_wait(void* waiter, void* producer);
/* sets the text vvhip_last_error() returns on this thread (host front-end errors) */
void vvhip_set_error(const char* what);
int vvhip_stream_sync(void* stream);
int vvhip_device_sync(void);
/* the calling thread's current HIP device (hipSetDevice / hipGetDevice) */
int vvhip_set_device(int device);
int vvhip_get_device(int* device);

/* ---- FFT: replaces the backend vtable slot (fft_backend.h:32-38) ----
 * type: 0 C2C, 1 R2C, 2 C2R (fft.h:152-156); dir: +1 forward, -1 backward.
 * Layout per transform as fft.h:169-172; `batch` transforms back to back. */
int vvhip_fft_plan_create(size_t n, int type, int dir, size_t batch, vvhip_fft** out);
int vvhip_fft_exec_host(vvhip_fft* plan, const void* in, void* out);
int vvhip_fft_exec_device(vvhip_fft* plan, const void* d_in, void* d_out, size_t batch,
                          void* stream);
void vvhip_fft_plan_destroy(vvhip_fft* plan);

/* ---- STFT (stft.c) ---- window: nfft floats computed by the caller. */
int vvhip_stft_create(size_t nfft, size_t hop, const float* window, vvhip_stft** out);
void vvhip_stft_destroy(vvhip_stft* h);
/* frames = n < nfft ? 1 : 1 + (n - nfft + hop) / hop   (stft.c:119) */
size_t vvhip_stft_num_frames(size_t n, size_t nfft, size_t hop);
int vvhip_stft_spectrogram_host(vvhip_stft* h, const float* signal, size_t n, float* out_mag);
/* nch channels at ch_stride floats; rows [ch][frame][...] at out_ch_stride elements.
 * out_kind 0: magnitudes sqrtf(re^2+im^2) of all nfft bins (stft.c:133-139);
 *          1: the full complex spectrum (float pairs, stft_process semantics);
 *          2: power re^2+im^2 of bins 0..nfft/2 (nfft/2+1 floats per row; the
 *             power spectrogram vv_dsp_compute_log_mel_spectrogram consumes). */
int vvhip_stft_spectrogram_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch,
                                  size_t ch_stride, void* d_out, size_t out_ch_stride,
                                  int out_kind, void* stream);
/* Power rows (kind 2) with rows row_pitch >= nfft/2+1 floats apart (the pad
 * floats are not written); out_ch_stride >= frames * row_pitch. */
int vvhip_stft_power_pitched_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch, size_t ch_stride,
                                    float* d_out, size_t out_ch_stride, size_t row_pitch, void* stream);
/* Frames [frame0, frame0 + nframes) of the same spectrogram (the row of frame
 * f is out + (f - frame0) * row): one shard of a long signal's frames.  With an
 * even frame0 the rows are bit-identical to the whole-signal call (frames are
 * transformed in pairs (2j, 2j+1)).  ST_RANGE if the range exceeds the frames. */
int vvhip_stft_spectrogram_range_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch,
                                        size_t ch_stride, size_t frame0, size_t nframes, void* d_out,
                                        size_t out_ch_stride, int out_kind, void* stream);
/* Half-spectrum rows for the config-5 gather: pack [rows][n] -> [rows][n/2+1]
 * (unpack 0), or expand [rows][n/2+1] -> [rows][n] by out[k] = in[n-k] above
 * n/2 (unpack 1; magnitude rows of real frames are mirror-symmetric). */
int vvhip_rows_half_device(const float* d_in, float* d_out, size_t rows, size_t n, int unpack, void* stream);
int vvhip_stft_process_host(vvhip_stft* h, const float* frame, float* spec_out);
int vvhip_stft_process_device(vvhip_stft* h, const float* d_frames, size_t count, float* d_spec,
                              void* stream);
int vvhip_stft_reconstruct_host(vvhip_stft* h, const float* spec, float* out_add, float* norm_add);
/* count frames (cpx[count][nfft]) overlap-added at `hop` into out_add/norm_add
 * (length (count-1)*hop + nfft); norm_add may be NULL. */
int vvhip_stft_reconstruct_device(vvhip_stft* h, const float* d_spec, size_t count, size_t hop,
                                  float* d_out_add, float* d_norm_add, void* stream);

/* ---- framing (src/core/framing.c:58-146) ----
 * Device: frames [frame0, frame0 + count) of an n-sample signal into
 * d_frames[count][frame_len] (zero padding, or reflection when center != 0;
 * times d_window when not NULL), and the overlap-add of count frames into
 * d_out[out_len] at (frame0 + f) * hop, each output sample summed in frame
 * order.  Host: one frame, the reference's signatures (via the device). */
int vvhip_fetch_frames_device(const float* d_signal, size_t n, float* d_frames, size_t frame_len, size_t hop,
                              size_t frame0, size_t count, int center, const float* d_window, void* stream);
int vvhip_overlap_add_device(const float* d_frames, size_t count, float* d_out, size_t out_len, size_t frame_len,
                             size_t hop, size_t frame0, void* stream);
int vvhip_fetch_frame_host(const float* signal, size_t n, float* frame, size_t frame_len, size_t hop,
                           size_t frame_index, int center, const float* window);
int vvhip_overlap_add_host(const float* frame, float* out, size_t out_len, size_t frame_len, size_t hop,
                           size_t frame_index);

/* ---- FIR (fir.c) ---- */
int vvhip_fir_create(const float* h, size_t taps, vvhip_fir** out);
void vvhip_fir_destroy(vvhip_fir* f);
/* mode 0: FFT overlap-save (fir_apply_fft semantics), mode 1: direct form,
 * same summation order as fir.c:170-186 (bit-identical to vv_dsp_fir_apply).
 * prefix: taps-1 samples preceding x[0] in time order (oldest first), or NULL
 * for zero initial state. */
int vvhip_fir_apply_host(vvhip_fir* f, const float* x, float* y, size_t n, const float* prefix,
                         int mode);
int vvhip_fir_apply_device(vvhip_fir* f, const float* d_x, float* d_y, size_t n, size_t nch,
                           size_t x_stride, size_t y_stride, const float* d_prefix, int mode,
                           void* stream);
/* ---- Mel / MFCC (src/features/mel.c:204-309) ----
 * fb: dense filterbank [n_mels][nbins] (vv_dsp_mel_filterbank_create), or NULL
 * for a plan that only maps log-mel rows to MFCC (kind 2).  n_coeffs: MFCC
 * coefficients (0 = log-mel only); lifter as mel.c:298-304; eps added before log. */
int vvhip_mel_create(const float* fb, size_t n_mels, size_t nbins, size_t n_coeffs, float lifter, float eps,
                     vvhip_mel** out);
void vvhip_mel_destroy(vvhip_mel* m);
/* kind 0: power rows [frames][nbins] -> log-mel [frames][n_mels]
 *      1: power rows -> MFCC [frames][n_coeffs]
 *      2: log-mel rows [frames][n_mels] -> MFCC [frames][n_coeffs] */
int vvhip_mel_device(vvhip_mel* m, const float* d_in, size_t frames, float* d_out, int kind, void* stream);
/* the same with power rows row_pitch >= nbins floats apart (kinds 0 / 1; 0 = nbins) */
int vvhip_mel_pitched_device(vvhip_mel* m, const float* d_in, size_t frames, size_t row_pitch, float* d_out, int kind,
                             void* stream);
/* signal [ch][n] (ch_stride floats apart) -> log-mel (kind 0) or MFCC (kind 1)
 * rows [ch][frame][n_mels | n_coeffs]: the stft's power rows feed the mel plan
 * in one kernel when nfft = 1024 (else two launches, same values) */
int vvhip_stft_mel_device(vvhip_stft* h, vvhip_mel* m, const float* d_signal, size_t n, size_t nch, size_t ch_stride,
                          float* d_out, size_t out_ch_stride, int kind, void* stream);
int vvhip_mel_host(vvhip_mel* m, const float* in, size_t frames, float* out, int kind);

/* Block length (real FFT size) the overlap-save path uses for a signal of n samples. */
/* zero-phase filtering (filter/common.c:23-80): reflection pad, direct form
 * forward and backward in the reference's summation order (bit-identical) */
int vvhip_fir_filtfilt_device(vvhip_fir* f, const float* d_x, float* d_y, size_t n, size_t nch, size_t x_stride,
                              size_t y_stride, void* stream);
int vvhip_fir_filtfilt_host(vvhip_fir* f, const float* x, float* y, size_t n);
size_t vvhip_fir_block_size(vvhip_fir* f, size_t n);

/* ---- Rational resampler (src/resample/resampler.c:65-119) ----
 * ratio = (double)num / (double)den and cutoff = fmin(1, ratio) as the reference
 * forms them.  Rows of in_n samples in_stride floats apart -> rows of out_n
 * samples out_stride floats apart, one launch; no alignment required.
 *
 * vvhip_resample_table_host (csrc/host/resampler.c; host arithmetic, no device):
 * the polyphase table of num/den reduced by their gcd, P = num / gcd.  Row p < P:
 * the reference's weights sinc_fn(t * cutoff) * hann(m, taps) at t = (m - taps/2) - p/P
 * (sinc rounded to f32 first, Hann indexed by the tap), divided by the row's sum,
 * all in f64, rounded to f32 once; row P: the same at fractional position 1
 * (where the reference's f64 quotient falls one ulp below an integer; the table
 * kernel evaluates those few outputs with the reference's own f64 loop, since
 * with 4 taps and cutoff 1 their value hangs on that ulp -- DESIGN.md section 4).
 * taps is clamped to >= 4 and raised to even as at processing time.  *phases =
 * P + 1, *taps_eff = the row length; out (may be NULL to ask for the sizes)
 * receives phases * taps_eff floats.
 * vvhip_resample_run_length: outputs of one row per workgroup of the table kernel
 * for this ratio and tap count; 0 when the table does not fit and the per-output
 * f64 kernel runs instead.
 * vvhip_resample_sinc_device: d_table = the table above on the stream's device
 * (table kernel), or NULL (generic kernel); knob RESAMPLE_GENERIC = 1 forces
 * the generic kernel. */
int vvhip_resample_table_host(unsigned num, unsigned den, unsigned taps, float* out, size_t* phases,
                              unsigned* taps_eff);
size_t vvhip_resample_run_length(unsigned num, unsigned den, unsigned taps);
/* the packed table [phases][taps] onto the current device in the table kernel's
 * padded row layout; release with vvhip_free */
int vvhip_resample_table_upload(const float* table, size_t phases, unsigned taps, float** d_table);
int vvhip_resample_linear_device(const float* d_in, size_t in_n, size_t nch, size_t in_stride, float* d_out,
                                 size_t out_n, size_t out_stride, double ratio, void* stream);
int vvhip_resample_sinc_device(const float* d_in, size_t in_n, size_t nch, size_t in_stride, float* d_out,
                               size_t out_n, size_t out_stride, double ratio, double cutoff, unsigned taps,
                               const float* d_table, size_t phases, void* stream);

/* ---- Interpolation at arbitrary positions (src/resample/interpolate.c:4-64) ----
 * `batch` rows of n samples x_stride floats apart (0: one row for every output
 * row), m positions per row -> rows of m outputs out_stride floats apart, one
 * launch; no alignment required.  method 0 linear, 1 cubic (Catmull-Rom), each
 * output the reference's value bit for bit; a NaN position gives that NaN.
 * _device: d_pos rows pos_stride floats apart, 0: one row of positions shared by
 * every signal row.  _uniform_device: position k = (float)(start + (double)k *
 * step), product and sum rounded separately; no position array is read.
 * Checks, before any device work: null pointers (1); n == 0 (2); m == 0 or
 * batch == 0 (0, nothing written); a non-zero stride shorter than its row, or
 * out_stride 0 with batch > 1 (2); an unknown method (3); n >= 2^31 (2).
 * d_out may not overlap d_x or d_pos (not detected).
 * vvhip_interp_run_length: consecutive outputs of one row per workgroup.
 * Where one position array serves several rows a workgroup takes its run through
 * 8 signal rows, reusing the positions and what they decide; knob INTERP_ROWS = 1
 * forces one row per workgroup; the bits are the same ("STAT_INTERP_ONE" /
 * "STAT_INTERP_ROWS" count the launches of either route).
 * _host: one row, positions and outputs in host memory. */
size_t vvhip_interp_run_length(void);
int vvhip_interp_device(const float* d_x, size_t n, size_t batch, size_t x_stride, const float* d_pos, size_t m,
                        size_t pos_stride, int method, float* d_out, size_t out_stride, void* stream);
int vvhip_interp_uniform_device(const float* d_x, size_t n, size_t batch, size_t x_stride, double start, double step,
                                size_t m, int method, float* d_out, size_t out_stride, void* stream);
int vvhip_interp_host(const float* x, size_t n, const float* pos, size_t m, int method, float* out);

/* ---- Hilbert analytic signal (hilbert.c:14-75) ---- */
int vvhip_hilbert_host(const float* x, size_t n, float* z_out);
int vvhip_hilbert_device(const float* d_x, size_t n, size_t batch, float* d_z, void* stream);
/* Instantaneous phase / frequency (hilbert.c:77-113) of `batch` contiguous rows
 * of n samples: z complex[batch][n] -> unwrapped phase real[batch][n];
 * phase -> frequency in Hz (freq[row][0] = 0), fs the sample rate. */
int vvhip_inst_phase_host(const float* z, size_t n, float* phase);
int vvhip_inst_phase_device(const float* d_z, size_t n, size_t batch, float* d_phase, void* stream);
int vvhip_inst_freq_host(const float* phase, size_t n, double fs, float* freq);
int vvhip_inst_freq_device(const float* d_phase, size_t n, size_t batch, double fs, float* d_freq, void* stream);

/* ---- Chirp-z transform (src/spectral/czt.c:58-178) ----
 * X[k] = sum_{n<N} x[n] A^-n W^(nk), k < M (scipy.signal.czt convention).  A plan
 * holds the chirps and the chirp's spectrum for P = next_pow2(N + M - 1) <= 2^24.
 * Device: `batch` contiguous rows, x complex[batch][N] (real_in 0) or
 * real[batch][N] (real_in 1) -> X complex[batch][M]. */
int vvhip_czt_create(size_t n, size_t m, float w_re, float w_im, float a_re, float a_im, vvhip_czt** out);
void vvhip_czt_destroy(vvhip_czt* h);
int vvhip_czt_exec_device(const vvhip_czt* h, const void* d_x, int real_in, size_t batch, void* d_X,
                          void* stream);
int vvhip_czt_exec_host(const void* x, int real_in, size_t n, size_t m, float w_re, float w_im, float a_re,
                        float a_im, void* X);

/* ---- Cepstrum / minimum phase (src/envelope/cepstrum.c:7-78, minphase.c:7-31) ----
 * `batch` contiguous rows of n: real cepstrum Re IFFT(log(|FFT x| + 1e-12));
 * Re IFFT(exp(Re FFT(fold c))) and the spectrum exp(Re FFT(fold c)) (complex,
 * imaginary parts 0), fold c = (c0, 2 c1 .. 2 c(n/2-1), 0 ..). */
int vvhip_cepstrum_device(const float* d_x, size_t n, size_t batch, float* d_c, void* stream);
int vvhip_icepstrum_minphase_device(const float* d_c, size_t n, size_t batch, float* d_x, void* stream);
int vvhip_minphase_from_cepstrum_device(const float* d_c, size_t n, size_t batch, float* d_spec, void* stream);
int vvhip_cepstrum_host(const float* x, size_t n, float* c);
int vvhip_icepstrum_minphase_host(const float* c, size_t n, float* x);
int vvhip_minphase_from_cepstrum_host(const float* c, size_t n, float* spec);

/* ---- Linear prediction (src/envelope/lpc.c:7-72) ----
 * `batch` contiguous rows: x [batch][n] -> r [batch][order+1] (lags 0..order);
 * r -> a [batch][order+1], err [batch] by the reference's Levinson-Durbin
 * recursion (A(z) = 1 + sum a[m] z^-m), bit-identical to it given the same r;
 * lpc = the two in one launch, bit-identical to them in sequence.  A row with
 * r[0] <= 0 (the reference's INTERNAL) gets a = {1, 0, ..}, err = 0 and sets
 * *d_flag (an int on the device, may be NULL) to 1.
 * _lpc_frames_: the same over `frames` frames per channel of signal [nch][n],
 * gathered as vvhip_fetch_frames_device gathers them, into a [ch][frame][order+1]
 * and err [ch][frame], channels a_ch_stride / err_ch_stride floats apart.
 * _lpspec_: mag [batch][nfft] = g / |1 - sum a[m] e^(-j 2 pi m k / nfft)| (the
 * reference's sign, lpc.c:60-69) or, levinson_sign != 0, g / |1 + sum ..|;
 * g = d_gain[row], or `gain` when d_gain is NULL.
 * Orders <= 32 on rows <= 4096 take the wave kernel, any other order < n the
 * generic kernels; knob LPC_GENERIC = 1 forces those ("STAT_LPC_WAVE" /
 * "STAT_LPC_GENERIC" count which ran). */
int vvhip_autocorr_device(const float* d_x, size_t n, size_t order, size_t batch, float* d_r, void* stream);
int vvhip_levinson_device(const float* d_r, size_t order, size_t batch, float* d_a, float* d_err, int* d_flag,
                          void* stream);
int vvhip_lpc_device(const float* d_x, size_t n, size_t order, size_t batch, float* d_a, float* d_err, int* d_flag,
                     void* stream);
int vvhip_lpc_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                            size_t hop, size_t frames, int center, const float* d_window, size_t order, float* d_a,
                            size_t a_ch_stride, float* d_err, size_t err_ch_stride, void* stream);
int vvhip_lpspec_device(const float* d_a, size_t order, const float* d_gain, float gain, size_t nfft, size_t batch,
                        int levinson_sign, float* d_mag, void* stream);
int vvhip_autocorr_host(const float* x, size_t n, size_t order, float* r);
int vvhip_levinson_host(const float* r, size_t order, float* a, float* err);
int vvhip_lpc_host(const float* x, size_t n, size_t order, float* a, float* err);
int vvhip_lpspec_host(const float* a, size_t order, float gain, size_t nfft, float* mag);

/* ---- Biquad cascade (src/filter/iir.c:21-43) ----
 * coef [stages][5] = b0 b1 b2 a1 a2, state [rows][stages][2] = z1 z2 (in/out;
 * NULL: zero in, none written), one cascade for all rows; y may be x.  Rows of
 * n <= 8192 run as one recurrence (bit-identical to the reference), longer
 * ones in chunks of 1024 with the boundary states propagated in f64
 * (iir_kernels.hip).  Knob IIR_CHUNK: 0 never chunks, k > 0 chunks of k;
 * "STAT_IIR_EXACT" / "STAT_IIR_CHUNKED" count the calls of either route.
 * _host: one row, coefficients and state in host memory. */
int vvhip_iir_device(const float* d_coef, size_t stages, float* d_state, const float* d_x, float* d_y, size_t n,
                     size_t batch, size_t x_stride, size_t y_stride, void* stream);
int vvhip_iir_host(const float* coef, size_t stages, float* state, const float* x, float* y, size_t n);

/* ---- Savitzky-Golay (src/filter/savgol.c:164-217) ----
 * h: the window's m coefficients in HOST memory (m odd, <= 257; designed by
 * vv_dsp_savgol_coeffs, csrc/host/savgol.c) -- they travel as kernel
 * arguments.  mode as vv_dsp_savgol_mode, nan_policy as core/nan_policy.h
 * (0..3), applied to the samples read and to the outputs; policy 2 waits for
 * the stream and returns 5 when either met a NaN or Inf. */
int vvhip_savgol_device(const float* d_x, size_t n, size_t batch, size_t x_stride, const float* h, int m, int mode,
                        int nan_policy, float* d_y, size_t y_stride, void* stream);
int vvhip_savgol_host(const float* x, size_t n, const float* h, int m, int mode, int nan_policy, float* y);

/* ---- Array statistics and lagged correlations (src/core/core.c:42-108,
 * src/core/stats.c:10-139) ----
 * vvhip_stats_out: one pointer per output, NULL = not wanted, else one value
 * per row (the layout of vv_dsp_stats_out, vv_dsp_amd.h).  _stats_: `batch`
 * rows of n samples row_stride floats apart; _stats_frames_: `frames` frames
 * per channel of signal [nch][n], gathered as vvhip_fetch_frames_device gathers
 * them, value of (ch, frame) at out + ch * out_ch_stride + frame.  One launch
 * writes every requested output; none requested: 0, nothing launched; a
 * requested output whose size rule fails (var n < 2, skewness n < 3, kurtosis
 * n < 4): 2, nothing written.  Rows up to 16384 samples take the wave kernel,
 * longer ones the long route (chunks of 4096 through scratch); knob
 * STATS_LONG = 1 forces it ("STAT_STATS_WAVE" / "STAT_STATS_LONG" count which
 * ran); both give the same bits (stats_kernels.hip).
 * Correlations: x [batch][nx], y [batch][ny] -> r [batch][r_len], r[lag] = the
 * f64 sum of x[i] y[i + lag] over the overlapping samples, over their count
 * (biased 0) or over nx (biased 1); 0 where nothing overlaps.
 * _stats_host: one row; bit k of mask = member k of vvhip_stats_out, float
 * outputs into vals[k] (k < 9), counts and indices into idx[k - 9]. */
typedef struct vvhip_stats_out {
    float *sum, *mean, *var, *rms, *min, *max, *crest, *skewness, *kurtosis;
    uint32_t *zero_crossings, *argmin, *argmax;
} vvhip_stats_out;
int vvhip_stats_device(const float* d_x, size_t n, size_t batch, size_t row_stride, const vvhip_stats_out* out,
                       void* stream);
int vvhip_stats_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                              size_t hop, size_t frames, int center, const float* d_window,
                              const vvhip_stats_out* out, size_t out_ch_stride, void* stream);
int vvhip_autocorrelation_device(const float* d_x, size_t n, size_t batch, size_t r_len, int biased, float* d_r,
                                 void* stream);
int vvhip_cross_correlation_device(const float* d_x, size_t nx, const float* d_y, size_t ny, size_t batch,
                                   size_t r_len, int biased, float* d_r, void* stream);
int vvhip_stats_host(const float* x, size_t n, unsigned mask, float* vals, size_t* idx);
int vvhip_cross_correlation_host(const float* x, size_t nx, const float* y, size_t ny, float* r, size_t r_len,
                                 int biased);

/* ---- Per-frame pitch by YIN (include/vv_dsp/features/pitch.h: the algorithm
 * and the checks, made in its order before any device work) ----
 * vvhip_pitch_params / vvhip_pitch_out: the layouts of vv_dsp_pitch_params and
 * vv_dsp_pitch_out.  _lag_range: host arithmetic, each output may be NULL,
 * nothing written unless the result is 0.  _pitch_: `batch` rows of n samples
 * row_stride floats apart, row r's curve at cmnd + r * cmnd_row_stride;
 * _pitch_frames_: `frames` frames per channel of signal [nch][n], gathered as
 * vvhip_fetch_frames_device gathers them, value of (ch, frame) at out + ch *
 * out_ch_stride + frame and its curve at cmnd + ch * cmnd_ch_stride + frame *
 * (tau_max + 1).  No output wanted: 0, nothing launched.  One kernel, one wave
 * per row ("STAT_PITCH_WAVE" counts its launches; pitch_kernels.hip).  The row
 * sits in LDS as f64 where four rows fit 64 KiB and as f32 beyond; knob
 * PITCH_F32 = 1 forces f32, with the same bits.
 * _host: one frame in host memory; f0 and aperiodicity may each be NULL. */
typedef struct vvhip_pitch_params {
    float sample_rate, fmin, fmax, threshold;
} vvhip_pitch_params;
typedef struct vvhip_pitch_out {
    float *f0, *aperiodicity;
    uint32_t* lag;
    float* cmnd;
} vvhip_pitch_out;
int vvhip_pitch_lag_range(const vvhip_pitch_params* params, size_t frame_len, size_t* tau_min, size_t* tau_max,
                          size_t* integration_len);
int vvhip_pitch_device(const float* d_x, size_t n, size_t batch, size_t row_stride, const vvhip_pitch_params* params,
                       const vvhip_pitch_out* out, size_t cmnd_row_stride, void* stream);
int vvhip_pitch_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                              size_t hop, size_t frames, int center, const float* d_window,
                              const vvhip_pitch_params* params, const vvhip_pitch_out* out, size_t out_ch_stride,
                              size_t cmnd_ch_stride, void* stream);
int vvhip_pitch_host(const float* x, size_t n, const vvhip_pitch_params* params, float* f0, float* aperiodicity);

/* ---- f0 tracking over the YIN curves (include/vv_dsp/features/pitch_track.h:
 * the definition and the checks, made in its order before any device work) ----
 * vvhip_pitch_track_params / vvhip_pitch_track_out: the layouts of
 * vv_dsp_pitch_track_params and vv_dsp_pitch_track_out.  _params_default: host
 * arithmetic over vvhip_pitch_lag_range.  _track_: curves [nch][frames][row_stride]
 * (channels cmnd_ch_stride floats apart) -> planes [nch][frames] (channels
 * out_ch_stride values apart) and cost [nch].  _track_frames_: signal [nch][n] ->
 * the same planes: vvhip_pitch_frames_device into scratch curves, then the
 * tracker, in channel groups of at most 2 GiB of curves (at least one channel);
 * track->tau_max must not exceed the curves' last lag.  The tracker's own scratch
 * is one byte per state and frame, in channel groups of at most 4 GiB.  Knob
 * PTRACK_GROUP = g > 0 forces groups of g channels; no value depends on it.
 * "STAT_PITCH_TRACK" counts the tracker's launches (pitch_track_kernels.hip).
 * _host: one channel of curves in host memory. */
typedef struct vvhip_pitch_track_params {
    float sample_rate;
    uint32_t tau_min, tau_max;
    float lambda, jump_cost, switch_cost, unvoiced_cost;
    uint32_t max_step;
} vvhip_pitch_track_params;
typedef struct vvhip_pitch_track_out {
    uint32_t* lag;
    float *f0, *aperiodicity;
    double* cost;
} vvhip_pitch_track_out;
int vvhip_pitch_track_params_default(const vvhip_pitch_params* pitch, size_t frame_len,
                                     vvhip_pitch_track_params* track);
int vvhip_pitch_track_device(const float* d_curves, size_t frames, size_t nch, size_t row_stride,
                             size_t cmnd_ch_stride, const vvhip_pitch_track_params* params,
                             const vvhip_pitch_track_out* out, size_t out_ch_stride, void* stream);
int vvhip_pitch_track_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                                    size_t hop, size_t frames, int center, const float* d_window,
                                    const vvhip_pitch_params* pitch, const vvhip_pitch_track_params* track,
                                    const vvhip_pitch_track_out* out, size_t out_ch_stride, void* stream);
int vvhip_pitch_track_host(const float* curves, size_t frames, size_t row_stride,
                           const vvhip_pitch_track_params* params, const vvhip_pitch_track_out* out);

/* ---- Per-frame spectral shape (include/vv_dsp/features/spectral_shape.h: the
 * definitions and the checks, made in its order before any device work) ----
 * vvhip_shape_params / vvhip_shape_out / vvhip_shape_values: the layouts of
 * vv_dsp_spectral_shape_params, _out and _values.  _shape_: `rows` rows of
 * n_fft/2 + 1 powers row_pitch floats apart, groups of rows_per_group rows (0: one
 * group), value of row r at out + r.  _stft_shape_: the handle's power rows
 * (vvhip_stft_power_pitched_device, whole 128 B lines per row) into
 * stream-ordered scratch, then _shape_ with one group per channel, value of
 * (ch, frame) at out + ch * out_ch_stride + frame.  No output wanted: 0, nothing
 * launched.  One kernel, one wave per run of rows ("STAT_SHAPE_WAVE" counts its
 * launches, "STAT_SHAPE_VEC16" those with 16-byte loads; shape_kernels.hip);
 * knob SHAPE_DWORD = 1 forces 4-byte loads, with
 * the same bits.  _host: one row (and its predecessor, or NULL) in host memory. */
typedef struct vvhip_shape_params {
    size_t n_fft;
    float sample_rate;
    int magnitude;
    size_t k_min, k_max;
    float rolloff, floor;
} vvhip_shape_params;
typedef struct vvhip_shape_out {
    float *energy, *centroid, *spread, *skewness, *kurtosis, *flatness, *rolloff, *flux, *crest;
    uint32_t* peak_bin;
} vvhip_shape_out;
typedef struct vvhip_shape_values {
    float energy, centroid, spread, skewness, kurtosis, flatness, rolloff, flux, crest;
    uint32_t peak_bin;
} vvhip_shape_values;
int vvhip_shape_device(const float* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                       const vvhip_shape_params* params, const vvhip_shape_out* out, void* stream);
int vvhip_stft_shape_device(vvhip_stft* h, const vvhip_shape_params* params, const float* d_signal, size_t n,
                            size_t nch, size_t ch_stride, const vvhip_shape_out* out, size_t out_ch_stride,
                            void* stream);
int vvhip_shape_host(const float* row, const float* prev, const vvhip_shape_params* params, vvhip_shape_values* out);

/* ---- Phase vocoder (include/vv_dsp/spectral/phase_vocoder.h: the definition and
 * the checks, made in its order before any device work) ----
 * d_spec [nch][T][n_fft] float pairs, channels spec_ch_stride pairs apart ->
 * d_out [nch][m][n_fft], channels out_ch_stride pairs apart.  d_pos null: output
 * row j at start + j step (check 3 applies); else at d_pos[j].  Three launches
 * (pvoc_kernels.hip; "STAT_PVOC_ROWS" counts the calls that made them; knob
 * PVOC_PLANE = 1: a fourth launch stores the rows' phases in an f64 plane the
 * walks read, with the same bits).
 * _host: one channel in host memory, uniform form.
 * _stft_stretch_: signal [nch][n] -> signal [nch][out_len] through the handle's
 * spectrum rows, the vocoder at start 0 and step rate, the overlap-add and the
 * division by the summed squared window, in channel groups (knob PVOC_GROUP).
 * _stretch_length: rows m and samples out_len of that call. */
int vvhip_pvoc_device(const float* d_spec, size_t T, size_t n_fft, size_t nch, size_t spec_ch_stride,
                      const float* d_pos, double start, double step, size_t m, float* d_out, size_t out_ch_stride,
                      void* stream);
int vvhip_pvoc_host(const float* spec, size_t T, size_t n_fft, double start, double step, size_t m, float* out);
int vvhip_stft_stretch_length(size_t n, size_t nfft, size_t hop, double rate, size_t* rows, size_t* out_len);
int vvhip_stft_stretch_device(vvhip_stft* h, const float* d_signal, size_t n, size_t nch, size_t ch_stride,
                              double rate, float* d_out, size_t out_ch_stride, void* stream, size_t* out_len);

/* ---- Running median and HPSS (include/vv_dsp/filter/median.h and
 * include/vv_dsp/spectral/hpss.h: the definitions and the checks, made in their
 * order before any device work; median_kernels.hip) ----
 * _medfilt_: `batch` rows of n floats, strides in floats; _host: one row in host
 * memory.  Knob MEDIAN_SELECT = 1 / 2 forces the counting / the bitwise select
 * (same bits).  vvhip_hpss_params / vvhip_hpss_out: the layouts of
 * vv_dsp_hpss_params and _out.  _hpss_: power rows -> the planes that are
 * wanted; _hpss_host: one group of packed rows in host memory.  _stft_hpss_:
 * signal [nch][n] -> the harmonic and the percussive signal [nch][out_len], in
 * channel groups (knob HPSS_GROUP = k: k channels per group). */
typedef struct vvhip_hpss_params {
    size_t n_fft;
    int magnitude, win_harm, win_perc;
    float margin_harm, margin_perc;
    int mask;
} vvhip_hpss_params;
typedef struct vvhip_hpss_out {
    float *harm, *perc, *mask_harm, *mask_perc;
} vvhip_hpss_out;
int vvhip_medfilt_device(const float* d_x, size_t n, size_t batch, size_t x_stride, int window_length, int mode,
                         float* d_y, size_t y_stride, void* stream);
int vvhip_medfilt_host(const float* x, size_t n, int window_length, int mode, float* y);
int vvhip_hpss_device(const float* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                      const vvhip_hpss_params* params, const vvhip_hpss_out* out, size_t out_pitch, void* stream);
int vvhip_hpss_host(const float* power_rows, size_t rows, const vvhip_hpss_params* params, const vvhip_hpss_out* out);
int vvhip_stft_hpss_device(vvhip_stft* h, const vvhip_hpss_params* params, const float* d_signal, size_t n, size_t nch,
                           size_t ch_stride, float* d_out_harm, float* d_out_perc, size_t out_ch_stride,
                           void* stream, size_t* out_len);

/* ---- Spectral noise suppression (include/vv_dsp/spectral/denoise.h: the
 * definition and the checks, made in its order before any device work;
 * denoise_kernels.hip) ----
 * vvhip_denoise_params / vvhip_denoise_out: the layouts of vv_dsp_denoise_params
 * and _out.  _denoise_: power rows -> the planes that are wanted, one launch;
 * _denoise_host: one group of packed rows in host memory.  _stft_denoise_: signal
 * [nch][n] -> the denoised signal [nch][out_len], in channel groups (knob
 * DENOISE_GROUP = k: k channels per group).  Knobs DENOISE_SEGMENT = L (the
 * segment length of the walk down the rows) and DENOISE_MIN = 1 / 2 (the direct /
 * the blockwise minimum) change no value; STAT_DENOISE counts the launches. */
typedef struct vvhip_denoise_params {
    size_t n_fft;
    int smooth_len, back, ahead;
    float bias, floor;
    int mode;
} vvhip_denoise_params;
typedef struct vvhip_denoise_out {
    float *smooth, *noise, *gain;
} vvhip_denoise_out;
int vvhip_denoise_device(const float* d_power, size_t rows, size_t row_pitch, size_t rows_per_group,
                         const vvhip_denoise_params* params, const vvhip_denoise_out* out, size_t out_pitch,
                         void* stream);
int vvhip_denoise_host(const float* power_rows, size_t rows, const vvhip_denoise_params* params,
                       const vvhip_denoise_out* out);
int vvhip_stft_denoise_device(vvhip_stft* h, const vvhip_denoise_params* params, const float* d_signal, size_t n,
                              size_t nch, size_t ch_stride, float* d_out, size_t out_ch_stride, void* stream,
                              size_t* out_len);

/* ---- LSF, reflection coefficients and formants of LPC rows
 * (include/vv_dsp/envelope/lsf.h, include/vv_dsp/features/formant.h; entry
 * points as vv_dsp_amd.h's, `frames` per channel given by the caller) ----
 * vvhip_formant_params / vvhip_formant_out: the layouts of vv_dsp_formant_params
 * and vv_dsp_formant_out.  "STAT_LSF" / "STAT_FORMANT" count the launches of
 * lsf_kernels.hip / formant_kernels.hip; knob LSF_GROUP = g > 0 forces channel
 * groups of g in the two _frames_ calls. */
typedef struct vvhip_formant_params {
    float sample_rate, f_min, f_max, bw_max;
    uint32_t n_formants;
} vvhip_formant_params;
typedef struct vvhip_formant_out {
    float* freq;
    float* bw;
    int32_t* count;
    int32_t* flags;
    double* roots;
} vvhip_formant_out;
int vvhip_lpc_to_lsf_device(const float* d_a, size_t order, size_t batch, size_t a_pitch, float* d_lsf, float* d_rc,
                            int32_t* d_flags, void* stream);
int vvhip_lsf_to_lpc_device(const float* d_lsf, size_t order, size_t batch, float* d_a, size_t a_pitch, void* stream);
int vvhip_lsf_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                            size_t hop, size_t frames, int center, const float* d_window, size_t order, float* d_lsf,
                            float* d_rc, int32_t* d_flags, float* d_err, void* stream);
int vvhip_lpc_to_lsf_host(const float* a, size_t order, float* lsf, float* rc, int32_t* flags);
int vvhip_lsf_to_lpc_host(const float* lsf, size_t order, float* a);
int vvhip_formant_params_default(float sample_rate, vvhip_formant_params* params);
int vvhip_formant_start_points(size_t order, double* out);
int vvhip_lpc_formants_device(const float* d_a, size_t order, size_t batch, size_t a_pitch,
                              const vvhip_formant_params* params, const vvhip_formant_out* out, void* stream);
int vvhip_formants_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                                 size_t hop, size_t frames, int center, const float* d_window, size_t order,
                                 const vvhip_formant_params* params, const vvhip_formant_out* out, void* stream);
int vvhip_lpc_formants_host(const float* a, size_t order, const vvhip_formant_params* params,
                            const vvhip_formant_out* out);

/* ---- LPC residual and synthesis filters (include/vv_dsp/envelope/lpc_filter.h;
 * entry points as vv_dsp_amd.h's, `frames` per channel of the _frames_ call given
 * by the caller) ----
 * "STAT_LPC_RESIDUAL" / "STAT_LPC_SYNTH_EXACT" / "STAT_LPC_SYNTH_CHUNKED" count
 * the calls of each route of lpc_filter_kernels.hip.  Knob LPC_SYNTH_CHUNK: 0
 * never chunks, k > 0 forces chunks of k; knob LPC_FILTER_GROUP = g > 0 forces
 * channel groups of g where scratch is taken per group (the chunked synthesis
 * and the _frames_ call). */
int vvhip_lpc_residual_device(const float* d_x, size_t n, size_t nch, size_t x_stride, const float* d_a, size_t order,
                              size_t frames, size_t a_pitch, size_t a_ch_stride, const float* d_gain,
                              size_t g_ch_stride, size_t seg_len, long long offset, double* d_state, float* d_e,
                              size_t e_stride, void* stream);
int vvhip_lpc_synth_device(const float* d_e, size_t n, size_t nch, size_t e_stride, const float* d_a, size_t order,
                           size_t frames, size_t a_pitch, size_t a_ch_stride, const float* d_gain, size_t g_ch_stride,
                           size_t seg_len, long long offset, double* d_state, float* d_y, size_t y_stride,
                           void* stream);
int vvhip_lpc_residual_frames_device(const float* d_signal, size_t n, size_t nch, size_t ch_stride, size_t frame_len,
                                     size_t hop, size_t frames, int center, const float* d_window, size_t order,
                                     float* d_a, size_t a_ch_stride, float* d_err, size_t err_ch_stride, float* d_e,
                                     size_t e_stride, void* stream);
int vvhip_lpc_residual_host(const float* x, size_t n, const float* a, size_t order, size_t frames, size_t seg_len,
                            long long offset, const float* gain, double* state, float* e);
int vvhip_lpc_synth_host(const float* e, size_t n, const float* a, size_t order, size_t frames, size_t seg_len,
                         long long offset, const float* gain, double* state, float* y);

/* ---- Spectral utilities (src/spectral/utils.c:5-73) ----
 * `batch` contiguous rows of n: fftshift (inverse 0) / ifftshift (inverse 1) of
 * float (cpx 0) or complex (cpx 1) rows, a permutation (in place allowed);
 * phase wrap of `count` floats into (-pi, pi]; phase unwrap of each row. */
int vvhip_fftshift_device(const void* d_in, void* d_out, size_t n, size_t batch, int cpx, int inverse,
                          void* stream);
int vvhip_phase_wrap_device(const float* d_in, float* d_out, size_t count, void* stream);
int vvhip_phase_unwrap_device(const float* d_in, float* d_out, size_t n, size_t batch, void* stream);
int vvhip_fftshift_host(const void* in, void* out, size_t n, int cpx, int inverse);
int vvhip_phase_wrap_host(const float* in, float* out, size_t n);
int vvhip_phase_unwrap_host(const float* in, float* out, size_t n);

/* ---- DCT (dct.c:86-136); nan_policy as core/nan_policy.h (0..3) ---- */
int vvhip_dct_host(const float* in, float* out, size_t n, int type, int dir, int nan_policy);
int vvhip_dct_device(const float* d_in, float* d_out, size_t n, size_t batch, int type, int dir,
                     int nan_policy, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
