/* vv_dsp_amd.h -- ADDITIVE batched / device-pointer entry points of the MI355X
 * backend.  The reference API (fft.h, stft.h, ...) is host-pointer and one
 * transform per call, which pays PCIe per call; these entry points take
 * device (HBM) pointers and whole batches and run asynchronously on a HIP
 * stream passed as void* (NULL = default stream).  Nothing here changes the
 * reference's C99 ABI. */
#ifndef VV_DSP_AMD_H
#define VV_DSP_AMD_H
#include <stdint.h>
#include "vv_dsp/vv_dsp_types.h"
#include "vv_dsp/spectral/fft.h"
#include "vv_dsp/spectral/stft.h"
#include "vv_dsp/spectral/dct.h"
#include "vv_dsp/filter/fir.h"
#include "vv_dsp/filter/iir.h"
#include "vv_dsp/filter/savgol.h"
#include "vv_dsp/filter/median.h"
#include "vv_dsp/features/mel.h"
#include "vv_dsp/features/pitch.h"
#include "vv_dsp/features/pitch_track.h"
#include "vv_dsp/features/formant.h"
#include "vv_dsp/features/spectral_shape.h"
#include "vv_dsp/spectral/czt.h"
#include "vv_dsp/spectral/phase_vocoder.h"
#include "vv_dsp/spectral/hpss.h"
#include "vv_dsp/spectral/denoise.h"
#include "vv_dsp/envelope/cepstrum.h"
#include "vv_dsp/envelope/minphase.h"
#include "vv_dsp/envelope/lpc.h"
#include "vv_dsp/envelope/lsf.h"
#include "vv_dsp/envelope/lpc_filter.h"
#include "vv_dsp/resample/resampler.h"
#include "vv_dsp/resample/interpolate.h"
#include "vv_dsp/core/stats.h"

#ifdef __cplusplus
extern "C" {
#endif

/* number of usable HIP devices */
int vv_dsp_amd_device_count(void);
const char* vv_dsp_amd_last_error(void);
/* The calling thread's device for the device-pointer calls below (hipSetDevice):
 * one process per GPU sets it once; one process driving several GPUs switches it
 * per shard.  OUT_OF_RANGE for a bad index, UNSUPPORTED with no device. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_amd_set_device(int device);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_amd_get_device(int* device);

/* FFT: `batch` contiguous transforms per execute (host or device pointers). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_fft_make_plan_many(size_t n, vv_dsp_fft_type type, vv_dsp_fft_dir dir,
                                                         size_t batch, vv_dsp_fft_plan** out_plan);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_fft_execute_device(const vv_dsp_fft_plan* plan, const void* d_in,
                                                         void* d_out, void* stream);

/* STFT over nch channels (ch_stride floats apart) into [ch][frame][fft_size]
 * rows (out_ch_stride floats apart): magnitudes (_spectrogram_) or complex
 * spectra (_spectrum_). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_spectrogram_device(vv_dsp_stft* h, const vv_dsp_real* d_signal,
                                                              size_t n, size_t nch, size_t ch_stride,
                                                              vv_dsp_real* d_out_mag, size_t out_ch_stride,
                                                              void* stream, size_t* out_frames);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_spectrum_device(vv_dsp_stft* h, const vv_dsp_real* d_signal,
                                                           size_t n, size_t nch, size_t ch_stride,
                                                           vv_dsp_cpx* d_out, size_t out_ch_stride,
                                                           void* stream, size_t* out_frames);
/* power spectrogram [ch][frame][fft_size/2+1] = re^2 + im^2 of bins 0..fft_size/2
 * (the input of vv_dsp_compute_log_mel_spectrogram / vv_dsp_mfcc_process) */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_power_device(vv_dsp_stft* h, const vv_dsp_real* d_signal,
                                                        size_t n, size_t nch, size_t ch_stride,
                                                        vv_dsp_real* d_out_power, size_t out_ch_stride,
                                                        void* stream, size_t* out_frames);
/* The same power rows placed row_pitch floats apart (row_pitch >= fft_size/2+1;
 * the pad floats past bin fft_size/2 are not written; out_ch_stride >= frames x
 * row_pitch).  A pitch of a whole number of 128 B lines -- 544 for fft_size
 * 1024: 17 lines -- starts every row on a line, so the rows leave as whole-line
 * stores; the values equal vv_dsp_stft_power_device's bit for bit.  The
 * reference's packed layout (mel.h:156-161) is row_pitch = fft_size/2+1. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_power_pitched_device(vv_dsp_stft* h, const vv_dsp_real* d_signal,
                                                                size_t n, size_t nch, size_t ch_stride,
                                                                vv_dsp_real* d_out_power, size_t out_ch_stride,
                                                                size_t row_pitch, void* stream, size_t* out_frames);
/* One shard of a long signal's frames: rows of frames [frame0, frame0 + nframes)
 * of the same spectrogram, row of frame f at d_out + (f - frame0) * row.
 * out_kind 0: magnitudes [fft_size] floats, 1: complex spectrum [fft_size]
 * vv_dsp_cpx, 2: power [fft_size/2+1] floats.  Even frame0 gives rows
 * bit-identical to the whole-signal call.  VV_DSP_ERROR_OUT_OF_RANGE when the
 * range passes the last frame (stft.c:119 frame count). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_frames_range_device(vv_dsp_stft* h, const vv_dsp_real* d_signal,
                                                               size_t n, size_t nch, size_t ch_stride,
                                                               size_t frame0, size_t nframes, void* d_out,
                                                               size_t out_ch_stride, int out_kind, void* stream);
/* the handle's fft_size and hop_size (either pointer may be NULL) */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_get_sizes(const vv_dsp_stft* h, size_t* fft_size, size_t* hop_size);
/* ---- Multi-GPU layout of config 5: channels shard with no
 * exchange; the only collective is the caller's gather of the rows. ----
 * The contiguous block split rank `rank` of `world` owns: channels
 * [*first, *first + *count), rank order = channel order, sizes differ by at most
 * one (the same split as vv-dsp_amd/vvdsp_dist.py channel_shard).  The RCCL
 * shard + gather entry points are in vv_dsp/vv_dsp_dist.h. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_shard_range(size_t total, size_t world, size_t rank, size_t* first,
                                                  size_t* count);
/* One rank's share of a multi-channel spectrogram on `device`: the rows of
 * channels [first, first + count) of a [total][n] job (d_signal points at the
 * shard's first channel, on that device) into d_out [count][frames][row].
 * out_kind as vv_dsp_stft_frames_range_device (0 magnitude, 1 complex, 2 power
 * n/2+1).  The handle may be shared by all devices: its window is copied to
 * each device once.  The thread's current device is restored on return. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_channel_shard_device(vv_dsp_stft* h, int device,
                                                                const vv_dsp_real* d_signal, size_t n, size_t count,
                                                                size_t ch_stride, int out_kind, void* d_out,
                                                                size_t out_ch_stride, void* stream, size_t* out_frames);
/* Half-spectrum rows for the gather: magnitude (or power) rows of real frames
 * are mirror-symmetric, |X[n-k]| = |X[k]|, so a rank can send bins 0..n/2 only
 * (half the xGMI bytes of config 5's gather) and the root expands them.
 * pack: [rows][fft_size] -> [rows][fft_size/2+1]; unpack: the reverse, bin k
 * above fft_size/2 taken from bin fft_size-k.  For rows of the fused STFT
 * kernels (power-of-two fft_size <= 8192, 7-smooth <= 4096) the mirror bins
 * are computed from the same conjugate pair, so unpack(pack(rows)) == rows bit
 * for bit. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_spectrogram_pack_half_device(const vv_dsp_real* d_rows, size_t rows,
                                                                   size_t fft_size, vv_dsp_real* d_half, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_spectrogram_unpack_half_device(const vv_dsp_real* d_half, size_t rows,
                                                                     size_t fft_size, vv_dsp_real* d_rows,
                                                                     void* stream);
/* Batched framing (vv_dsp_fetch_frame / vv_dsp_overlap_add, framing.c:71-146):
 * frames [frame0, frame0 + count) into d_frames[count][frame_len]; and count
 * frames added into d_out[output_len] at (frame0 + f) * hop_len, every output
 * sample summed in frame order (bit-identical to the per-frame loop). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_fetch_frames_device(const vv_dsp_real* d_signal, size_t signal_len,
                                                          vv_dsp_real* d_frames, size_t frame_len, size_t hop_len,
                                                          size_t frame0, size_t count, int center,
                                                          const vv_dsp_real* d_window, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_overlap_add_device(const vv_dsp_real* d_frames, size_t count,
                                                         vv_dsp_real* d_out, size_t output_len, size_t frame_len,
                                                         size_t hop_len, size_t frame0, void* stream);
/* count frames real[count][fft_size] -> cpx[count][fft_size] (vv_dsp_stft_process batched) */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_process_device(vv_dsp_stft* h, const vv_dsp_real* d_frames,
                                                          size_t count, vv_dsp_cpx* d_spec, void* stream);
/* count spectra overlap-added at the handle's hop (vv_dsp_stft_reconstruct batched) */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_reconstruct_device(vv_dsp_stft* h, const vv_dsp_cpx* d_spec,
                                                              size_t count, vv_dsp_real* d_out_add,
                                                              vv_dsp_real* d_norm_add, void* stream);

/* FIR plan: coefficients resident on the device; overlap-save for fir_apply_fft
 * semantics, direct form (bit-identical to vv_dsp_fir_apply) on request. */
typedef struct vv_dsp_fir_plan vv_dsp_fir_plan;
VV_DSP_NODISCARD vv_dsp_status vv_dsp_fir_plan_create(const vv_dsp_real* coeffs, size_t num_taps,
                                                      vv_dsp_fir_plan** out);
vv_dsp_status vv_dsp_fir_plan_destroy(vv_dsp_fir_plan* p);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_fir_apply_fft_device(vv_dsp_fir_plan* p, const vv_dsp_real* d_x,
                                                           vv_dsp_real* d_y, size_t n, size_t nch,
                                                           size_t x_stride, size_t y_stride, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_fir_apply_direct_device(vv_dsp_fir_plan* p, const vv_dsp_real* d_x,
                                                              vv_dsp_real* d_y, size_t n, size_t nch,
                                                              size_t x_stride, size_t y_stride, void* stream);
/* vv_dsp_filtfilt_fir over nch rows (filter/common.c:23-80), bit-identical */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_filtfilt_fir_device(vv_dsp_fir_plan* p, const vv_dsp_real* d_x,
                                                          vv_dsp_real* d_y, size_t n, size_t nch, size_t x_stride,
                                                          size_t y_stride, void* stream);

/* Rational resampler (vv_dsp/resample/resampler.h) on device rows.
 * _output_length: the reference's floor((in_n - 1) * ratio) + 1 in f64 with
 * ratio = (double)num / (double)den; 0 for in_n == 0 or a NULL plan.
 * _process_device: nch rows of in_n samples, in_stride floats apart, into rows
 * out_stride floats apart, one launch on `stream`; *out_n (may be NULL) receives
 * the row length.  Checks as vv_dsp_resampler_process_real, then
 * VV_DSP_ERROR_INVALID_SIZE for in_n >= 2^31 (the reference's centre index is
 * an int).  No alignment of pointers or strides is required.  Linear rows are
 * bit-identical to the reference; sinc rows come from the polyphase table
 * kernel, or from the per-output f64 kernel when the table of the reduced
 * ratio is too large for LDS (vvhip_debug_get("STAT_RESAMPLE_TABLE") /
 * ("STAT_RESAMPLE_GENERIC") count which ran). */
size_t vv_dsp_resampler_output_length(const vv_dsp_resampler* rs, size_t in_n);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_resampler_process_device(vv_dsp_resampler* rs, const vv_dsp_real* d_in,
                                                               size_t in_n, size_t nch, size_t in_stride,
                                                               vv_dsp_real* d_out, size_t out_cap, size_t out_stride,
                                                               void* stream, size_t* out_n);

/* Interpolation of rows at arbitrary fractional positions
 * (vv_dsp/resample/interpolate.h, interpolate.c:4-64): reading a signal along a
 * curve -- vibrato, pitch and tempo warps, reverse playback, non-rational rates.
 * _device: `batch` rows of n samples, x_stride floats apart (0: one signal row
 * read by every output row), at m positions per row from d_pos, rows pos_stride
 * floats apart (0: one row of positions shared by every signal row), into rows
 * of m outputs out_stride floats apart.  One launch on `stream`; no alignment of
 * pointers or strides is required.
 * _uniform_device: position k is (float)(start + (double)k * step), the f64
 * product and the f64 sum rounded separately (no fused multiply-add); no
 * position array is read.
 * _real_batch: one row, positions and outputs in host memory, staged through the
 * device once.
 * Every output is the reference's value for its position, bit for bit:
 * pos <= 0 gives x[0] and pos >= (float)(n - 1) gives x[n - 1], so -Inf and +Inf
 * follow the end clamps; the cubic (Catmull-Rom with clamped neighbour indices)
 * gives x[0] when n < 2, whatever the position; every product and sum is rounded
 * separately, in the reference's order.  A NaN position, which the reference
 * leaves undefined, gives a NaN output and touches nothing else.  The thread's
 * NaN policy is not applied (the reference does not apply it here).
 * Checks, all before any device work, in this order: a NULL pointer
 * (NULL_POINTER); n == 0 (INVALID_SIZE, the reference's order); m == 0 or
 * batch == 0 (OK, nothing written); a non-zero stride shorter than its row, or
 * out_stride == 0 with batch > 1 (INVALID_SIZE); an unknown method
 * (OUT_OF_RANGE); n >= 2^31 (INVALID_SIZE, as the resampler).
 * d_out may not overlap d_x or d_pos; this is not detected.
 * Where one position row serves several signal rows a workgroup takes its run
 * of positions through 8 of them; knob INTERP_ROWS = 1 forces one row per
 * workgroup, and both give the same bits (vvhip_debug_get("STAT_INTERP_ONE") /
 * ("STAT_INTERP_ROWS") count which ran). */
typedef enum vv_dsp_interp_method { VV_DSP_INTERP_LINEAR = 0, VV_DSP_INTERP_CUBIC = 1 } vv_dsp_interp_method;
VV_DSP_NODISCARD vv_dsp_status vv_dsp_interpolate_device(const vv_dsp_real* d_x, size_t n, size_t batch,
                                                         size_t x_stride, const vv_dsp_real* d_pos, size_t m,
                                                         size_t pos_stride, vv_dsp_interp_method method,
                                                         vv_dsp_real* d_out, size_t out_stride, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_interpolate_uniform_device(const vv_dsp_real* d_x, size_t n, size_t batch,
                                                                 size_t x_stride, double start, double step, size_t m,
                                                                 vv_dsp_interp_method method, vv_dsp_real* d_out,
                                                                 size_t out_stride, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_interpolate_real_batch(const vv_dsp_real* x, size_t n, const vv_dsp_real* pos,
                                                             size_t m, vv_dsp_interp_method method, vv_dsp_real* out);

/* Hilbert analytic signal of `batch` contiguous real[N] rows -> cpx[batch][N] */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_hilbert_analytic_device(const vv_dsp_real* d_x, size_t N, size_t batch,
                                                              vv_dsp_cpx* d_z, void* stream);
/* Instantaneous phase (unwrapped, radians) of `batch` contiguous analytic rows
 * cpx[batch][N] -> real[batch][N]; instantaneous frequency (Hz) of phase rows
 * real[batch][N] -> real[batch][N], element 0 of each row = 0 (hilbert.c:77-113). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_instantaneous_phase_device(const vv_dsp_cpx* d_analytic, size_t N,
                                                                 size_t batch, vv_dsp_real* d_phase, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_instantaneous_frequency_device(const vv_dsp_real* d_phase, size_t N,
                                                                     size_t batch, double sample_rate,
                                                                     vv_dsp_real* d_freq, void* stream);
/* DCT of `batch` contiguous rows with the plan's type/direction */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_dct_execute_device(const vv_dsp_dct_plan* plan, const vv_dsp_real* d_in,
                                                         vv_dsp_real* d_out, size_t batch, void* stream);

/* MFCC plan (vv_dsp_mfcc_init) on device rows: power [frames][n_fft/2+1]
 * (e.g. vv_dsp_stft_power_device) -> MFCC [frames][num_mfcc_coeffs], or ->
 * log-mel [frames][n_mels]; one fused kernel, the spectrogram read once. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_mfcc_process_device(const vv_dsp_mfcc_plan* plan, const vv_dsp_real* d_power,
                                                          size_t num_frames, vv_dsp_real* d_out_mfcc, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_log_mel_device(const vv_dsp_mfcc_plan* plan, const vv_dsp_real* d_power,
                                                     size_t num_frames, vv_dsp_real* d_out_log_mel, void* stream);
/* the same on power rows row_pitch >= n_fft/2+1 floats apart (e.g.
 * vv_dsp_stft_power_pitched_device's); the values do not depend on the pitch */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_mfcc_process_pitched_device(const vv_dsp_mfcc_plan* plan,
                                                                  const vv_dsp_real* d_power, size_t num_frames,
                                                                  size_t row_pitch, vv_dsp_real* d_out_mfcc,
                                                                  void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_log_mel_pitched_device(const vv_dsp_mfcc_plan* plan, const vv_dsp_real* d_power,
                                                             size_t num_frames, size_t row_pitch,
                                                             vv_dsp_real* d_out_log_mel, void* stream);
/* Signal -> log-mel / MFCC rows without the power spectrogram in HBM:
 * d_signal [nch][n] (ch_stride floats apart) -> d_out [nch][frames][n_mels]
 * (log-mel) or [nch][frames][num_mfcc_coeffs] (MFCC), out_ch_stride floats
 * apart.  The values are those of vv_dsp_stft_power_device followed by
 * vv_dsp_log_mel_device / vv_dsp_mfcc_process_device (the stft's window,
 * nfft and hop; the plan's filterbank, log epsilon, DCT and lifter), bit for
 * bit.  One kernel computes them with the power rows kept in LDS when
 * nfft = 1024, hop <= 256 and a multiple of 4, the signal 16-B aligned with
 * ch_stride a multiple of 4, n_mels <= 128 (log-mel) or n_mels <= 60 and
 * num_mfcc_coeffs <= 64 (MFCC: the log-mel rows stay in the exchange buffer's
 * spare tail), and a filterbank whose chunk schedule has at most 256 chunks
 * (four per lane; 128 bands over 0-24 kHz at 48 kHz have 308); any other
 * shape runs the two steps through a scratch buffer
 * (vvhip_debug_get("STAT_MEL_FUSED") / ("STAT_MEL_SPLIT") count which ran).
 * The plan's n_fft must equal the stft's nfft (VV_DSP_ERROR_INVALID_SIZE). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_log_mel_device(vv_dsp_stft* h, const vv_dsp_mfcc_plan* plan,
                                                          const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                          size_t ch_stride, vv_dsp_real* d_out, size_t out_ch_stride,
                                                          void* stream, size_t* out_frames);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_mfcc_device(vv_dsp_stft* h, const vv_dsp_mfcc_plan* plan,
                                                       const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                       size_t ch_stride, vv_dsp_real* d_out, size_t out_ch_stride,
                                                       void* stream, size_t* out_frames);

/* Chirp-z plan (vv_dsp_czt_exec_cpx / _real semantics, czt.c:44-178): chirps and
 * the chirp's spectrum resident on the device; `batch` contiguous rows
 * complex[batch][N] (real_input 0) or real[batch][N] (real_input 1) ->
 * complex[batch][M].  N + M - 1 <= 2^24. */
typedef struct vv_dsp_czt_plan vv_dsp_czt_plan;
VV_DSP_NODISCARD vv_dsp_status vv_dsp_czt_plan_create(size_t N, size_t M, vv_dsp_real W_real, vv_dsp_real W_imag,
                                                      vv_dsp_real A_real, vv_dsp_real A_imag, vv_dsp_czt_plan** out);
vv_dsp_status vv_dsp_czt_plan_destroy(vv_dsp_czt_plan* p);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_czt_execute_device(const vv_dsp_czt_plan* p, const void* d_in, int real_input,
                                                         size_t batch, vv_dsp_cpx* d_out, void* stream);
/* Cepstrum family on `batch` contiguous rows of n (cepstrum.c:7-78, minphase.c:7-31) */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_cepstrum_real_device(const vv_dsp_real* d_x, size_t n, size_t batch,
                                                           vv_dsp_real* d_cep, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_icepstrum_minphase_device(const vv_dsp_real* d_c, size_t n, size_t batch,
                                                                vv_dsp_real* d_x, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_minphase_from_cepstrum_device(const vv_dsp_real* d_c, size_t n, size_t batch,
                                                                    vv_dsp_cpx* d_spec, void* stream);
/* Linear prediction on `batch` contiguous rows (vv_dsp/envelope/lpc.h, lpc.c:7-72).
 * _autocorr_: x [batch][n] -> r [batch][order+1].  The sums are not the
 * reference's sequential ones (64 partial sums and a fixed tree per lag); their
 * order depends on n alone, never on the batch or the entry point.
 * _levinson_: r [batch][order+1] -> a [batch][order+1], err [batch], the
 * reference's recursion, bit-identical to it given the same r.  A row with
 * r[0] <= 0 (the silent frame, the reference's VV_DSP_ERROR_INTERNAL) gets
 * a = {1, 0, .., 0} and err = 0; its neighbours are unaffected.
 * _lpc_: the two in one launch, bit-identical to them in sequence.
 * Orders <= 32 on rows of n <= 4096 take the wave kernel, any other order < n
 * a generic one (vvhip_debug_get("STAT_LPC_WAVE") / ("STAT_LPC_GENERIC")). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_autocorr_device(const vv_dsp_real* d_x, size_t n, size_t order, size_t batch,
                                                      vv_dsp_real* d_r, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_levinson_device(const vv_dsp_real* d_r, size_t order, size_t batch,
                                                      vv_dsp_real* d_a, vv_dsp_real* d_err, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpc_device(const vv_dsp_real* d_x, size_t n, size_t order, size_t batch,
                                                 vv_dsp_real* d_a, vv_dsp_real* d_err, void* stream);
/* Signal -> framed, windowed LPC in one kernel, no frame rows in HBM: d_signal
 * [nch][n] (ch_stride floats apart) -> a [nch][frames][order+1] and err
 * [nch][frames] (channels a_ch_stride / err_ch_stride floats apart), frames =
 * vv_dsp_get_num_frames(n, frame_len, hop_len, center).  Frame contents are
 * vv_dsp_fetch_frames_device's (zero padding, reflection when center, times
 * d_window when not NULL), and the result is bit-identical to that call
 * followed by vv_dsp_lpc_device.  Zero frames: OK, nothing written.
 * hop_len = 0, frame_len = 0 or order + 1 > frame_len: INVALID_SIZE. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpc_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                        size_t ch_stride, size_t frame_len, size_t hop_len, int center,
                                                        const vv_dsp_real* d_window, size_t order, vv_dsp_real* d_a,
                                                        size_t a_ch_stride, vv_dsp_real* d_err, size_t err_ch_stride,
                                                        void* stream);
/* a [batch][order+1] -> mag [batch][nfft] = g / |A(e^(j 2 pi k / nfft))|, g =
 * d_gain[row] (NULL: 1).  levinson_sign 0: A = 1 - sum a[m] z^-m, vv_dsp_lpspec's
 * (the reference's) convention; nonzero: A = 1 + sum a[m] z^-m, so rows of
 * vv_dsp_levinson_device / vv_dsp_lpc_device feed it directly.  The phase of
 * term (m, k) is exact: (m k) mod nfft as an integer. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpspec_device(const vv_dsp_real* d_a, size_t order, const vv_dsp_real* d_gain,
                                                    size_t nfft, size_t batch, int levinson_sign, vv_dsp_real* d_mag,
                                                    void* stream);
/* Line spectral frequencies, reflection coefficients and formants of LPC rows
 * (vv_dsp/envelope/lsf.h and vv_dsp/features/formant.h, which state the
 * definitions and the order of the checks).
 * _lpc_to_lsf_: d_a [batch] rows a_pitch floats apart (a_pitch >= order + 1, so
 * rows of vv_dsp_lpc_frames_device feed it directly) -> d_lsf and d_rc packed
 * [batch][order], d_flags [batch] int32 (VV_DSP_LSF_STABLE | _COMPLETE); any
 * output may be NULL, not all.  _lsf_to_lpc_: d_lsf packed [batch][order] -> d_a
 * rows a_pitch floats apart.
 * _lpc_formants_: d_a as above -> the planes of vv_dsp_formant_out, packed by row.
 * _lsf_frames_ / _formants_frames_: the signal arguments of
 * vv_dsp_lpc_frames_device; the LPC rows go to stream-ordered scratch in groups
 * of channels and are converted from there, bit-identical to
 * vv_dsp_lpc_frames_device followed by the row call.  lsf and rc are
 * [nch][frames][order], flags and err [nch][frames]; the formant planes are
 * [nch * frames] rows, channel-major; each may be NULL, not all.  Zero frames: OK,
 * nothing written.  Zero rows: OK, nothing launched.
 * vvhip_debug_get("STAT_LSF") / ("STAT_FORMANT") count the launches. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpc_to_lsf_device(const vv_dsp_real* d_a, size_t order, size_t batch,
                                                        size_t a_pitch, vv_dsp_real* d_lsf, vv_dsp_real* d_rc,
                                                        int32_t* d_flags, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lsf_to_lpc_device(const vv_dsp_real* d_lsf, size_t order, size_t batch,
                                                        vv_dsp_real* d_a, size_t a_pitch, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lsf_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                        size_t ch_stride, size_t frame_len, size_t hop_len, int center,
                                                        const vv_dsp_real* d_window, size_t order, vv_dsp_real* d_lsf,
                                                        vv_dsp_real* d_rc, int32_t* d_flags, vv_dsp_real* d_err,
                                                        void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpc_formants_device(const vv_dsp_real* d_a, size_t order, size_t batch,
                                                          size_t a_pitch, const vv_dsp_formant_params* params,
                                                          const vv_dsp_formant_out* out, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_formants_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                             size_t ch_stride, size_t frame_len, size_t hop_len,
                                                             int center, const vv_dsp_real* d_window, size_t order,
                                                             const vv_dsp_formant_params* params,
                                                             const vv_dsp_formant_out* out, void* stream);
/* LPC rows applied to a signal (vv_dsp/envelope/lpc_filter.h, which states the
 * arithmetic, the row that governs a sample and the order of the checks).
 * _lpc_residual_ / _lpc_synth_: signal [nch][n], channels x_stride floats apart,
 * -> [nch][n], channels y_stride apart.  d_a: `frames` rows per channel, a_pitch
 * >= order + 1 floats apart (rows of vv_dsp_lpc_frames_device and
 * vv_dsp_lsf_to_lpc_device feed it directly), channels a_ch_stride apart;
 * a_ch_stride == 0: one envelope for every channel.  d_gain: NULL (1), or
 * [frames] floats per channel, channels g_ch_stride apart, 0 likewise.  d_state:
 * NULL (zeros in, nothing out) or doubles [nch][order], read and overwritten.
 * Synthesis may run in place (d_y == d_e); the residual may not.  Rows of n <=
 * VV_DSP_LPC_SYNTH_EXACT_MAX are synthesised as one recursion, longer ones in
 * chunks (knob LPC_SYNTH_CHUNK: 0 never chunks, k > 0 forces chunks of k).
 * vvhip_debug_get("STAT_LPC_RESIDUAL") / ("STAT_LPC_SYNTH_EXACT") /
 * ("STAT_LPC_SYNTH_CHUNKED") count the calls of each route.
 * _lpc_residual_frames_: the signal arguments of vv_dsp_lpc_frames_device; the
 * LPC rows go to d_a / d_err as that call lays them out, or, where one is NULL,
 * to stream-ordered scratch in groups of channels; the residual of the signal
 * through its own rows goes to d_e, with seg_len = hop_len and offset =
 * hop_len / 2 when center, else hop_len / 2 - frame_len / 2 (the frame whose
 * centre is nearest governs), bit-identical to vv_dsp_lpc_frames_device followed
 * by vv_dsp_lpc_residual_device.  Zero frames: OK, nothing written. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpc_residual_device(const vv_dsp_real* d_x, size_t n, size_t nch,
                                                          size_t x_stride, const vv_dsp_real* d_a, size_t order,
                                                          size_t frames, size_t a_pitch, size_t a_ch_stride,
                                                          const vv_dsp_real* d_gain, size_t g_ch_stride,
                                                          size_t seg_len, long long offset, double* d_state,
                                                          vv_dsp_real* d_e, size_t e_stride, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpc_synth_device(const vv_dsp_real* d_e, size_t n, size_t nch, size_t e_stride,
                                                       const vv_dsp_real* d_a, size_t order, size_t frames,
                                                       size_t a_pitch, size_t a_ch_stride, const vv_dsp_real* d_gain,
                                                       size_t g_ch_stride, size_t seg_len, long long offset,
                                                       double* d_state, vv_dsp_real* d_y, size_t y_stride,
                                                       void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_lpc_residual_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                                 size_t ch_stride, size_t frame_len, size_t hop_len,
                                                                 int center, const vv_dsp_real* d_window, size_t order,
                                                                 vv_dsp_real* d_a, size_t a_ch_stride,
                                                                 vv_dsp_real* d_err, size_t err_ch_stride,
                                                                 vv_dsp_real* d_e, size_t e_stride, void* stream);
/* Array statistics (vv_dsp/core/stats.h, which states the numerics: the exact
 * class bit-identical to the reference, the f64 class within 1 ulp of it, one
 * summation order whatever the batch, stride, outputs or entry point).
 * vv_dsp_stats_out: one pointer per output, NULL = not wanted, else one value
 * per row; zero_crossings, argmin and argmax are uint32.
 * _stats_: `batch` rows of n samples, row_stride floats apart.
 * _stats_frames_: d_signal [nch][n] (ch_stride floats apart) -> planes
 * [nch][frames] (channels out_ch_stride values apart), frames =
 * vv_dsp_get_num_frames(n, frame_len, hop_len, center), the frames exactly those
 * of vv_dsp_fetch_frames_device (zero padding, reflection when center, times
 * d_window when not NULL); bit-identical to that call followed by
 * vv_dsp_stats_device, without the frame rows in HBM.
 * One launch reads each row or frame once from HBM (the second pass of var /
 * skewness / kurtosis and the frames' overlap come from cache) and writes every
 * requested output.  No output requested: OK, nothing launched.  A requested
 * output whose size rule fails (var n < 2, skewness n < 3, kurtosis n < 4, n =
 * the row or frame length), hop_len == 0 or frame_len == 0: INVALID_SIZE,
 * nothing written.  Zero frames or rows: OK, nothing written.  n (frame_len)
 * must be below 2^32.
 * Rows or frames of up to 16384 samples take the wave kernel (one wave per
 * row); longer ones the long route (one wave per chunk of 4096 samples, the
 * chunks' results combined per row in chunk order through scratch).  Knob
 * STATS_LONG = 1 forces the long route; both give the same bits
 * (vvhip_debug_get("STAT_STATS_WAVE") / ("STAT_STATS_LONG") count which ran).
 * A mask without sum, mean, var, skewness and kurtosis runs a kernel with no
 * f64 sum and no second pass. */
typedef struct vv_dsp_stats_out {   /* each NULL (not wanted) or one value per row */
    vv_dsp_real *sum, *mean, *var, *rms, *min, *max, *crest, *skewness, *kurtosis;
    uint32_t *zero_crossings, *argmin, *argmax;
} vv_dsp_stats_out;
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stats_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t row_stride,
                                                   const vv_dsp_stats_out* out, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stats_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                          size_t ch_stride, size_t frame_len, size_t hop_len,
                                                          int center, const vv_dsp_real* d_window,
                                                          const vv_dsp_stats_out* out, size_t out_ch_stride,
                                                          void* stream);
/* Lagged correlations of `batch` contiguous rows: x [batch][n] -> r [batch][r_len]
 * (vv_dsp_autocorrelation), x [batch][nx] and y [batch][ny] -> r [batch][r_len]
 * (vv_dsp_cross_correlation).  Direct f64 sums, one workgroup per (row, lag),
 * rounded once; lags with no overlapping sample give 0.  n, nx, ny < 2^32 and
 * batch * r_len < 2^31. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_autocorrelation_device(const vv_dsp_real* d_x, size_t n, size_t batch,
                                                             size_t r_len, int biased, vv_dsp_real* d_r, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_cross_correlation_device(const vv_dsp_real* d_x, size_t nx,
                                                               const vv_dsp_real* d_y, size_t ny, size_t batch,
                                                               size_t r_len, vv_dsp_real* d_r, void* stream);
/* Per-frame pitch by YIN (vv_dsp/features/pitch.h, which states the algorithm,
 * its numerics and the argument checks, made in its order before any device work).
 * vv_dsp_pitch_out: one pointer per output, NULL = not wanted, else one value
 * per row: f0 in Hz (0 = unvoiced), aperiodicity = d' at the chosen lag, lag
 * (uint32), and cmnd, the curve d'(0 .. tau_max), tau_max + 1 floats per row
 * (vv_dsp_pitch_lag_range gives tau_max).  No output requested: OK, nothing
 * launched.  A value depends on the row's samples and the parameters alone.
 * _pitch_: `batch` rows of n samples, row_stride floats apart; row r's curve
 * at cmnd + r * cmnd_row_stride (>= tau_max + 1).
 * _pitch_frames_: d_signal [nch][n] (ch_stride floats apart) -> planes
 * [nch][frames] (channels out_ch_stride values apart) and curves
 * [nch][frames][tau_max + 1] (channels cmnd_ch_stride floats apart), frames =
 * vv_dsp_get_num_frames(n, frame_len, hop_len, center), the frames exactly those
 * of vv_dsp_fetch_frames_device (zero padding, reflection when center, times
 * d_window when not NULL); bit-identical to that call followed by
 * vv_dsp_pitch_device, without the frame rows in HBM.  Zero frames or rows: OK,
 * nothing written.  hop_len == 0: INVALID_SIZE, as is a stride shorter than
 * what it steps over.
 * One kernel, one wave per row, the row in LDS
 * (vvhip_debug_get("STAT_PITCH_WAVE") counts its launches). */
typedef struct vv_dsp_pitch_out {   /* each NULL (not wanted) or per row */
    vv_dsp_real *f0, *aperiodicity;
    uint32_t* lag;
    vv_dsp_real* cmnd;
} vv_dsp_pitch_out;
VV_DSP_NODISCARD vv_dsp_status vv_dsp_pitch_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t row_stride,
                                                   const vv_dsp_pitch_params* params, const vv_dsp_pitch_out* out,
                                                   size_t cmnd_row_stride, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_pitch_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                          size_t ch_stride, size_t frame_len, size_t hop_len,
                                                          int center, const vv_dsp_real* d_window,
                                                          const vv_dsp_pitch_params* params,
                                                          const vv_dsp_pitch_out* out, size_t out_ch_stride,
                                                          size_t cmnd_ch_stride, void* stream);
/* One f0 contour per channel from the YIN curves of its frames
 * (vv_dsp/features/pitch_track.h, which states the path's definition, its
 * numerics and the argument checks, made in its order before any device work).
 * _pitch_track_: d_curves [nch][frames][row_stride] (row_stride >= tau_max + 1,
 * channels cmnd_ch_stride floats apart: the cmnd plane of
 * vv_dsp_pitch_frames_device) -> planes [nch][frames] (channels out_ch_stride
 * values apart) and cost [nch]; vv_dsp_pitch_track_out: one pointer per output,
 * NULL = not wanted.
 * _pitch_track_frames_: d_signal [nch][n] -> the same planes, bit-identical to
 * vv_dsp_pitch_frames_device (cmnd) followed by vv_dsp_pitch_track_device: the
 * curves go to scratch in groups of channels, at most 2 GiB of curves a group
 * (at least one channel), and no value depends on the grouping.  track->tau_max
 * must not exceed the curves' last lag (vv_dsp_pitch_lag_range's tau_max), else
 * INVALID_SIZE; vv_dsp_pitch_track_params_default gives matching parameters.
 * The tracker's own scratch is one byte per state and frame plus four bytes per
 * frame, in channel groups of at most 4 GiB.
 * vvhip_debug_get("STAT_PITCH_TRACK") counts the tracker's launches. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_pitch_track_device(const vv_dsp_real* d_curves, size_t frames, size_t nch,
                                                         size_t row_stride, size_t cmnd_ch_stride,
                                                         const vv_dsp_pitch_track_params* params,
                                                         const vv_dsp_pitch_track_out* out, size_t out_ch_stride,
                                                         void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_pitch_track_frames_device(const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                                size_t ch_stride, size_t frame_len, size_t hop_len,
                                                                int center, const vv_dsp_real* d_window,
                                                                const vv_dsp_pitch_params* pitch,
                                                                const vv_dsp_pitch_track_params* track,
                                                                const vv_dsp_pitch_track_out* out,
                                                                size_t out_ch_stride, void* stream);
/* Per-frame spectral shape descriptors of power rows
 * (vv_dsp/features/spectral_shape.h, which states every value's definition, its
 * numerics and the argument checks, made in its order before any device work).
 * vv_dsp_spectral_shape_out: one pointer per output, NULL = not wanted, else one
 * value per row.  No output requested: OK, nothing launched; zero rows: OK,
 * nothing written.  One kernel, one wave per run of rows, all outputs of a row
 * from one read of it (vvhip_debug_get("STAT_SHAPE_WAVE") counts its launches,
 * "STAT_SHAPE_VEC16" those that load 16 bytes at a time: a 16-byte aligned
 * base and a pitch that is a multiple of 4; knob SHAPE_DWORD = 1 forces 4-byte
 * loads, with the same bits).
 * _spectral_shape_: `rows` rows of n_fft/2 + 1 powers, row_pitch floats apart
 * (the packed layout, n_fft/2 + 1, or vv_dsp_stft_power_pitched_device's, e.g.
 * 544 for n_fft 1024); rows_per_group is the number of frames per channel: row
 * r starts a group (flux 0) when r % rows_per_group == 0; 0 means one group.
 * _stft_spectral_shape_: d_signal [nch][n] (ch_stride floats apart) -> planes
 * [nch][frames], channels out_ch_stride (>= frames, else INVALID_SIZE) values
 * apart: vv_dsp_stft_power_pitched_device (pitch: n_fft/2 + 1 rounded up to a
 * whole number of 128 B lines) into stream-ordered scratch, then
 * _spectral_shape_ with one group per channel -- the values of the two public
 * calls in sequence, bit for bit.  The scratch holds every row: 4 nch frames
 * pitch bytes (2.6 GB for 32 channels x 10 min at 16 kHz, n_fft 1024, hop 256),
 * allocated and freed on the stream.  params->n_fft must equal the handle's
 * fft_size (INVALID_SIZE). */
typedef struct vv_dsp_spectral_shape_out {   /* each NULL (not wanted) or one value per row */
    vv_dsp_real *energy, *centroid, *spread, *skewness, *kurtosis, *flatness, *rolloff, *flux, *crest;
    uint32_t* peak_bin;
} vv_dsp_spectral_shape_out;
VV_DSP_NODISCARD vv_dsp_status vv_dsp_spectral_shape_device(const vv_dsp_real* d_power, size_t rows, size_t row_pitch,
                                                            size_t rows_per_group,
                                                            const vv_dsp_spectral_shape_params* params,
                                                            const vv_dsp_spectral_shape_out* out, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_spectral_shape_device(vv_dsp_stft* h,
                                                                 const vv_dsp_spectral_shape_params* params,
                                                                 const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                                 size_t ch_stride, const vv_dsp_spectral_shape_out* out,
                                                                 size_t out_ch_stride, void* stream,
                                                                 size_t* out_frames);
/* Phase vocoder: time-stretch of STFT rows (vv_dsp/spectral/phase_vocoder.h, which
 * states every value's definition, the order of the phase sum, and the argument
 * checks, made in its order before any device work).  d_spec [nch][T][n_fft]
 * complex rows, channels spec_ch_stride vv_dsp_cpx apart (>= T n_fft), only bins
 * 0 .. n_fft/2 read -> d_out [nch][m][n_fft], channels out_ch_stride vv_dsp_cpx
 * apart (>= m n_fft), every bin of rows 0 .. m - 1 written and nothing else.
 * _uniform_: output row j at start + j step; _device: at d_pos[j], m floats on the
 * device shared by all channels.  Equal positions give equal bits.  Three
 * launches: the segments' phase totals, their scan, the rows
 * (vvhip_debug_get("STAT_PVOC_ROWS") counts the calls that launched them);
 * stream-ordered scratch of 8 nch (n_fft/2 + 1) (segments + 1) bytes.  Knob
 * PVOC_PLANE = 1 (for timing; the same bits): a fourth launch stores the rows'
 * phases in 8 nch T (n_fft/2 + 1) more bytes of scratch and the walks read them
 * instead of calling atan2 a second time. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_phase_vocoder_uniform_device(const vv_dsp_cpx* d_spec, size_t T, size_t n_fft,
                                                                   size_t nch, size_t spec_ch_stride, double start,
                                                                   double step, size_t m, vv_dsp_cpx* d_out,
                                                                   size_t out_ch_stride, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_phase_vocoder_device(const vv_dsp_cpx* d_spec, size_t T, size_t n_fft, size_t nch,
                                                           size_t spec_ch_stride, const vv_dsp_real* d_pos, size_t m,
                                                           vv_dsp_cpx* d_out, size_t out_ch_stride, void* stream);
/* Time-stretch, signal to signal: d_signal [nch][n] (ch_stride floats apart) ->
 * d_out [nch][out_len] (out_ch_stride floats apart, >= out_len), a signal `rate`
 * times as fast at the same pitch (rate 0.5: twice as long).  With T the handle's
 * frame count of n samples, m the number of j >= 0 with (double)j rate < (double)T
 * and out_len = (m - 1) hop + fft_size: vv_dsp_stft_spectrum_device, the vocoder at
 * start 0 and step rate, vv_dsp_stft_reconstruct_device of each channel's m rows
 * into zeroed out and norm, then y[i] = norm[i] > VV_DSP_PVOC_NORM_FLOOR ?
 * out[i] / norm[i] : 0 -- the values of the public calls in sequence, bit for bit.
 * The rows live in stream-ordered scratch, a group of channels at a time (as
 * many as fit 1 GiB, at least one; knob PVOC_GROUP = k: k channels per group; the
 * result does not depend on it).  Checks in this order: NULL handle, signal or
 * out; fft_size < 2, ch_stride < n or out_ch_stride < out_len -- INVALID_SIZE; a
 * rate that is not finite or <= 0 -- OUT_OF_RANGE; the vocoder's limits --
 * UNSUPPORTED.  out_len depends on the rate, so out_ch_stride is checked for a
 * valid rate only: a bad rate with a short out_ch_stride gives OUT_OF_RANGE.
 * ch_stride is checked for nch > 1 only, as the neighbouring STFT calls check
 * theirs (one channel has no stride to step over); out_ch_stride, like the
 * strides of vv_dsp_phase_vocoder_*_device, is checked for one channel too.  *out_len (may be NULL) is set once every check has passed.
 * _length: m and out_len for n samples (either pointer may be NULL), to size d_out. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_time_stretch_length(const vv_dsp_stft* h, size_t n, double rate,
                                                               size_t* out_rows, size_t* out_len);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_time_stretch_device(vv_dsp_stft* h, const vv_dsp_real* d_signal, size_t n,
                                                               size_t nch, size_t ch_stride, double rate,
                                                               vv_dsp_real* d_out, size_t out_ch_stride, void* stream,
                                                               size_t* out_len);
/* Running median of `batch` rows of n samples, x_stride / y_stride floats apart
 * (vv_dsp/filter/median.h, which states the order, the boundary modes and the
 * argument checks, made in its order before any device work).  One launch, 256
 * positions of a row per block: the tile and its halo are turned into keys in
 * LDS with the boundary mode resolved, then every lane selects rank h of its
 * window by counting (window_length < 33) or bit by bit (knob MEDIAN_SELECT = 1 /
 * 2 forces either, with the same bits).  The floats between n and a stride are
 * never read or written; a row's output never depends on the batch, the strides
 * or the entry point.  d_y must not overlap d_x (not checked).  batch == 0: OK. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_medfilt_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t x_stride,
                                                     int window_length, vv_dsp_medfilt_mode mode, vv_dsp_real* d_y,
                                                     size_t y_stride, void* stream);
/* Harmonic-percussive separation (vv_dsp/spectral/hpss.h, which states every
 * value's definition and the argument checks, made in its order before any
 * device work).
 * _hpss_: `rows` rows of n_fft/2 + 1 powers, row_pitch floats apart, in groups of
 * rows_per_group rows (0: one group; the last may be short) -> the planes of
 * `out` that are not NULL, [rows][out_pitch], the pads past bin n_fft/2 neither
 * read nor written.  Launches: the time median (reads the rows, writes H) when
 * harm or a mask is wanted; the frequency median (reads the rows, and H where a
 * mask is wanted; writes perc and the masks that are wanted) when perc or a mask
 * is wanted.  Scratch, allocated and freed on the stream: 4 rows (n_fft/2 + 1)
 * bytes for H when a mask is wanted and harm is not, else none.
 * _stft_hpss_: d_signal [nch][n] (ch_stride floats apart) -> d_out_harm and
 * d_out_perc [nch][out_len] (out_ch_stride floats apart; either may be NULL),
 * out_len = (T - 1) hop + fft_size with T the handle's frame count of n samples
 * (a signal shorter than one frame is one zero-padded frame, as everywhere in the
 * STFT): vv_dsp_stft_power_device rows; vv_dsp_hpss_device masks, one group per
 * channel; vv_dsp_stft_spectrum_device rows whose bin k has its real and its
 * imaginary part each multiplied in float by mask[k] (bin n_fft - k by the same
 * mask); vv_dsp_stft_reconstruct_device of each channel's rows into zeroed out and
 * norm; y[i] = norm[i] > VV_DSP_PVOC_NORM_FLOOR ? out[i] / norm[i] : 0 -- the
 * values of the public calls in sequence, bit for bit.  The rows live in
 * stream-ordered scratch, a group of channels at a time (as many as fit 1 GiB, at
 * least one; knob HPSS_GROUP = k: k channels per group; the result does not depend
 * on it).  Checks in this order, as vv_dsp_stft_time_stretch_device orders its
 * own: NULL handle, params or signal, or both outputs NULL; fft_size < 2,
 * params->n_fft != fft_size, ch_stride < n (for nch > 1 only) or out_ch_stride <
 * out_len (for one channel too) -- INVALID_SIZE; then checks 3 and 4 of hpss.h.
 * *out_len (may be NULL) is set once every check has passed; nch == 0: OK. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_hpss_device(const vv_dsp_real* d_power, size_t rows, size_t row_pitch,
                                                  size_t rows_per_group, const vv_dsp_hpss_params* params,
                                                  const vv_dsp_hpss_out* out, size_t out_pitch, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_hpss_device(vv_dsp_stft* h, const vv_dsp_hpss_params* params,
                                                       const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                       size_t ch_stride, vv_dsp_real* d_out_harm,
                                                       vv_dsp_real* d_out_perc, size_t out_ch_stride, void* stream,
                                                       size_t* out_len);
/* Spectral noise suppression (vv_dsp/spectral/denoise.h, which states every
 * value's definition and the argument checks, made in its order before any
 * device work).
 * _denoise_: `rows` rows of n_fft/2 + 1 powers, row_pitch floats apart, in groups
 * of rows_per_group rows (0: one group; the last may be short) -> the planes of
 * `out` that are not NULL, [rows][out_pitch], the pads past bin n_fft/2 neither
 * read nor written.  One launch: a block walks a segment of a group's rows for 64
 * consecutive bins with the smoothed halo of the segment in LDS; no scratch.
 * Knobs DENOISE_SEGMENT = L (the segment length) and DENOISE_MIN = 1 / 2 (the
 * direct / the blockwise minimum) change no value.
 * _stft_denoise_: d_signal [nch][n] (ch_stride floats apart) -> d_out
 * [nch][out_len] (out_ch_stride floats apart), out_len = (T - 1) hop + fft_size
 * with T the handle's frame count of n samples (a signal shorter than one frame
 * is one zero-padded frame, as everywhere in the STFT):
 * vv_dsp_stft_power_device rows; vv_dsp_denoise_device gain, one group per
 * channel; vv_dsp_stft_spectrum_device rows whose bin k has its real and its
 * imaginary part each multiplied in float by gain[k] (bin n_fft - k by the same
 * gain); vv_dsp_stft_reconstruct_device of each channel's rows into zeroed out and
 * norm; y[i] = norm[i] > VV_DSP_PVOC_NORM_FLOOR ? out[i] / norm[i] : 0 -- the
 * values of the public calls in sequence, bit for bit.  The rows live in
 * stream-ordered scratch, a group of channels at a time (as many as fit 1 GiB, at
 * least one; knob DENOISE_GROUP = k: k channels per group; the result does not
 * depend on it).  Checks in this order, as vv_dsp_stft_hpss_device orders its
 * own: NULL handle, params, signal or output; fft_size < 2, params->n_fft !=
 * fft_size, ch_stride < n (for nch > 1 only) or out_ch_stride < out_len (for one
 * channel too) -- INVALID_SIZE; then checks 3 and 4 of denoise.h.  *out_len (may
 * be NULL) is set once every check has passed; nch == 0: OK. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_denoise_device(const vv_dsp_real* d_power, size_t rows, size_t row_pitch,
                                                     size_t rows_per_group, const vv_dsp_denoise_params* params,
                                                     const vv_dsp_denoise_out* out, size_t out_pitch, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_stft_denoise_device(vv_dsp_stft* h, const vv_dsp_denoise_params* params,
                                                          const vv_dsp_real* d_signal, size_t n, size_t nch,
                                                          size_t ch_stride, vv_dsp_real* d_out, size_t out_ch_stride,
                                                          void* stream, size_t* out_len);
/* Biquad cascade on `batch` rows of n samples, x_stride / y_stride floats apart
 * (vv_dsp/filter/iir.h, iir.c:21-43).  d_coef [num_stages][5] = b0 b1 b2 a1 a2
 * per stage, one cascade for every row.  d_state [batch][num_stages][2] = z1 z2
 * per row and stage, read as the incoming state and overwritten with the final
 * one; NULL: zero state in, none written.  d_y == d_x is allowed.
 * Rows of n <= 8192 run as one recurrence, bit-identical to the reference,
 * states included.  Longer rows are cut into chunks of 1024 samples: every
 * chunk is walked from zero state, the chunk-boundary states are propagated
 * per row in f64 through the cascade's 1024-step transition matrix, and every
 * chunk is walked again from its true incoming state (rounded to float).  The
 * outputs then differ from the reference's by rounding of the same size as its
 * own error against exact arithmetic.  A row's output depends on that row, the
 * cascade, its state and n alone.  After a NaN input the reference keeps finite
 * states in the stages ahead of the poisoned one; on chunked rows every state
 * is NaN from the next chunk boundary on (the outputs are NaN either way).
 * Knob IIR_CHUNK: 0 never chunks, k > 0 forces chunks of k samples
 * (vvhip_debug_get("STAT_IIR_EXACT") / ("STAT_IIR_CHUNKED") count which ran). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_iir_apply_device(const vv_dsp_real* d_coef, size_t num_stages,
                                                       vv_dsp_real* d_state, const vv_dsp_real* d_x, vv_dsp_real* d_y,
                                                       size_t n, size_t batch, size_t x_stride, size_t y_stride,
                                                       void* stream);
/* Savitzky-Golay (vv_dsp/filter/savgol.h).  _coeffs: the window h[window_length]
 * the filter convolves with, host setup in f64 with the reference's operations
 * (savgol.c:28-162), bit-identical to its coefficients; needs no GPU.
 * _device: `batch` rows of n samples, x_stride / y_stride floats apart; every
 * output is the f64 sum in window order, rounded once: bit-identical to the
 * reference.  d_y == d_x is allowed (the rows are staged).  The thread's NaN
 * policy applies to the samples as read and to the outputs as written; under
 * the ERROR policy the call waits for the stream and returns
 * VV_DSP_ERROR_NAN_INF when either met a NaN or Inf (d_y is then unspecified). */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_savgol_coeffs(int window_length, int polyorder, int deriv, vv_dsp_real delta,
                                                    vv_dsp_real* h);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_savgol_device(const vv_dsp_real* d_x, size_t n, size_t batch, size_t x_stride,
                                                    int window_length, int polyorder, int deriv, vv_dsp_real delta,
                                                    vv_dsp_savgol_mode mode, vv_dsp_real* d_y, size_t y_stride,
                                                    void* stream);
/* Spectral utilities on `batch` contiguous rows of n (utils.c:5-73): fftshift
 * (inverse 0) / ifftshift (inverse 1) of float or complex rows (in place
 * allowed); phase wrap of `count` floats; phase unwrap of each row. */
VV_DSP_NODISCARD vv_dsp_status vv_dsp_fftshift_device(const void* d_in, void* d_out, size_t n, size_t batch,
                                                      int is_complex, int inverse, void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_phase_wrap_device(const vv_dsp_real* d_in, vv_dsp_real* d_out, size_t count,
                                                        void* stream);
VV_DSP_NODISCARD vv_dsp_status vv_dsp_phase_unwrap_device(const vv_dsp_real* d_in, vv_dsp_real* d_out, size_t n,
                                                          size_t batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
