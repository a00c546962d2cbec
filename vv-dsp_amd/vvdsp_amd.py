"""ctypes binding of libvvdsp_amd.so's batched / device-pointer API (vv_dsp_amd.h).

Device memory and streams come from PyTorch (plumbing only): tensors are
passed as raw HBM pointers, streams as hipStream_t handles.  All compute runs
in the library's hand-written gfx950 kernels; there is no Python or CPU
fallback -- loading fails loudly when the library or a device is missing.

`import torch` happens before the library is loaded so that one HIP runtime
(torch's libamdhip64.so.7) serves both.
"""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VVDSP_AMD_LIB") or os.path.join(HERE, "lib", "libvvdsp_amd.so")   # override: A/B builds

OK = 0
C2C, R2C, C2R = 0, 1, 2
FWD, BWD = 1, -1
WIN_BOXCAR, WIN_HANN, WIN_HAMMING = 0, 1, 2

_vp = C.c_void_p
_sz = C.c_size_t
_lib = None


class StftParams(C.Structure):
    _fields_ = [("fft_size", C.c_size_t), ("hop_size", C.c_size_t), ("window", C.c_int)]


class StatsOut(C.Structure):
    """vv_dsp_stats_out: one device pointer per output, NULL = not wanted"""
    _fields_ = [(name, C.c_void_p) for name in ("sum", "mean", "var", "rms", "min", "max", "crest", "skewness",
                                                 "kurtosis", "zero_crossings", "argmin", "argmax")]


STATS_NAMES = tuple(name for name, _ in StatsOut._fields_)
STATS_COUNTS = ("zero_crossings", "argmin", "argmax")          # uint32 on the device, int32 tensors here
STATS_MIN_LEN = {"var": 2, "skewness": 3, "kurtosis": 4}       # the reference's size rules


class PitchParams(C.Structure):
    """vv_dsp_pitch_params (vv_dsp/features/pitch.h)"""
    _fields_ = [("sample_rate", C.c_float), ("fmin", C.c_float), ("fmax", C.c_float), ("threshold", C.c_float)]


class PitchOut(C.Structure):
    """vv_dsp_pitch_out: one device pointer per output, NULL = not wanted"""
    _fields_ = [(name, C.c_void_p) for name in ("f0", "aperiodicity", "lag", "cmnd")]


PITCH_NAMES = tuple(name for name, _ in PitchOut._fields_)


class PitchTrackParams(C.Structure):
    """vv_dsp_pitch_track_params (vv_dsp/features/pitch_track.h)"""
    _fields_ = [("sample_rate", C.c_float), ("tau_min", C.c_uint32), ("tau_max", C.c_uint32), ("lambda_", C.c_float),
                ("jump_cost", C.c_float), ("switch_cost", C.c_float), ("unvoiced_cost", C.c_float),
                ("max_step", C.c_uint32)]


class PitchTrackOut(C.Structure):
    """vv_dsp_pitch_track_out: one device pointer per output, NULL = not wanted"""
    _fields_ = [(name, C.c_void_p) for name in ("lag", "f0", "aperiodicity", "cost")]


TRACK_NAMES = tuple(name for name, _ in PitchTrackOut._fields_)


class FormantParams(C.Structure):
    """vv_dsp_formant_params (vv_dsp/features/formant.h)"""
    _fields_ = [("sample_rate", C.c_float), ("f_min", C.c_float), ("f_max", C.c_float), ("bw_max", C.c_float),
                ("n_formants", C.c_uint32)]


class FormantOut(C.Structure):
    """vv_dsp_formant_out: one device pointer per output, NULL = not wanted"""
    _fields_ = [(name, C.c_void_p) for name in ("freq", "bw", "count", "flags", "roots")]


FORMANT_NAMES = tuple(name for name, _ in FormantOut._fields_)
LSF_NAMES = ("lsf", "rc", "flags")
LSF_STABLE, LSF_COMPLETE = 1, 2          # bits of the lsf flags word
FORMANT_CONVERGED = 1                    # bit of the formant flags word
LSF_MAX_ORDER = 32
LPC_FILTER_MAX_ORDER = 32


class SpectralShapeParams(C.Structure):
    """vv_dsp_spectral_shape_params (vv_dsp/features/spectral_shape.h)"""
    _fields_ = [("n_fft", C.c_size_t), ("sample_rate", C.c_float), ("magnitude", C.c_int), ("k_min", C.c_size_t),
                ("k_max", C.c_size_t), ("rolloff", C.c_float), ("floor", C.c_float)]


class SpectralShapeOut(C.Structure):
    """vv_dsp_spectral_shape_out: one device pointer per output, NULL = not wanted"""
    _fields_ = [(name, C.c_void_p) for name in ("energy", "centroid", "spread", "skewness", "kurtosis", "flatness",
                                                 "rolloff", "flux", "crest", "peak_bin")]


SHAPE_NAMES = tuple(name for name, _ in SpectralShapeOut._fields_)

MEDFILT_REFLECT, MEDFILT_NEAREST, MEDFILT_ZERO = 0, 1, 2
HPSS_HARD, HPSS_SOFT, HPSS_WIENER = 0, 1, 2


class HpssParams(C.Structure):
    """vv_dsp_hpss_params (vv_dsp/spectral/hpss.h)"""
    _fields_ = [("n_fft", C.c_size_t), ("magnitude", C.c_int), ("win_harm", C.c_int), ("win_perc", C.c_int),
                ("margin_harm", C.c_float), ("margin_perc", C.c_float), ("mask", C.c_int)]


class HpssOut(C.Structure):
    """vv_dsp_hpss_out: one device pointer per plane, NULL = not wanted"""
    _fields_ = [(name, C.c_void_p) for name in ("harm", "perc", "mask_harm", "mask_perc")]


HPSS_NAMES = tuple(name for name, _ in HpssOut._fields_)

DENOISE_GATE, DENOISE_WIENER, DENOISE_SUBTRACT = 0, 1, 2


class DenoiseParams(C.Structure):
    """vv_dsp_denoise_params (vv_dsp/spectral/denoise.h)"""
    _fields_ = [("n_fft", C.c_size_t), ("smooth_len", C.c_int), ("back", C.c_int), ("ahead", C.c_int),
                ("bias", C.c_float), ("floor", C.c_float), ("mode", C.c_int)]


class DenoiseOut(C.Structure):
    """vv_dsp_denoise_out: one device pointer per plane, NULL = not wanted"""
    _fields_ = [(name, C.c_void_p) for name in ("smooth", "noise", "gain")]


DENOISE_NAMES = tuple(name for name, _ in DenoiseOut._fields_)


class VvError(RuntimeError):
    pass


def lib():
    """Load (once) and return the CDLL; raise if the native library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VvError(f"native library missing: {LIB_PATH} (run `make -C vv-dsp_amd`)")
    L = C.CDLL(LIB_PATH)
    L.vvhip_available.restype = C.c_int
    L.vvhip_last_error.restype = C.c_char_p
    L.vvhip_version.restype = C.c_char_p
    L.vvhip_debug_set.argtypes = [C.c_char_p, C.c_longlong]
    L.vvhip_debug_clear.argtypes = [C.c_char_p]
    L.vvhip_debug_get.argtypes = [C.c_char_p]
    L.vvhip_debug_get.restype = C.c_longlong
    L.vv_dsp_fft_make_plan_many.argtypes = [_sz, C.c_int, C.c_int, _sz, C.POINTER(_vp)]
    L.vv_dsp_fft_execute_device.argtypes = [_vp, _vp, _vp, _vp]
    L.vv_dsp_fft_destroy.argtypes = [_vp]
    L.vv_dsp_stft_create.argtypes = [C.POINTER(StftParams), C.POINTER(_vp)]
    L.vv_dsp_stft_destroy.argtypes = [_vp]
    L.vv_dsp_stft_spectrogram_device.argtypes = [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, C.POINTER(_sz)]
    L.vv_dsp_stft_spectrum_device.argtypes = [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, C.POINTER(_sz)]
    L.vv_dsp_stft_power_device.argtypes = [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, C.POINTER(_sz)]
    L.vv_dsp_stft_power_pitched_device.argtypes = [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _sz, _vp, C.POINTER(_sz)]
    L.vv_dsp_mfcc_process_pitched_device.argtypes = [_vp, _vp, _sz, _sz, _vp, _vp]
    L.vv_dsp_log_mel_pitched_device.argtypes = [_vp, _vp, _sz, _sz, _vp, _vp]
    L.vv_dsp_stft_log_mel_device.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, C.POINTER(_sz)]
    L.vv_dsp_stft_mfcc_device.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _sz, _vp, C.POINTER(_sz)]
    L.vv_dsp_stft_frames_range_device.argtypes = [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp, _sz, C.c_int, _vp]
    L.vv_dsp_stft_process_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.vv_dsp_stft_reconstruct_device.argtypes = [_vp, _vp, _sz, _vp, _vp, _vp]
    L.vv_dsp_instantaneous_phase_device.argtypes = [_vp, _sz, _sz, _vp, _vp]
    L.vv_dsp_instantaneous_frequency_device.argtypes = [_vp, _sz, _sz, C.c_double, _vp, _vp]
    L.vv_dsp_fir_plan_create.argtypes = [_vp, _sz, C.POINTER(_vp)]
    L.vv_dsp_fir_plan_destroy.argtypes = [_vp]
    L.vv_dsp_fir_apply_fft_device.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp]
    L.vv_dsp_fir_apply_direct_device.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp]
    L.vv_dsp_filtfilt_fir_device.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp]
    L.vv_dsp_resampler_create.argtypes = [C.c_uint, C.c_uint]
    L.vv_dsp_resampler_create.restype = _vp
    L.vv_dsp_resampler_destroy.argtypes = [_vp]
    L.vv_dsp_resampler_destroy.restype = None
    L.vv_dsp_resampler_set_ratio.argtypes = [_vp, C.c_uint, C.c_uint]
    L.vv_dsp_resampler_set_quality.argtypes = [_vp, C.c_int, C.c_uint]
    L.vv_dsp_resampler_output_length.argtypes = [_vp, _sz]
    L.vv_dsp_resampler_output_length.restype = _sz
    L.vv_dsp_resampler_process_device.argtypes = [_vp, _vp, _sz, _sz, _sz, _vp, _sz, _sz, _vp, C.POINTER(_sz)]
    L.vvhip_resample_run_length.argtypes = [C.c_uint, C.c_uint, C.c_uint]
    L.vvhip_resample_run_length.restype = _sz
    L.vv_dsp_interpolate_device.argtypes = [_vp, _sz, _sz, _sz, _vp, _sz, _sz, C.c_int, _vp, _sz, _vp]
    L.vv_dsp_interpolate_uniform_device.argtypes = [_vp, _sz, _sz, _sz, C.c_double, C.c_double, _sz, C.c_int, _vp,
                                                    _sz, _vp]
    L.vv_dsp_interpolate_real_batch.argtypes = [_vp, _sz, _vp, _sz, C.c_int, _vp]
    L.vvhip_interp_run_length.argtypes = []
    L.vvhip_interp_run_length.restype = _sz
    L.vv_dsp_hilbert_analytic_device.argtypes = [_vp, _sz, _sz, _vp, _vp]
    L.vv_dsp_dct_make_plan.argtypes = [_sz, C.c_int, C.c_int, C.POINTER(_vp)]
    L.vv_dsp_dct_execute_device.argtypes = [_vp, _vp, _vp, _sz, _vp]
    L.vv_dsp_dct_destroy.argtypes = [_vp]
    L.vv_dsp_mfcc_init.argtypes = [_sz, _sz, _sz, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float,
                                   C.c_float, C.POINTER(_vp)]
    L.vv_dsp_mfcc_destroy.argtypes = [_vp]
    L.vv_dsp_mfcc_process_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.vv_dsp_log_mel_device.argtypes = [_vp, _vp, _sz, _vp, _vp]
    L.vv_dsp_czt_plan_create.argtypes = [_sz, _sz, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(_vp)]
    L.vv_dsp_czt_plan_destroy.argtypes = [_vp]
    L.vv_dsp_czt_execute_device.argtypes = [_vp, _vp, C.c_int, _sz, _vp, _vp]
    L.vv_dsp_dist_init_all.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(_vp)]
    L.vv_dsp_dist_init_loopback.argtypes = [C.c_int, C.c_int, C.POINTER(_vp)]
    L.vv_dsp_dist_from_comm.argtypes = [_vp, C.POINTER(_vp)]
    L.vv_dsp_dist_unique_id.argtypes = [C.c_char_p]
    L.vv_dsp_dist_init_rank.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(_vp)]
    L.vv_dsp_dist_comm_count.argtypes = [_vp, C.c_int, C.POINTER(C.c_int)]
    L.vv_dsp_dist_destroy.argtypes = [_vp]
    L.vv_dsp_dist_local_ranks.argtypes = [_vp]
    L.vv_dsp_dist_rank_info.argtypes = [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.vv_dsp_dist_stft.argtypes = [_vp, _vp, _vp, _sz, _sz, _sz, C.c_int, _vp, _vp, C.POINTER(_sz)]
    L.vv_dsp_dist_gather_rows.argtypes = [_vp, _vp, _sz, _sz, _sz, C.c_int, _vp, C.c_int, _vp]
    L.vv_dsp_dist_fft.argtypes = [_vp, _sz, C.c_int, C.c_int, _sz, _vp, _vp, _vp]
    L.vv_dsp_dist_fir_apply_fft.argtypes = [_vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp]
    L.vv_dsp_stft_get_sizes.argtypes = [_vp, C.POINTER(_sz), C.POINTER(_sz)]
    for f in ("cepstrum_real", "icepstrum_minphase", "minphase_from_cepstrum"):
        getattr(L, f"vv_dsp_{f}_device").argtypes = [_vp, _sz, _sz, _vp, _vp]
    L.vv_dsp_autocorr_device.argtypes = [_vp, _sz, _sz, _sz, _vp, _vp]
    L.vv_dsp_levinson_device.argtypes = [_vp, _sz, _sz, _vp, _vp, _vp]
    L.vv_dsp_lpc_device.argtypes = [_vp, _sz, _sz, _sz, _vp, _vp, _vp]
    L.vv_dsp_lpc_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _sz, _vp, _sz, _vp, _sz, _vp]
    L.vv_dsp_lpspec_device.argtypes = [_vp, _sz, _vp, _sz, _sz, C.c_int, _vp, _vp]
    L.vv_dsp_lpc_to_lsf_device.argtypes = [_vp, _sz, _sz, _sz, _vp, _vp, _vp, _vp]
    L.vv_dsp_lsf_to_lpc_device.argtypes = [_vp, _sz, _sz, _vp, _sz, _vp]
    L.vv_dsp_lsf_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _sz, _vp, _vp, _vp, _vp, _vp]
    L.vv_dsp_lpc_to_lsf.argtypes = [_vp, _sz, _vp, _vp, _vp]
    L.vv_dsp_lsf_to_lpc.argtypes = [_vp, _sz, _vp]
    for f in ("residual", "synth"):
        getattr(L, f"vv_dsp_lpc_{f}_device").argtypes = [_vp, _sz, _sz, _sz, _vp, _sz, _sz, _sz, _sz, _vp, _sz, _sz,
                                                         C.c_longlong, _vp, _vp, _sz, _vp]
        getattr(L, f"vv_dsp_lpc_{f}").argtypes = [_vp, _sz, _vp, _sz, _sz, _sz, C.c_longlong, _vp, _vp, _vp]
    L.vv_dsp_lpc_residual_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _sz, _vp, _sz, _vp,
                                                    _sz, _vp, _sz, _vp]
    L.vv_dsp_formant_params_default.argtypes = [C.c_float, C.POINTER(FormantParams)]
    L.vv_dsp_formant_start_points.argtypes = [_sz, _vp]
    L.vv_dsp_lpc_formants.argtypes = [_vp, _sz, C.POINTER(FormantParams), C.POINTER(FormantOut)]
    L.vv_dsp_lpc_formants_device.argtypes = [_vp, _sz, _sz, _sz, C.POINTER(FormantParams), C.POINTER(FormantOut), _vp]
    L.vv_dsp_formants_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, _sz,
                                                C.POINTER(FormantParams), C.POINTER(FormantOut), _vp]
    L.vv_dsp_stats_device.argtypes = [_vp, _sz, _sz, _sz, C.POINTER(StatsOut), _vp]
    L.vv_dsp_stats_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, C.POINTER(StatsOut), _sz, _vp]
    L.vv_dsp_autocorrelation_device.argtypes = [_vp, _sz, _sz, _sz, C.c_int, _vp, _vp]
    L.vv_dsp_cross_correlation_device.argtypes = [_vp, _sz, _vp, _sz, _sz, _sz, _vp, _vp]
    L.vv_dsp_pitch_lag_range.argtypes = [C.POINTER(PitchParams), _sz, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]
    L.vv_dsp_pitch_yin.argtypes = [_vp, _sz, C.POINTER(PitchParams), _vp, _vp]
    L.vv_dsp_pitch_device.argtypes = [_vp, _sz, _sz, _sz, C.POINTER(PitchParams), C.POINTER(PitchOut), _sz, _vp]
    L.vv_dsp_pitch_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, C.POINTER(PitchParams),
                                             C.POINTER(PitchOut), _sz, _sz, _vp]
    L.vv_dsp_pitch_track_params_default.argtypes = [C.POINTER(PitchParams), _sz, C.POINTER(PitchTrackParams)]
    L.vv_dsp_pitch_track.argtypes = [_vp, _sz, _sz, C.POINTER(PitchTrackParams), C.POINTER(PitchTrackOut)]
    L.vv_dsp_pitch_track_device.argtypes = [_vp, _sz, _sz, _sz, _sz, C.POINTER(PitchTrackParams),
                                            C.POINTER(PitchTrackOut), _sz, _vp]
    L.vv_dsp_pitch_track_frames_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp, C.POINTER(PitchParams),
                                                   C.POINTER(PitchTrackParams), C.POINTER(PitchTrackOut), _sz, _vp]
    L.vv_dsp_spectral_shape.argtypes = [_vp, _vp, C.POINTER(SpectralShapeParams), _vp]
    L.vv_dsp_spectral_shape_device.argtypes = [_vp, _sz, _sz, _sz, C.POINTER(SpectralShapeParams),
                                               C.POINTER(SpectralShapeOut), _vp]
    L.vv_dsp_stft_spectral_shape_device.argtypes = [_vp, C.POINTER(SpectralShapeParams), _vp, _sz, _sz, _sz,
                                                    C.POINTER(SpectralShapeOut), _sz, _vp, C.POINTER(_sz)]
    L.vv_dsp_phase_vocoder.argtypes = [_vp, _sz, _sz, C.c_double, C.c_double, _sz, _vp]
    L.vv_dsp_phase_vocoder_uniform_device.argtypes = [_vp, _sz, _sz, _sz, _sz, C.c_double, C.c_double, _sz, _vp, _sz,
                                                      _vp]
    L.vv_dsp_phase_vocoder_device.argtypes = [_vp, _sz, _sz, _sz, _sz, _vp, _sz, _vp, _sz, _vp]
    L.vv_dsp_stft_time_stretch_length.argtypes = [_vp, _sz, C.c_double, C.POINTER(_sz), C.POINTER(_sz)]
    L.vv_dsp_stft_time_stretch_device.argtypes = [_vp, _vp, _sz, _sz, _sz, C.c_double, _vp, _sz, _vp, C.POINTER(_sz)]
    L.vvhip_stft_stretch_length.argtypes = [_sz, _sz, _sz, C.c_double, C.POINTER(_sz), C.POINTER(_sz)]
    L.vv_dsp_medfilt.argtypes = [_vp, _sz, C.c_int, C.c_int, _vp]
    L.vv_dsp_medfilt_device.argtypes = [_vp, _sz, _sz, _sz, C.c_int, C.c_int, _vp, _sz, _vp]
    L.vv_dsp_hpss.argtypes = [_vp, _sz, C.POINTER(HpssParams), C.POINTER(HpssOut)]
    L.vv_dsp_hpss_device.argtypes = [_vp, _sz, _sz, _sz, C.POINTER(HpssParams), C.POINTER(HpssOut), _sz, _vp]
    L.vv_dsp_stft_hpss_device.argtypes = [_vp, C.POINTER(HpssParams), _vp, _sz, _sz, _sz, _vp, _vp, _sz, _vp,
                                          C.POINTER(_sz)]
    L.vv_dsp_denoise_params_default.argtypes = [_sz, C.POINTER(DenoiseParams)]
    L.vv_dsp_denoise.argtypes = [_vp, _sz, C.POINTER(DenoiseParams), C.POINTER(DenoiseOut)]
    L.vv_dsp_denoise_device.argtypes = [_vp, _sz, _sz, _sz, C.POINTER(DenoiseParams), C.POINTER(DenoiseOut), _sz, _vp]
    L.vv_dsp_stft_denoise_device.argtypes = [_vp, C.POINTER(DenoiseParams), _vp, _sz, _sz, _sz, _vp, _sz, _vp,
                                             C.POINTER(_sz)]
    L.vv_dsp_iir_apply_device.argtypes =[_vp, _sz, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp]
    L.vv_dsp_savgol_coeffs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, _vp]
    L.vv_dsp_savgol_device.argtypes = [_vp, _sz, _sz, _sz, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _vp, _sz,
                                       _vp]
    L.vv_dsp_get_num_frames.argtypes = [_sz, _sz, _sz, C.c_int]
    L.vv_dsp_get_num_frames.restype = _sz
    L.vvhip_fir_block_size.argtypes = [_vp, _sz]
    L.vvhip_fir_block_size.restype = _sz
    L.vv_dsp_amd_set_device.argtypes = [C.c_int]
    L.vv_dsp_amd_get_device.argtypes = [C.POINTER(C.c_int)]
    L.vv_dsp_shard_range.argtypes = [_sz, _sz, _sz, C.POINTER(_sz), C.POINTER(_sz)]
    L.vv_dsp_stft_channel_shard_device.argtypes = [_vp, C.c_int, _vp, _sz, _sz, _sz, C.c_int, _vp, _sz, _vp,
                                                   C.POINTER(_sz)]
    L.vv_dsp_spectrogram_pack_half_device.argtypes = [_vp, _sz, _sz, _vp, _vp]
    L.vv_dsp_spectrogram_unpack_half_device.argtypes = [_vp, _sz, _sz, _vp, _vp]
    _lib = L
    return L


def _check(st, what):
    if st != OK:
        msg = lib().vvhip_last_error().decode(errors="replace")
        raise VvError(f"{what} failed with status {st}: {msg}")


def _ptr(t):
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA(HIP) tensors"
    return C.c_void_p(t.data_ptr())


def _stream(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _expect(t, dtype, numel, what):
    """A kernel trusts the sizes it is given: check a tensor against the plan
    before its pointer goes down (too few elements would be read or written
    past the allocation)."""
    if t.dtype != dtype:
        raise VvError(f"{what}: dtype {t.dtype}, expected {dtype}")
    if t.numel() < numel:
        raise VvError(f"{what}: {t.numel()} elements, the plan needs {numel}")
    if not (t.is_cuda and t.is_contiguous()):
        raise VvError(f"{what}: must be a contiguous device tensor")


def debug_set(name, value):
    """Select a launcher alternative (csrc/hip/debug.hip knob, e.g. "STFT_DYN", 0)."""
    if lib().vvhip_debug_set(name.encode(), int(value)) != 0:
        raise VvError(f"unknown knob {name!r} or bad value {value!r}")


def debug_clear(name=None):
    """Back to the default path (None: every knob, and every path counter to 0)."""
    if lib().vvhip_debug_clear(None if name is None else name.encode()) != 0:
        raise VvError(f"unknown knob {name!r}")


def debug_get(name):
    """A knob's value (-1 = unset) or a path counter ("STAT_FIR_DYN", ...)."""
    v = lib().vvhip_debug_get(name.encode())
    if v == -2:
        raise VvError(f"unknown knob {name!r}")
    return v


class knobs:
    """with vv.knobs(STFT_DYN=0): ...  -- set knobs for a block, clear them after."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            debug_set(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            debug_clear(k)
        return False


def device_count():
    return lib().vvhip_available()


class FftPlan:
    """Batched FFT plan (vv_dsp_fft_make_plan_many) executed on device tensors."""

    def __init__(self, n, kind=C2C, direction=FWD, batch=1):
        self.n, self.kind, self.direction, self.batch = n, kind, direction, batch
        self.h = _vp()
        _check(lib().vv_dsp_fft_make_plan_many(n, kind, direction, batch, C.byref(self.h)), "make_plan_many")

    def __call__(self, x, out=None, stream=None):
        n, b = self.n, self.batch
        if self.kind == C2C:
            shape, dt, in_dt, in_len = (b, n), torch.complex64, torch.complex64, n
        elif self.kind == R2C:
            shape, dt, in_dt, in_len = (b, n // 2 + 1), torch.complex64, torch.float32, n
        else:
            shape, dt, in_dt, in_len = (b, n), torch.float32, torch.complex64, n // 2 + 1
        _expect(x, in_dt, b * in_len, "fft input")
        if out is None:
            out = torch.empty(shape, dtype=dt, device=x.device)
        _expect(out, dt, shape[0] * shape[1], "fft output")
        _check(lib().vv_dsp_fft_execute_device(self.h, _ptr(x), _ptr(out), _stream(stream)), "fft_execute_device")
        return out

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.vv_dsp_fft_destroy(self.h)
            self.h = None


class Stft:
    """STFT handle: fused window + FFT + |X| (or complex) over many channels.

    Frames 2j and 2j + 1 of a channel share one complex transform in the fused
    kernels: a frame's rounding error is bounded relative to the larger frame
    of its pair, and a NaN or Inf sample makes the frames that hold it
    non-finite and may make their pair partners non-finite, and no other
    frame.  The one-frame host API (vv_dsp_stft_process) has no pairs."""

    def __init__(self, nfft, hop, window=WIN_HANN):
        self.nfft, self.hop = nfft, hop
        self.h = _vp()
        prm = StftParams(nfft, hop, window)
        _check(lib().vv_dsp_stft_create(C.byref(prm), C.byref(self.h)), "stft_create")

    def frames(self, n):
        return 1 if n < self.nfft else 1 + (n - self.nfft + self.hop) // self.hop

    def spectrogram(self, sig, out=None, stream=None, complex_out=False):
        """sig: (nch, n) or (n,) float32 device tensor -> (nch, frames, nfft)."""
        sig2 = sig if sig.dim() == 2 else sig.unsqueeze(0)
        nch, n = sig2.shape
        fr = self.frames(n)
        dt = torch.complex64 if complex_out else torch.float32
        if sig2.dtype != torch.float32 or sig2.stride(1) != 1:
            raise VvError("stft signal: float32 rows with unit sample stride")
        if out is None:
            out = torch.empty((nch, fr, self.nfft), dtype=dt, device=sig.device)
        _expect(out, dt, nch * fr * self.nfft, "stft output")
        nf = _sz(0)
        f = lib().vv_dsp_stft_spectrum_device if complex_out else lib().vv_dsp_stft_spectrogram_device
        _check(f(self.h, _ptr(sig2), n, nch, sig2.stride(0), _ptr(out), fr * self.nfft, _stream(stream),
                 C.byref(nf)), "stft_spectrogram_device")
        assert nf.value == fr
        return out if sig.dim() == 2 else out[0]

    def power(self, sig, out=None, stream=None, pitch=None):
        """sig: (nch, n) or (n,) float32 -> power spectrogram (nch, frames, nfft//2 + 1).
        pitch: rows `pitch` >= nfft//2 + 1 floats apart (vv_dsp_stft_power_pitched_device):
        returns the (nch, frames, pitch) buffer, bins 0..nfft//2 of each row written."""
        sig2 = sig if sig.dim() == 2 else sig.unsqueeze(0)
        nch, n = sig2.shape
        fr, nh = self.frames(n), self.nfft // 2 + 1
        if sig2.dtype != torch.float32 or sig2.stride(1) != 1:
            raise VvError("stft signal: float32 rows with unit sample stride")
        w = nh if pitch is None else int(pitch)
        if out is None:
            out = torch.empty((nch, fr, w), dtype=torch.float32, device=sig.device)
        _expect(out, torch.float32, nch * fr * w, "stft power output")
        nf = _sz(0)
        if pitch is None:
            _check(lib().vv_dsp_stft_power_device(self.h, _ptr(sig2), n, nch, sig2.stride(0), _ptr(out), fr * nh,
                                                   _stream(stream), C.byref(nf)), "stft_power_device")
        else:
            _check(lib().vv_dsp_stft_power_pitched_device(self.h, _ptr(sig2), n, nch, sig2.stride(0), _ptr(out),
                                                           fr * w, w, _stream(stream), C.byref(nf)),
                   "stft_power_pitched_device")
        assert nf.value == fr
        return out if sig.dim() == 2 else out[0]

    def spectral_shape(self, sig, params, what, stream=None):
        """sig: (nch, n) or (n,) float32 -> {name: (nch, frames) or (frames,)} for the names
        in `what` (SHAPE_NAMES): power(pitch=...) -> spectral_shape() in one call, the
        power rows in stream-ordered scratch (vv_dsp_stft_spectral_shape_device)."""
        sig2, nch, n = _signal(sig, "stft spectral_shape")
        fr = self.frames(n)
        planes, out = _shape_planes(params, what, (nch, fr), sig.device, "stft spectral_shape")
        if planes and nch:
            nf = _sz(0)
            _check(lib().vv_dsp_stft_spectral_shape_device(self.h, C.byref(params), _vp(sig2.data_ptr()), n, nch,
                                                           sig2.stride(0), C.byref(out), fr, _stream(stream),
                                                           C.byref(nf)), "stft_spectral_shape_device")
            assert nf.value == fr
        return _planes_of(planes, sig)

    def time_stretch_length(self, n, rate):
        """(rows, samples) of time_stretch() of an n-sample signal (vv_dsp_stft_time_stretch_length)"""
        m, ln = _sz(0), _sz(0)
        _check(lib().vv_dsp_stft_time_stretch_length(self.h, n, float(rate), C.byref(m), C.byref(ln)),
               "stft_time_stretch_length")
        return m.value, ln.value

    def time_stretch(self, sig, rate, out=None, stream=None):
        """sig: (nch, n) or (n,) float32 -> (nch, out_len) or (out_len,), `rate` times as
        fast at the same pitch: spectrogram(complex_out=True) -> phase_vocoder(step=rate) ->
        reconstruct() into zeros -> out / norm, in one call with the rows in stream-ordered
        scratch (vv_dsp_stft_time_stretch_device), bit-identical to those steps."""
        sig2, nch, n = _signal(sig, "stft time_stretch")
        _, ln = self.time_stretch_length(n, rate)
        if out is None:
            out = torch.empty((nch, ln) if sig.dim() == 2 else (ln,), dtype=torch.float32, device=sig.device)
        out2 = out if out.dim() == 2 else out.unsqueeze(0)
        if out.dim() != sig.dim() or out2.dtype != torch.float32 or not out2.is_cuda or out2.shape != (nch, ln) or \
                (ln > 1 and out2.stride(1) != 1):
            raise VvError(f"stft time_stretch output: float32 device rows of shape ({nch}, {ln})")
        got = _sz(0)
        if nch:
            _check(lib().vv_dsp_stft_time_stretch_device(self.h, _vp(sig2.data_ptr()), n, nch, sig2.stride(0),
                                                         float(rate), _vp(out2.data_ptr()),
                                                         out2.stride(0) if nch > 1 else ln, _stream(stream),
                                                         C.byref(got)), "stft_time_stretch_device")
            assert got.value == ln
        return out

    def hpss(self, sig, params, harm=True, perc=True, stream=None):
        """sig: (nch, n) or (n,) float32 -> (harmonic, percussive), each (nch, out_len) or
        (out_len,), out_len = (frames - 1) * hop + nfft, or None where not asked for:
        power() -> hpss() masks -> spectrogram(complex_out=True) times a mask ->
        reconstruct() into zeros -> out / norm, in one call with the rows in stream-ordered
        scratch (vv_dsp_stft_hpss_device), bit-identical to those steps."""
        if not isinstance(params, HpssParams):
            raise VvError("stft hpss: params must be an HpssParams")
        if not (harm or perc):
            raise VvError("stft hpss: neither output asked for")
        sig2, nch, n = _signal(sig, "stft hpss")
        ln = (self.frames(n) - 1) * self.hop + self.nfft
        outs = [torch.empty((nch, ln), dtype=torch.float32, device=sig.device) if want else None
                for want in (harm, perc)]
        got = _sz(0)
        if nch:
            _check(lib().vv_dsp_stft_hpss_device(self.h, C.byref(params), _vp(sig2.data_ptr()), n, nch, sig2.stride(0),
                                                 *(None if o is None else _vp(o.data_ptr()) for o in outs), ln,
                                                 _stream(stream), C.byref(got)), "stft_hpss_device")
            assert got.value == ln
        return tuple(o if o is None or sig.dim() == 2 else o[0] for o in outs)

    def denoise(self, sig, params, stream=None):
        """sig: (nch, n) or (n,) float32 -> the signal with its stationary noise floor
        suppressed, (nch, out_len) or (out_len,), out_len = (frames - 1) * hop + nfft:
        power() -> denoise() gain -> spectrogram(complex_out=True) times the gain ->
        reconstruct() into zeros -> out / norm, in one call with the rows in stream-ordered
        scratch (vv_dsp_stft_denoise_device), bit-identical to those steps."""
        if not isinstance(params, DenoiseParams):
            raise VvError("stft denoise: params must be a DenoiseParams")
        sig2, nch, n = _signal(sig, "stft denoise")
        ln = (self.frames(n) - 1) * self.hop + self.nfft
        out = torch.empty((nch, ln), dtype=torch.float32, device=sig.device)
        got = _sz(0)
        if nch:
            _check(lib().vv_dsp_stft_denoise_device(self.h, C.byref(params), _vp(sig2.data_ptr()), n, nch,
                                                    sig2.stride(0), _vp(out.data_ptr()), ln, _stream(stream),
                                                    C.byref(got)), "stft_denoise_device")
            assert got.value == ln
        return out if sig.dim() == 2 else out[0]

    def frames_range(self, sig, frame0, nframes, kind=0, out=None, stream=None):
        """Rows of frames [frame0, frame0 + nframes) of sig's spectrogram (one shard
        of a long signal): kind 0 magnitude, 1 complex, 2 power (nfft//2 + 1 bins)."""
        sig2 = sig if sig.dim() == 2 else sig.unsqueeze(0)
        nch, n = sig2.shape
        width = self.nfft // 2 + 1 if kind == 2 else self.nfft
        dt = torch.complex64 if kind == 1 else torch.float32
        if sig2.dtype != torch.float32 or sig2.stride(1) != 1:
            raise VvError("stft signal: float32 rows with unit sample stride")
        if out is None:
            out = torch.empty((nch, nframes, width), dtype=dt, device=sig.device)
        _expect(out, dt, nch * nframes * width, "stft frames_range output")
        if nframes == 0 and frame0 <= self.frames(n):   # empty range: nothing to write (out has no storage)
            return out if sig.dim() == 2 else out[0]
        _check(lib().vv_dsp_stft_frames_range_device(self.h, _ptr(sig2), n, nch, sig2.stride(0), frame0, nframes,
                                                      _ptr(out), nframes * width, kind, _stream(stream)),
               "stft_frames_range_device")
        return out if sig.dim() == 2 else out[0]

    def process(self, frames, stream=None):
        """frames: (count, nfft) float32 -> (count, nfft) complex64 (vv_dsp_stft_process batched)."""
        _expect(frames, torch.float32, frames.shape[0] * self.nfft, "stft_process frames")
        out = torch.empty((frames.shape[0], self.nfft), dtype=torch.complex64, device=frames.device)
        _check(lib().vv_dsp_stft_process_device(self.h, _ptr(frames), frames.shape[0], _ptr(out),
                                                _stream(stream)), "stft_process_device")
        return out

    def reconstruct(self, spec, out_add, norm_add=None, stream=None):
        """spec: (count, nfft) complex64 frames at this handle's hop; adds into
        out_add (and norm_add), each at least (count - 1) * hop + nfft long."""
        count = spec.shape[0]
        _expect(spec, torch.complex64, count * self.nfft, "stft_reconstruct spectra")
        need = (count - 1) * self.hop + self.nfft if count else 0
        _expect(out_add, torch.float32, need, "stft_reconstruct out_add")
        if norm_add is not None:
            _expect(norm_add, torch.float32, need, "stft_reconstruct norm_add")
        _check(lib().vv_dsp_stft_reconstruct_device(self.h, _ptr(spec), spec.shape[0], _ptr(out_add),
                                                    _ptr(norm_add) if norm_add is not None else None,
                                                    _stream(stream)), "stft_reconstruct_device")
        return out_add

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.vv_dsp_stft_destroy(self.h)
            self.h = None


class Mfcc:
    """vv_dsp_mfcc_init plan (src/features/mel.c:249-310) run on device power rows:
    (..., n_fft//2 + 1) float32 -> MFCC (..., n_coeffs) or log-mel (..., n_mels)."""

    def __init__(self, n_fft, n_mels, n_coeffs, sample_rate, fmin, fmax, lifter=0.0, eps=1e-10):
        self.n_fft, self.n_mels, self.n_coeffs = n_fft, n_mels, n_coeffs
        self.h = _vp()
        _check(lib().vv_dsp_mfcc_init(n_fft, n_mels, n_coeffs, sample_rate, fmin, fmax, 0, 2, lifter, eps,
                                      C.byref(self.h)), "mfcc_init")

    def _run(self, power, width, f, fp, what, stream, pitched):
        nb = self.n_fft // 2 + 1
        if pitched:   # rows power.shape[-1] >= nb floats apart, bins 0..nb-1 used
            w = power.shape[-1]
            if w < nb:
                raise VvError(f"pitched power rows: pitch {w} below {nb} bins")
            p2 = power.reshape(-1, w)
            out = torch.empty((p2.shape[0], width), dtype=torch.float32, device=power.device)
            _check(fp(self.h, _ptr(p2), p2.shape[0], w, _ptr(out), _stream(stream)), what)
            return out.reshape(*power.shape[:-1], width)
        assert power.shape[-1] == nb, f"power rows must have {nb} bins"
        p2 = power.reshape(-1, nb)
        out = torch.empty((p2.shape[0], width), dtype=torch.float32, device=power.device)
        _check(f(self.h, _ptr(p2), p2.shape[0], _ptr(out), _stream(stream)), what)
        return out.reshape(*power.shape[:-1], width)

    def __call__(self, power, stream=None, pitched=False):
        """pitched: power's last dimension is the row pitch (vv_dsp_mfcc_process_pitched_device)"""
        return self._run(power, self.n_coeffs, lib().vv_dsp_mfcc_process_device,
                         lib().vv_dsp_mfcc_process_pitched_device, "mfcc_process_device", stream, pitched)

    def log_mel(self, power, stream=None, pitched=False):
        return self._run(power, self.n_mels, lib().vv_dsp_log_mel_device, lib().vv_dsp_log_mel_pitched_device,
                         "log_mel_device", stream, pitched)

    def from_signal(self, stft, sig, log_mel=False, out=None, stream=None):
        """Signal (nch, n) or (n,) float32 -> MFCC (nch, frames, n_coeffs), or log-mel
        (nch, frames, n_mels) with log_mel=True, through `stft`'s power rows without
        writing them to HBM (vv_dsp_stft_mfcc_device / vv_dsp_stft_log_mel_device):
        equal to self(stft.power(sig)) / self.log_mel(stft.power(sig))."""
        sig2 = sig if sig.dim() == 2 else sig.unsqueeze(0)
        nch, n = sig2.shape
        if sig2.dtype != torch.float32 or sig2.stride(1) != 1:
            raise VvError("mel signal: float32 rows with unit sample stride")
        fr = stft.frames(n)
        width = self.n_mels if log_mel else self.n_coeffs
        if out is None:
            out = torch.empty((nch, fr, width), dtype=torch.float32, device=sig.device)
        _expect(out, torch.float32, nch * fr * width, "mel output")
        f = lib().vv_dsp_stft_log_mel_device if log_mel else lib().vv_dsp_stft_mfcc_device
        nf = _sz(0)
        _check(f(stft.h, self.h, _ptr(sig2), n, nch, sig2.stride(0), _ptr(out), fr * width, _stream(stream),
                 C.byref(nf)), "stft_mel_device")
        assert nf.value == fr
        return out if sig.dim() == 2 else out[0]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.vv_dsp_mfcc_destroy(self.h)
            self.h = None


class FirPlan:
    def __init__(self, h):
        h = h.detach().to("cpu", torch.float32).contiguous()
        self.taps = h.numel()
        self.h = _vp()
        _check(lib().vv_dsp_fir_plan_create(C.c_void_p(h.data_ptr()), self.taps, C.byref(self.h)), "fir_plan_create")

    def __call__(self, x, out=None, direct=False, stream=None):
        """x: (nch, n) float32 device tensor -> y (nch, n)."""
        x2 = x if x.dim() == 2 else x.unsqueeze(0)
        nch, n = x2.shape
        if out is None:
            out = torch.empty_like(x2)
        f = lib().vv_dsp_fir_apply_direct_device if direct else lib().vv_dsp_fir_apply_fft_device
        _check(f(self.h, _ptr(x2), _ptr(out), n, nch, x2.stride(0), out.stride(0), _stream(stream)), "fir_apply")
        return out if x.dim() == 2 else out[0]

    def filtfilt(self, x, out=None, stream=None):
        """Zero-phase filtering (vv_dsp_filtfilt_fir, filter/common.c:23-80) of
        x: (nch, n) float32 device tensor -> y (nch, n), bit-identical per row."""
        x2 = x if x.dim() == 2 else x.unsqueeze(0)
        nch, n = x2.shape
        if x2.dtype != torch.float32 or x2.stride(1) != 1:
            raise VvError("filtfilt input: float32 rows with unit sample stride")
        if out is None:
            out = torch.empty_like(x2)
        _expect(out, torch.float32, nch * n, "filtfilt output")
        _check(lib().vv_dsp_filtfilt_fir_device(self.h, _ptr(x2), _ptr(out), n, nch, x2.stride(0), out.stride(0),
                                                _stream(stream)), "filtfilt_device")
        return out if x.dim() == 2 else out[0]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.vv_dsp_fir_plan_destroy(self.h)
            self.h = None


class Resampler:
    """Fixed-ratio resampler (vv_dsp_resampler_*): out_rate / in_rate = num / den.
    sinc=False: linear interpolation, bit-identical to the reference; sinc=True:
    windowed sinc with `taps` taps (clamped to 4..128, raised to even)."""

    def __init__(self, num, den, sinc=False, taps=32):
        L = lib()
        self.h = _vp(L.vv_dsp_resampler_create(int(num), int(den)))
        if not self.h:
            raise VvError(f"resampler_create({num}, {den}): the ratio's terms must be positive")
        _check(L.vv_dsp_resampler_set_quality(self.h, 1 if sinc else 0, int(taps)), "resampler_set_quality")

    def set_ratio(self, num, den):
        _check(lib().vv_dsp_resampler_set_ratio(self.h, int(num), int(den)), "resampler_set_ratio")

    def set_quality(self, sinc, taps=32):
        _check(lib().vv_dsp_resampler_set_quality(self.h, 1 if sinc else 0, int(taps)), "resampler_set_quality")

    def output_length(self, n):
        return lib().vv_dsp_resampler_output_length(self.h, int(n))

    def __call__(self, x, out=None, stream=None):
        """x: (n,) or (nch, n) float32 device tensor (rows with unit sample stride)
        -> y (output_length(n),) or (nch, output_length(n))."""
        x2 = x if x.dim() == 2 else x.unsqueeze(0)
        if x2.dim() != 2 or x2.dtype != torch.float32 or not x2.is_cuda or (x2.shape[1] > 1 and x2.stride(1) != 1):
            raise VvError("resampler input: float32 device rows with unit sample stride")
        nch, n = x2.shape
        m = self.output_length(n)
        if out is None:
            out = torch.empty((nch, m), dtype=torch.float32, device=x.device)
        o2 = out if out.dim() == 2 else out.unsqueeze(0)
        if o2.dtype != torch.float32 or not o2.is_cuda or o2.shape[0] != nch or o2.shape[1] < m or \
                (o2.shape[1] > 1 and o2.stride(1) != 1):
            raise VvError(f"resampler output: float32 device rows, {nch} x at least {m}")
        got = _sz(0)
        xs = x2.stride(0) if nch > 1 else n
        os_ = o2.stride(0) if nch > 1 else o2.shape[1]
        _check(lib().vv_dsp_resampler_process_device(self.h, C.c_void_p(x2.data_ptr()), n, nch, xs,
                                                     C.c_void_p(o2.data_ptr()), o2.shape[1], os_, _stream(stream),
                                                     C.byref(got)), "resampler_process_device")
        y = o2[:, :got.value]
        return y if x.dim() == 2 else y[0]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.vv_dsp_resampler_destroy(self.h)
            self.h = None


def shard_range(total, world, rank):
    """vv_dsp_shard_range: rank's contiguous channel block (first, count)."""
    a, b = _sz(), _sz()
    _check(lib().vv_dsp_shard_range(total, world, rank, C.byref(a), C.byref(b)), "shard_range")
    return a.value, b.value


def pack_half(rows, nfft, out=None, stream=None):
    """[..., nfft] float32 device rows -> [..., nfft/2+1] (vv_dsp_spectrogram_pack_half_device)."""
    if rows.shape[-1] != nfft:
        raise VvError(f"pack_half: rows of {rows.shape[-1]} bins, expected {nfft}")
    nrows = rows.numel() // nfft
    if out is None:
        out = torch.empty(tuple(rows.shape[:-1]) + (nfft // 2 + 1,), dtype=torch.float32, device=rows.device)
    _expect(rows, torch.float32, nrows * nfft, "pack_half input")
    _expect(out, torch.float32, nrows * (nfft // 2 + 1), "pack_half output")
    _check(lib().vv_dsp_spectrogram_pack_half_device(_ptr(rows), nrows, nfft, _ptr(out), _stream(stream)),
           "spectrogram_pack_half_device")
    return out


def unpack_half(half, nfft, out=None, stream=None):
    """[..., nfft/2+1] -> [..., nfft], bin k > nfft/2 from bin nfft-k (vv_dsp_spectrogram_unpack_half_device)."""
    if half.shape[-1] != nfft // 2 + 1:
        raise VvError(f"unpack_half: rows of {half.shape[-1]} bins, expected {nfft // 2 + 1}")
    nrows = half.numel() // (nfft // 2 + 1)
    if out is None:
        out = torch.empty(tuple(half.shape[:-1]) + (nfft,), dtype=torch.float32, device=half.device)
    _expect(half, torch.float32, nrows * (nfft // 2 + 1), "unpack_half input")
    _expect(out, torch.float32, nrows * nfft, "unpack_half output")
    _check(lib().vv_dsp_spectrogram_unpack_half_device(_ptr(half), nrows, nfft, _ptr(out), _stream(stream)),
           "spectrogram_unpack_half_device")
    return out


def hilbert(x, stream=None):
    """x: (batch, N) or (N,) float32 device tensor -> complex64 analytic signal.

    For power-of-two N <= 8192 rows 2j and 2j + 1 of a batch share one complex
    transform: a row's rounding error is bounded relative to the larger row of
    its pair (2e-6 * max(1, log2 N) of the pair's max-abs), and a NaN or Inf
    makes its own row non-finite and may make its pair partner non-finite, and
    no other row.  Other N, and the one-row host API, have no pairs."""
    x2 = x if x.dim() == 2 else x.unsqueeze(0)
    b, n = x2.shape
    z = torch.empty((b, n), dtype=torch.complex64, device=x.device)
    _check(lib().vv_dsp_hilbert_analytic_device(_ptr(x2), n, b, _ptr(z), _stream(stream)), "hilbert_device")
    return z if x.dim() == 2 else z[0]


def instantaneous_phase(z, stream=None):
    """z: (batch, N) or (N,) complex64 analytic rows -> unwrapped phase float32 (hilbert.c:77-96)."""
    z2 = z if z.dim() == 2 else z.unsqueeze(0)
    b, n = z2.shape
    _expect(z2, torch.complex64, b * n, "instantaneous_phase input")
    p = torch.empty((b, n), dtype=torch.float32, device=z.device)
    _check(lib().vv_dsp_instantaneous_phase_device(_ptr(z2), n, b, _ptr(p), _stream(stream)),
           "instantaneous_phase_device")
    return p if z.dim() == 2 else p[0]


def instantaneous_frequency(phase, sample_rate, stream=None):
    """phase: (batch, N) or (N,) float32 -> frequency in Hz, element 0 of a row = 0 (hilbert.c:98-113)."""
    p2 = phase if phase.dim() == 2 else phase.unsqueeze(0)
    b, n = p2.shape
    _expect(p2, torch.float32, b * n, "instantaneous_frequency input")
    f = torch.empty_like(p2)
    _check(lib().vv_dsp_instantaneous_frequency_device(_ptr(p2), n, b, float(sample_rate), _ptr(f),
                                                       _stream(stream)), "instantaneous_frequency_device")
    return f if phase.dim() == 2 else f[0]


def dct(x, dct_type=2, inverse=False, stream=None):
    """x: (batch, N) or (N,) float32 device tensor -> its DCT rows (type 2, 3 or
    4, forward or inverse; vv_dsp_dct_execute, dct.c:21-68, under the current
    vv_dsp_set_nan_policy).

    The forward type-2 transform of power-of-two N <= 8192 puts rows 2j and
    2j + 1 of a batch into one complex transform: a row's rounding error is
    bounded relative to the larger row of its pair (2e-6 * max(1, log2 N) of
    the pair's max-abs), and under the PROPAGATE policy a NaN or Inf makes its
    own row non-finite and may make its pair partner non-finite, and no other
    row.  Every other type, direction and N, and the one-row host API, have
    no pairs."""
    x2 = x if x.dim() == 2 else x.unsqueeze(0)
    b, n = x2.shape
    p = _vp()
    _check(lib().vv_dsp_dct_make_plan(n, dct_type, -1 if inverse else 1, C.byref(p)), "dct_make_plan")
    try:
        y = torch.empty_like(x2)
        _check(lib().vv_dsp_dct_execute_device(p, _ptr(x2), _ptr(y), b, _stream(stream)), "dct_execute_device")
    finally:
        lib().vv_dsp_dct_destroy(p)
    return y if x.dim() == 2 else y[0]


class CztPlan:
    """Chirp-z transform of `batch` rows (vv_dsp_czt_exec_cpx / _real semantics,
    czt.c:44-178): X[k] = sum_n x[n] A^-n W^(nk), k < m.  x: (batch, n) or (n,)
    complex64 or float32 device tensor -> complex64 (batch, m)."""

    def __init__(self, n, m, w, a=1.0 + 0j):
        self.n, self.m = n, m
        self.h = _vp()
        w, a = complex(w), complex(a)
        _check(lib().vv_dsp_czt_plan_create(n, m, w.real, w.imag, a.real, a.imag, C.byref(self.h)),
               "czt_plan_create")

    def __call__(self, x, out=None, stream=None):
        x2 = x if x.dim() == 2 else x.unsqueeze(0)
        b = x2.shape[0]
        real = not x2.is_complex()
        _expect(x2, torch.float32 if real else torch.complex64, b * self.n, "czt input")
        if x2.shape[1] != self.n:
            raise VvError(f"czt input: rows of {x2.shape[1]}, the plan's N is {self.n}")
        if out is None:
            out = torch.empty((b, self.m), dtype=torch.complex64, device=x.device)
        _expect(out, torch.complex64, b * self.m, "czt output")
        _check(lib().vv_dsp_czt_execute_device(self.h, _ptr(x2), 1 if real else 0, b, _ptr(out), _stream(stream)),
               "czt_execute_device")
        return out if x.dim() == 2 else out.view(-1)[:self.m]

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.vv_dsp_czt_plan_destroy(self.h)
            self.h = None


def _ceps_rows(fn, x, out_dtype, what, stream):
    x2 = x if x.dim() == 2 else x.unsqueeze(0)
    b, n = x2.shape
    _expect(x2, torch.float32, b * n, what + " input")
    y = torch.empty((b, n), dtype=out_dtype, device=x.device)
    _check(getattr(lib(), fn)(_ptr(x2), n, b, _ptr(y), _stream(stream)), fn)
    return y if x.dim() == 2 else y[0]


def cepstrum(x, stream=None):
    """real cepstrum of float32 rows (cepstrum.c:7-41): Re IFFT(log(|FFT x| + 1e-12))"""
    return _ceps_rows("vv_dsp_cepstrum_real_device", x, torch.float32, "cepstrum", stream)


def icepstrum_minphase(c, stream=None):
    """minimum-phase signal from cepstrum rows (cepstrum.c:43-78)"""
    return _ceps_rows("vv_dsp_icepstrum_minphase_device", c, torch.float32, "icepstrum_minphase", stream)


def minphase_from_cepstrum(c, stream=None):
    """minimum-phase spectrum (complex64, imaginary parts 0) from cepstrum rows (minphase.c:7-31)"""
    return _ceps_rows("vv_dsp_minphase_from_cepstrum_device", c, torch.complex64, "minphase_from_cepstrum", stream)


def _rows(x, what, min_len=1):
    """float32 rows (b, n) of a (n,) or (b, n) device tensor"""
    if x.dim() not in (1, 2):
        raise VvError(f"{what}: rows of shape (n,) or (batch, n), got {tuple(x.shape)}")
    x2 = x if x.dim() == 2 else x.unsqueeze(0)
    if x2.shape[1] < min_len:
        raise VvError(f"{what}: rows of {x2.shape[1]} elements, at least {min_len} needed")
    _expect(x2, torch.float32, x2.shape[0] * x2.shape[1], what)
    return x2


def autocorr(x, order, stream=None):
    """lags 0..order of float32 rows (lpc.c:7-16): (..., n) -> (..., order + 1)"""
    x2 = _rows(x, "autocorr input", order + 1)
    b, n = x2.shape
    r = torch.empty((b, order + 1), dtype=torch.float32, device=x.device)
    _check(lib().vv_dsp_autocorr_device(_ptr(x2), n, order, b, _ptr(r), _stream(stream)), "autocorr_device")
    return r if x.dim() == 2 else r[0]


def levinson(r, stream=None):
    """Levinson-Durbin on autocorrelation rows (lpc.c:18-41): (..., order + 1) ->
    a (..., order + 1) with A(z) = 1 + sum a[m] z^-m, err (...).  A row with
    r[0] <= 0 gives a = (1, 0, ..), err = 0."""
    r2 = _rows(r, "levinson input")
    b, w = r2.shape
    a = torch.empty((b, w), dtype=torch.float32, device=r.device)
    err = torch.empty((b,), dtype=torch.float32, device=r.device)
    _check(lib().vv_dsp_levinson_device(_ptr(r2), w - 1, b, _ptr(a), _ptr(err), _stream(stream)), "levinson_device")
    return (a, err) if r.dim() == 2 else (a[0], err[0])


def lpc(x, order, stream=None):
    """autocorr + levinson of float32 rows in one launch, bit-identical to
    levinson(autocorr(x, order)): (..., n) -> a (..., order + 1), err (...)"""
    x2 = _rows(x, "lpc input", order + 1)
    b, n = x2.shape
    a = torch.empty((b, order + 1), dtype=torch.float32, device=x.device)
    err = torch.empty((b,), dtype=torch.float32, device=x.device)
    _check(lib().vv_dsp_lpc_device(_ptr(x2), n, order, b, _ptr(a), _ptr(err), _stream(stream)), "lpc_device")
    return (a, err) if x.dim() == 2 else (a[0], err[0])


def num_frames(n, frame_len, hop, center=False):
    return lib().vv_dsp_get_num_frames(n, frame_len, hop, int(bool(center)))


def _signal(sig, who):
    """(sig2, nch, n) of the signal of a per-frame call: float32 device rows (nch, n) or (n,)"""
    sig2 = sig if sig.dim() == 2 else sig.unsqueeze(0)
    if sig.dim() not in (1, 2) or sig2.dtype != torch.float32 or sig2.stride(1) != 1 or not sig2.is_cuda:
        raise VvError(f"{who} signal: float32 device rows with unit sample stride")
    return (sig2,) + tuple(sig2.shape)


def _window(window, frame_len, who):
    """the optional window of a per-frame call as a pointer argument"""
    if window is None:
        return None
    _expect(window, torch.float32, frame_len, f"{who} window")
    return _ptr(window)


def _planes_of(planes, x):
    """the result planes of a (batch, n) input, or their first rows for a (n,) input"""
    return planes if x.dim() == 2 else {k: v[0] for k, v in planes.items()}


def lpc_frames(sig, frame_len, hop, order, window=None, center=False, out=None, stream=None):
    """Signal (nch, n) or (n,) float32 -> a (nch, frames, order + 1), err (nch, frames):
    the frames of vv_dsp_fetch_frames_device (times `window`, frame_len float32, when
    given) through lpc() in one kernel, bit-identical to the two steps.  out: (a, err)
    tensors to write into."""
    sig2, nch, n = _signal(sig, "lpc_frames")
    if frame_len <= 0 or hop <= 0 or order + 1 > frame_len:
        raise VvError(f"lpc_frames: frame_len {frame_len}, hop {hop}, order {order}")
    win = _window(window, frame_len, "lpc_frames")
    fr = num_frames(n, frame_len, hop, center)
    if out is None:
        a = torch.empty((nch, fr, order + 1), dtype=torch.float32, device=sig.device)
        err = torch.empty((nch, fr), dtype=torch.float32, device=sig.device)
    else:
        a, err = out
    _expect(a, torch.float32, nch * fr * (order + 1), "lpc_frames coefficients")
    _expect(err, torch.float32, nch * fr, "lpc_frames error")
    # rows may be sig2.stride(0) >= n floats apart (a view of a wider buffer)
    _check(lib().vv_dsp_lpc_frames_device(_vp(sig2.data_ptr()), n, nch, sig2.stride(0), frame_len, hop,
                                          int(bool(center)), win, order,
                                          _ptr(a), fr * (order + 1), _ptr(err), fr, _stream(stream)),
           "lpc_frames_device")
    return (a, err) if sig.dim() == 2 or out is not None else (a[0], err[0])


def _lpc_rows(a, order, who):
    """(a2, batch, order, pitch) of LPC rows (batch, w) or (w,), w >= order + 1 (order None: w - 1),
    rows a.stride(0) floats apart"""
    a2 = a if a.dim() == 2 else a.unsqueeze(0)
    if a.dim() not in (1, 2) or a2.dtype != torch.float32 or not a2.is_cuda or \
            (a2.numel() and a2.stride(1) != 1):   # an empty batch has no strides to speak of
        raise VvError(f"{who}: float32 device rows (batch, order + 1) or (order + 1,) with unit stride")
    batch, w = a2.shape
    order = w - 1 if order is None else int(order)
    if order < 1 or order > LSF_MAX_ORDER or order + 1 > w:
        raise VvError(f"{who}: order {order} for rows of {w} coefficients (1..{LSF_MAX_ORDER})")
    pitch = a2.stride(0) if batch > 1 else max(w, a2.stride(0))
    if batch and pitch < order + 1:
        raise VvError(f"{who}: overlapping rows")
    return a2, batch, order, pitch


def _named(what, names, who):
    what = (what,) if isinstance(what, str) else tuple(what)
    for name in what:
        if name not in names:
            raise VvError(f"{who}: unknown output {name!r} (one of {', '.join(names)})")
    if not what:
        raise VvError(f"{who}: no output wanted")
    return what


def _lsf_planes(what, rows_shape, order, device, who, names=LSF_NAMES):
    planes = {}
    for name in _named(what, names, who):
        if name in ("lsf", "rc"):
            planes[name] = torch.empty(rows_shape + (order,), dtype=torch.float32, device=device)
        else:
            planes[name] = torch.empty(rows_shape, dtype=torch.int32 if name == "flags" else torch.float32,
                                       device=device)
    return planes


def _opt(planes, name):
    return _vp(planes[name].data_ptr()) if name in planes else None


def lpc_to_lsf(a, what=LSF_NAMES, order=None, stream=None):
    """LPC rows (batch, w) or (w,) float32, A(z) = 1 + sum a[m] z^-m (levinson's / lpc_frames'
    rows; rows a.stride(0) floats apart, order = w - 1 unless given) -> {name: tensor} for the
    names in `what` (LSF_NAMES): lsf (batch, order) radians ascending, NaN rows where the scan is
    not complete; rc (batch, order) reflection coefficients; flags (batch,) int32, LSF_STABLE |
    LSF_COMPLETE (vv_dsp/envelope/lsf.h)."""
    a2, batch, order, pitch = _lpc_rows(a, order, "lpc_to_lsf")
    planes = _lsf_planes(what, (batch,), order, a.device, "lpc_to_lsf")
    if batch:
        _check(lib().vv_dsp_lpc_to_lsf_device(_vp(a2.data_ptr()), order, batch, pitch, _opt(planes, "lsf"),
                                              _opt(planes, "rc"), _opt(planes, "flags"), _stream(stream)),
               "lpc_to_lsf_device")
    return _planes_of(planes, a)


def lsf_to_lpc(lsf, out=None, stream=None):
    """LSF rows (batch, order) or (order,) float32 radians -> {"a": (batch, order + 1)}, a[0] = 1.
    out: a (batch, w >= order + 1) tensor whose rows (out.stride(0) apart) take the coefficients."""
    l2 = lsf if lsf.dim() == 2 else lsf.unsqueeze(0)
    if lsf.dim() not in (1, 2) or l2.dtype != torch.float32 or not l2.is_cuda or not l2.is_contiguous():
        raise VvError("lsf_to_lpc: contiguous float32 device rows (batch, order) or (order,)")
    batch, order = l2.shape
    if order < 1 or order > LSF_MAX_ORDER:
        raise VvError(f"lsf_to_lpc: order {order} (1..{LSF_MAX_ORDER})")
    a = torch.empty((batch, order + 1), dtype=torch.float32, device=lsf.device) if out is None else out
    a2, ob, _, pitch = _lpc_rows(a if a.dim() == 2 else a.unsqueeze(0), order, "lsf_to_lpc out")
    if ob < batch:
        raise VvError(f"lsf_to_lpc out: {ob} rows, {batch} needed")
    if batch:
        _check(lib().vv_dsp_lsf_to_lpc_device(_vp(l2.data_ptr()), order, batch, _vp(a2.data_ptr()), pitch,
                                              _stream(stream)), "lsf_to_lpc_device")
    return {"a": a2[:, :order + 1] if lsf.dim() == 2 else a2[0, :order + 1]}


def lsf_frames(sig, frame_len, hop, order, what=LSF_NAMES + ("err",), window=None, center=False, stream=None):
    """Signal (nch, n) or (n,) float32 -> {name: tensor}: lsf, rc (nch, frames, order), flags, err
    (nch, frames).  lpc_frames into scratch rows and lpc_to_lsf, in channel groups, bit-identical to
    the two calls (vv_dsp_lsf_frames_device)."""
    sig2, nch, n = _signal(sig, "lsf_frames")
    if frame_len <= 0 or hop <= 0 or order < 1 or order > LSF_MAX_ORDER or order + 1 > frame_len:
        raise VvError(f"lsf_frames: frame_len {frame_len}, hop {hop}, order {order}")
    win = _window(window, frame_len, "lsf_frames")
    fr = num_frames(n, frame_len, hop, center)
    planes = _lsf_planes(what, (nch, fr), order, sig.device, "lsf_frames", LSF_NAMES + ("err",))
    if fr and nch:
        _check(lib().vv_dsp_lsf_frames_device(_vp(sig2.data_ptr()), n, nch, sig2.stride(0), frame_len, hop,
                                              int(bool(center)), win, order, _opt(planes, "lsf"), _opt(planes, "rc"),
                                              _opt(planes, "flags"), _opt(planes, "err"), _stream(stream)),
               "lsf_frames_device")
    return _planes_of(planes, sig)


def _lpc_filter(which, x, a, seg_len, offset, gain, state, out, stream):
    who = f"lpc_{which}"
    x2 = _strided_rows(x, f"{who} input")
    nch, n = x2.shape
    if a.dim() not in (2, 3) or a.dtype != torch.float32 or not a.is_cuda or a.numel() == 0 or a.stride(-1) != 1 \
            or (a.dim() == 3 and a.shape[0] != nch):
        raise VvError(f"{who} rows: float32 device rows (frames, order + 1), or (nch, frames, order + 1) with "
                      f"nch = {nch}, with unit coefficient stride")
    frames, w = a.shape[-2:]
    order = w - 1
    if order < 1 or order > LPC_FILTER_MAX_ORDER or seg_len < 1:
        raise VvError(f"{who}: order {order} (1..{LPC_FILTER_MAX_ORDER}), seg_len {seg_len}")
    pitch = a.stride(-2) if frames > 1 else max(w, a.stride(-2))
    a_ch = 0 if a.dim() == 2 else a.stride(0) if nch > 1 else max(a.stride(0), (frames - 1) * pitch + w)
    if pitch < w or (a_ch and a_ch < (frames - 1) * pitch + w):
        raise VvError(f"{who} rows: overlapping rows")
    g_ch = 0
    if gain is not None:
        if gain.dim() not in (1, 2) or gain.dtype != torch.float32 or not gain.is_cuda or gain.shape[-1] != frames \
                or (frames > 1 and gain.stride(-1) != 1) or (gain.dim() == 2 and gain.shape[0] != nch):
            raise VvError(f"{who} gain: float32 device tensor ({frames},) or ({nch}, {frames}) with unit stride "
                          f"along the frames")
        g_ch = 0 if gain.dim() == 1 else gain.stride(0) if nch > 1 else max(frames, gain.stride(0))
        if g_ch and g_ch < frames:
            raise VvError(f"{who} gain: overlapping rows")
    if state is not None:
        _expect(state, torch.float64, nch * order, f"{who} state")
        if state.numel() != nch * order:
            raise VvError(f"{who} state: ({nch}, {order}) float64")
    y = torch.empty((nch, n), dtype=torch.float32, device=x.device) if out is None else out
    y2 = _strided_rows(y, f"{who} output")
    if tuple(y2.shape) != (nch, n):
        raise VvError(f"{who} output: shape {tuple(y2.shape)}, expected {(nch, n)}")
    if n and nch:
        fn = getattr(lib(), f"vv_dsp_lpc_{which}_device")
        _check(fn(_vp(x2.data_ptr()), n, nch, x2.stride(0) if nch > 1 else n, _vp(a.data_ptr()), order, frames, pitch,
                  a_ch, None if gain is None else _vp(gain.data_ptr()), g_ch, int(seg_len), int(offset),
                  None if state is None else _vp(state.data_ptr()), _vp(y2.data_ptr()),
                  y2.stride(0) if nch > 1 else n, _stream(stream)), f"{who}_device")
    return y if out is not None or x.dim() == 2 else y[0]


def lpc_residual(x, a, seg_len, offset=0, gain=None, state=None, out=None, stream=None):
    """The time-varying inverse filter A(z) (vv_dsp/envelope/lpc_filter.h): x (nch, n) or (n,)
    float32 rows, which may be x.stride(0) floats apart -> e of the same shape.  a: LPC rows
    (frames, order + 1) shared by every channel or (nch, frames, order + 1), A(z) = 1 + sum a[m]
    z^-m, rows a.stride(-2) floats apart (the rows of lpc_frames and lsf_to_lpc as they are).
    Sample t is governed by row clamp((t + offset) // seg_len, 0, frames - 1).  gain: (frames,) or
    (nch, frames) float32 (rows gain.stride(0) apart), e is divided by it; state: (nch, order) float64, the inputs before
    sample 0 newest first, updated in place (None: zeros).  Bit-identical to the header's f64
    arithmetic.  out may not overlap x."""
    return _lpc_filter("residual", x, a, seg_len, offset, gain, state, out, stream)


def lpc_synth(e, a, seg_len, offset=0, gain=None, state=None, out=None, stream=None):
    """The time-varying all-pole filter g / A(z), the inverse of lpc_residual with the same
    arguments: e (nch, n) or (n,) -> y.  The state holds the f64 outputs before sample 0.  Rows up
    to 8192 samples are one recursion, bit-identical to the header; longer rows are chunked with
    the chunks' states carried in f64.  out may be e."""
    return _lpc_filter("synth", e, a, seg_len, offset, gain, state, out, stream)


def lpc_residual_frames(sig, frame_len, hop, order, window=None, center=False, what=("e",), stream=None):
    """Signal (nch, n) or (n,) float32 -> {name: tensor} for the names in `what`: "e" the residual
    of the signal through its own per-frame LPC rows, (nch, n); "a" the rows (nch, frames, order +
    1); "err" (nch, frames).  lpc_frames followed by lpc_residual with seg_len = hop and the
    offset that lets the frame with the nearest centre govern, bit-identical to the two calls;
    rows that are not asked for stay in scratch (vv_dsp_lpc_residual_frames_device)."""
    sig2, nch, n = _signal(sig, "lpc_residual_frames")
    what = _named(what, ("e", "a", "err"), "lpc_residual_frames")
    if frame_len <= 0 or hop <= 0 or order < 1 or order > LPC_FILTER_MAX_ORDER or order + 1 > frame_len:
        raise VvError(f"lpc_residual_frames: frame_len {frame_len}, hop {hop}, order {order}")
    win = _window(window, frame_len, "lpc_residual_frames")
    fr = num_frames(n, frame_len, hop, center)
    planes = {"e": torch.empty((nch, n), dtype=torch.float32, device=sig.device)}
    if "a" in what:
        planes["a"] = torch.empty((nch, fr, order + 1), dtype=torch.float32, device=sig.device)
    if "err" in what:
        planes["err"] = torch.empty((nch, fr), dtype=torch.float32, device=sig.device)
    if fr and nch and n:
        _check(lib().vv_dsp_lpc_residual_frames_device(_vp(sig2.data_ptr()), n, nch, max(sig2.stride(0), n),
                                                       frame_len, hop, int(bool(center)), win, order,
                                                       _opt(planes, "a"), fr * (order + 1), _opt(planes, "err"), fr,
                                                       _vp(planes["e"].data_ptr()), n, _stream(stream)),
               "lpc_residual_frames_device")
    return _planes_of({k: planes[k] for k in what}, sig)


def pitch_shift_lpc(sig, ratio, frame_len, hop, order, n_fft, stft_hop, window=None):
    """Pitch shift by `ratio` with the formants kept (the chain of INTEGRATION.md): the residual
    of sig (nch, n) or (n,) through its own centred LPC rows, time-stretched to `ratio` times its
    length by the phase vocoder (Stft(n_fft, stft_hop).time_stretch at rate 1 / ratio), read back
    at step `ratio` (cubic) to n samples, and synthesised through the original rows.  A pure
    composition of lpc_residual_frames, Stft.time_stretch, interpolate_uniform and lpc_synth."""
    if not ratio > 0:
        raise VvError(f"pitch_shift_lpc: ratio {ratio}")
    sig2, nch, n = _signal(sig, "pitch_shift_lpc")
    r = lpc_residual_frames(sig2, frame_len, hop, order, window=window, center=True, what=("e", "a"))
    st = Stft(n_fft, stft_hop)
    long = st.time_stretch(r["e"], 1.0 / float(ratio))
    e2 = interpolate_uniform(long, 0.0, float(ratio), n, method="cubic")
    y = lpc_synth(e2, r["a"], hop, hop // 2)
    return y if sig.dim() == 2 else y[0]


def formant_params(sample_rate, **fields):
    """vv_dsp_formant_params_default (f_min 50 Hz, f_max sample_rate / 2 - 50, bw_max 600 Hz, 5
    formants) with `fields` overridden; host arithmetic, needs no device"""
    p = FormantParams()
    _check(lib().vv_dsp_formant_params_default(float(sample_rate), C.byref(p)), "formant_params_default")
    for k, v in fields.items():
        if k not in dict(FormantParams._fields_):
            raise VvError(f"formant_params: unknown field {k!r}")
        setattr(p, k, v)
    return p


def formant_start_points(order):
    """the Aberth start points of `order` roots as a (order, 2) float64 host tensor
    (vv_dsp_formant_start_points; host arithmetic, needs no device)"""
    out = torch.empty((max(int(order), 0), 2), dtype=torch.float64)
    _check(lib().vv_dsp_formant_start_points(int(order), _vp(out.data_ptr())), "formant_start_points")
    return out


def _formant_planes(params, what, rows_shape, order, device, who):
    if not isinstance(params, FormantParams):
        raise VvError(f"{who}: params must be a FormantParams")
    if not 1 <= params.n_formants <= 16:
        raise VvError(f"{who}: n_formants {params.n_formants} outside 1..16")
    planes, out = {}, FormantOut()
    for name in _named(what, FORMANT_NAMES, who):
        if name in ("freq", "bw"):
            planes[name] = torch.empty(rows_shape + (params.n_formants,), dtype=torch.float32, device=device)
        elif name == "roots":
            planes[name] = torch.empty(rows_shape + (order, 2), dtype=torch.float64, device=device)
        else:
            planes[name] = torch.empty(rows_shape, dtype=torch.int32, device=device)
        setattr(out, name, planes[name].data_ptr())
    return planes, out


def formants(a, params, what=("freq", "bw", "count", "flags"), order=None, stream=None):
    """LPC rows (batch, w) or (w,) float32 (as lpc_to_lsf takes them) -> {name: tensor} for the names
    in `what` (FORMANT_NAMES): freq, bw (batch, n_formants) Hz, NaN past the count; count, flags
    (batch,) int32 (FORMANT_CONVERGED); roots (batch, order, 2) float64, the poles of 1/A(z) by
    Aberth-Ehrlich (vv_dsp/features/formant.h)."""
    a2, batch, order, pitch = _lpc_rows(a, order, "formants")
    planes, out = _formant_planes(params, what, (batch,), order, a.device, "formants")
    if batch:
        _check(lib().vv_dsp_lpc_formants_device(_vp(a2.data_ptr()), order, batch, pitch, C.byref(params),
                                                C.byref(out), _stream(stream)), "lpc_formants_device")
    return _planes_of(planes, a)


def formant_frames(sig, frame_len, hop, order, params, what=("freq", "bw", "count", "flags"), window=None,
                   center=False, stream=None):
    """Signal (nch, n) or (n,) float32 -> the planes of formants() per frame, (nch, frames, ...):
    lpc_frames into scratch rows and formants, in channel groups, bit-identical to the two calls
    (vv_dsp_formants_frames_device).  Pre-emphasise the signal first where that is wanted."""
    sig2, nch, n = _signal(sig, "formant_frames")
    if frame_len <= 0 or hop <= 0 or order < 1 or order > LSF_MAX_ORDER or order + 1 > frame_len:
        raise VvError(f"formant_frames: frame_len {frame_len}, hop {hop}, order {order}")
    win = _window(window, frame_len, "formant_frames")
    fr = num_frames(n, frame_len, hop, center)
    planes, out = _formant_planes(params, what, (nch, fr), order, sig.device, "formant_frames")
    if fr and nch:
        _check(lib().vv_dsp_formants_frames_device(_vp(sig2.data_ptr()), n, nch, sig2.stride(0), frame_len, hop,
                                                   int(bool(center)), win, order, C.byref(params), C.byref(out),
                                                   _stream(stream)), "formants_frames_device")
    return _planes_of(planes, sig)


def lpspec(a, nfft, gain=None, levinson_sign=False, stream=None):
    """All-pole magnitude rows (lpc.c:55-72): a (..., order + 1) -> (..., nfft),
    gain / |1 - sum a[m] e^(-j 2 pi m k / nfft)| (the reference's sign) or, with
    levinson_sign, gain / |1 + sum ..| for rows of levinson() / lpc().  gain: one
    float32 per row (None: 1)."""
    a2 = _rows(a, "lpspec coefficients")
    b, w = a2.shape
    if gain is not None:
        _expect(gain, torch.float32, b, "lpspec gain")
    mag = torch.empty((b, nfft), dtype=torch.float32, device=a.device)
    _check(lib().vv_dsp_lpspec_device(_ptr(a2), w - 1, None if gain is None else _ptr(gain), nfft, b,
                                      int(bool(levinson_sign)), _ptr(mag), _stream(stream)), "lpspec_device")
    return mag if a.dim() == 2 else mag[0]


def _stats_planes(what, length, shape, device, who):
    """the output tensors of `what` and the vv_dsp_stats_out that points at them"""
    if isinstance(what, str):
        what = (what,)
    planes, out = {}, StatsOut()
    for name in what:
        if name not in STATS_NAMES:
            raise VvError(f"{who}: unknown statistic {name!r} (one of {', '.join(STATS_NAMES)})")
        if length < STATS_MIN_LEN.get(name, 1):
            raise VvError(f"{who}: {name} needs rows of at least {STATS_MIN_LEN.get(name, 1)} samples, got {length}")
        if name not in planes:
            planes[name] = torch.empty(shape, dtype=torch.int32 if name in STATS_COUNTS else torch.float32,
                                       device=device)
            setattr(out, name, planes[name].data_ptr())
    return planes, out


def stats(x, what, stream=None):
    """Statistics of float32 device rows (vv_dsp/core/stats.h): x (n,) or (batch, n),
    rows x.stride(0) floats apart -> {name: tensor (batch,) or scalar tensor} for the
    names in `what` (STATS_NAMES), all from one launch.  zero_crossings, argmin and
    argmax are int32 views of the uint32 values."""
    x2 = _strided_rows(x, "stats input")
    b, n = x2.shape
    if n < 1:
        raise VvError("stats input: empty rows")
    planes, out = _stats_planes(what, n, (b,), x.device, "stats")
    if planes and b:
        _check(lib().vv_dsp_stats_device(_vp(x2.data_ptr()), n, b, x2.stride(0) if b > 1 else n, C.byref(out),
                                         _stream(stream)), "stats_device")
    return _planes_of(planes, x)


def stats_frames(sig, frame_len, hop, what, window=None, center=False, stream=None):
    """Per-frame statistics straight from the signal: sig (nch, n) or (n,) float32 ->
    {name: (nch, frames) or (frames,)}, the frames of vv_dsp_fetch_frames_device (times
    `window`, frame_len float32, when given) through stats() in one kernel, bit-identical
    to the two steps."""
    sig2, nch, n = _signal(sig, "stats_frames")
    if frame_len <= 0 or hop <= 0:
        raise VvError(f"stats_frames: frame_len {frame_len}, hop {hop}")
    win = _window(window, frame_len, "stats_frames")
    fr = num_frames(n, frame_len, hop, center)
    planes, out = _stats_planes(what, frame_len, (nch, fr), sig.device, "stats_frames")
    if planes and fr and nch:
        _check(lib().vv_dsp_stats_frames_device(_vp(sig2.data_ptr()), n, nch, sig2.stride(0), frame_len, hop,
                                                int(bool(center)), win,
                                                C.byref(out), fr, _stream(stream)), "stats_frames_device")
    return _planes_of(planes, sig)


def pitch_lag_range(params, frame_len):
    """(tau_min, tau_max, integration_len) of frames of frame_len samples
    (vv_dsp_pitch_lag_range; host arithmetic, needs no device)"""
    if not isinstance(params, PitchParams):
        raise VvError("pitch: params must be a PitchParams")
    lo, hi, w = _sz(0), _sz(0), _sz(0)
    _check(lib().vv_dsp_pitch_lag_range(C.byref(params), frame_len, C.byref(lo), C.byref(hi), C.byref(w)),
           "pitch_lag_range")
    return lo.value, hi.value, w.value


def _pitch_planes(what, tau_max, shape, device, who):
    """the output tensors of `what` and the vv_dsp_pitch_out that points at them"""
    if isinstance(what, str):
        what = (what,)
    planes, out = {}, PitchOut()
    for name in what:
        if name not in PITCH_NAMES:
            raise VvError(f"{who}: unknown output {name!r} (one of {', '.join(PITCH_NAMES)})")
        if name not in planes:
            planes[name] = torch.empty(shape + (tau_max + 1,) if name == "cmnd" else shape,
                                       dtype=torch.int32 if name == "lag" else torch.float32, device=device)
            setattr(out, name, planes[name].data_ptr())
    return planes, out


def pitch(x, params, what, stream=None):
    """YIN pitch of float32 device rows (vv_dsp/features/pitch.h): x (n,) or (batch, n),
    rows x.stride(0) floats apart -> {name: tensor} for the names in `what`
    (PITCH_NAMES): f0, aperiodicity (batch,), lag (batch,) int32, cmnd (batch,
    tau_max + 1), all from one launch."""
    x2 = _strided_rows(x, "pitch input")
    b, n = x2.shape
    _, tau_max, _ = pitch_lag_range(params, n)
    planes, out = _pitch_planes(what, tau_max, (b,), x.device, "pitch")
    if planes and b:
        _check(lib().vv_dsp_pitch_device(_vp(x2.data_ptr()), n, b, x2.stride(0) if b > 1 else n, C.byref(params),
                                         C.byref(out), tau_max + 1, _stream(stream)), "pitch_device")
    return _planes_of(planes, x)


def pitch_frames(sig, frame_len, hop, params, what, window=None, center=False, stream=None):
    """Per-frame YIN pitch straight from the signal: sig (nch, n) or (n,) float32 ->
    {name: (nch, frames[, tau_max + 1]) or (frames[, tau_max + 1])}, the frames of
    vv_dsp_fetch_frames_device (times `window`, frame_len float32, when given) through
    pitch() in one kernel, bit-identical to the two steps."""
    sig2, nch, n = _signal(sig, "pitch_frames")
    if frame_len <= 0 or hop <= 0:
        raise VvError(f"pitch_frames: frame_len {frame_len}, hop {hop}")
    win = _window(window, frame_len, "pitch_frames")
    _, tau_max, _ = pitch_lag_range(params, frame_len)
    fr = num_frames(n, frame_len, hop, center)
    planes, out = _pitch_planes(what, tau_max, (nch, fr), sig.device, "pitch_frames")
    if planes and fr and nch:
        _check(lib().vv_dsp_pitch_frames_device(_vp(sig2.data_ptr()), n, nch, sig2.stride(0), frame_len, hop,
                                                int(bool(center)), win,
                                                C.byref(params), C.byref(out), fr, fr * (tau_max + 1),
                                                _stream(stream)), "pitch_frames_device")
    return _planes_of(planes, sig)


def pitch_track_params(params, frame_len):
    """the tracker's default parameters for the curves of `params` on frames of frame_len
    samples (vv_dsp_pitch_track_params_default; host arithmetic, needs no device)"""
    if not isinstance(params, PitchParams):
        raise VvError("pitch_track: params must be a PitchParams")
    tp = PitchTrackParams()
    _check(lib().vv_dsp_pitch_track_params_default(C.byref(params), frame_len, C.byref(tp)),
           "pitch_track_params_default")
    return tp


def _track_planes(tparams, what, nch, frames, device, who):
    """the output tensors of `what` and the vv_dsp_pitch_track_out that points at them"""
    if not isinstance(tparams, PitchTrackParams):
        raise VvError(f"{who}: track parameters must be a PitchTrackParams")
    if isinstance(what, str):
        what = (what,)
    planes, out = {}, PitchTrackOut()
    for name in what:
        if name not in TRACK_NAMES:
            raise VvError(f"{who}: unknown output {name!r} (one of {', '.join(TRACK_NAMES)})")
        if name not in planes:
            if name == "cost":
                planes[name] = torch.empty((nch,), dtype=torch.float64, device=device)
            else:
                planes[name] = torch.empty((nch, frames), dtype=torch.int32 if name == "lag" else torch.float32,
                                           device=device)
            setattr(out, name, planes[name].data_ptr())
    return planes, out


def pitch_track(curves, tparams, what, stream=None):
    """One f0 contour per channel from its YIN curves (vv_dsp/features/pitch_track.h):
    curves (frames, w) or (nch, frames, w) float32 device rows, w >= tau_max + 1 (the cmnd
    output of pitch_frames; rows curves.stride(-2) and channels curves.stride(0) floats
    apart) -> {name: tensor} for the names in `what` (TRACK_NAMES): lag (nch, frames)
    int32 (0 = unvoiced), f0, aperiodicity (nch, frames), cost (nch,) float64."""
    c3 = curves if curves.dim() == 3 else curves.unsqueeze(0)
    if curves.dim() not in (2, 3) or c3.dtype != torch.float32 or not c3.is_cuda or \
            (c3.shape[2] > 1 and c3.stride(2) != 1):
        raise VvError("pitch_track: float32 device curves (frames, w) or (nch, frames, w) with unit lag stride")
    nch, fr, w = c3.shape
    row = c3.stride(1) if fr > 1 else w
    chs = c3.stride(0) if nch > 1 else fr * row
    if row < w or (nch > 1 and chs < (fr - 1) * row + w):
        raise VvError("pitch_track: overlapping rows or channels")
    planes, out = _track_planes(tparams, what, nch, fr, curves.device, "pitch_track")
    if w < tparams.tau_max + 1:
        raise VvError(f"pitch_track: curves of {w} values, tau_max {tparams.tau_max}")
    if planes and fr and nch:
        _check(lib().vv_dsp_pitch_track_device(_vp(c3.data_ptr()), fr, nch, row, chs, C.byref(tparams), C.byref(out),
                                               fr, _stream(stream)), "pitch_track_device")
    return planes if curves.dim() == 3 else {k: v[0] for k, v in planes.items()}


def pitch_track_frames(sig, frame_len, hop, params, tparams, what, window=None, center=False, stream=None):
    """Signal (nch, n) or (n,) float32 -> the tracked planes of pitch_track(): pitch_frames
    (cmnd) into scratch curves and the tracker, in channel groups, bit-identical to the
    two calls (vv_dsp_pitch_track_frames_device)."""
    sig2, nch, n = _signal(sig, "pitch_track_frames")
    if frame_len <= 0 or hop <= 0:
        raise VvError(f"pitch_track_frames: frame_len {frame_len}, hop {hop}")
    if not isinstance(params, PitchParams):
        raise VvError("pitch_track_frames: params must be a PitchParams")
    win = _window(window, frame_len, "pitch_track_frames")
    fr = num_frames(n, frame_len, hop, center)
    planes, out = _track_planes(tparams, what, nch, fr, sig.device, "pitch_track_frames")
    if planes and fr and nch:
        _check(lib().vv_dsp_pitch_track_frames_device(_vp(sig2.data_ptr()), n, nch, sig2.stride(0), frame_len, hop,
                                                      int(bool(center)), win, C.byref(params), C.byref(tparams),
                                                      C.byref(out), fr, _stream(stream)), "pitch_track_frames_device")
    return _planes_of(planes, sig)


def _shape_planes(params, what, shape, device, who):
    """the output tensors of `what` and the vv_dsp_spectral_shape_out that points at them"""
    if not isinstance(params, SpectralShapeParams):
        raise VvError(f"{who}: params must be a SpectralShapeParams")
    if isinstance(what, str):
        what = (what,)
    planes, out = {}, SpectralShapeOut()
    for name in what:
        if name not in SHAPE_NAMES:
            raise VvError(f"{who}: unknown output {name!r} (one of {', '.join(SHAPE_NAMES)})")
        if name not in planes:
            planes[name] = torch.empty(shape, dtype=torch.int32 if name == "peak_bin" else torch.float32,
                                       device=device)
            setattr(out, name, planes[name].data_ptr())
    return planes, out


def spectral_shape(power, params, what, rows_per_group=0, stream=None):
    """Spectral shape descriptors of float32 device power rows
    (vv_dsp/features/spectral_shape.h): power (rows, pitch) or (ch, frames, pitch), the
    rows power.stride(-2) >= n_fft//2 + 1 floats apart (bins 0..n_fft//2 of each are
    read) -> {name: tensor (rows,) or (ch, frames)} for the names in `what`
    (SHAPE_NAMES), all from one launch; peak_bin is an int32 view of the uint32 values.
    A (ch, frames, pitch) tensor is ch groups of `frames` rows (flux is 0 at each
    channel's first frame); for (rows, pitch), rows_per_group rows form a group (0: one)."""
    if not isinstance(params, SpectralShapeParams):
        raise VvError("spectral_shape: params must be a SpectralShapeParams")
    if power.dim() not in (2, 3) or power.dtype != torch.float32 or not power.is_cuda:
        raise VvError("spectral_shape: float32 device rows (rows, pitch) or (ch, frames, pitch)")
    nb = params.n_fft // 2 + 1
    lead = tuple(power.shape[:-1])
    rows = 1
    for d in lead:
        rows *= d
    pitch = power.stride(-2) if power.shape[-2] > 1 else power.shape[-1]
    if power.shape[-1] < nb or (power.shape[-1] > 1 and power.stride(-1) != 1) or pitch < nb:
        raise VvError(f"spectral_shape: rows of {power.shape[-1]} floats, pitch {pitch}, for {nb} bins")
    if power.dim() == 3:
        if power.shape[0] > 1 and power.stride(0) != power.shape[1] * pitch:
            raise VvError("spectral_shape: channels must follow each other, frames x pitch floats apart")
        rows_per_group = power.shape[1]
    planes, out = _shape_planes(params, what, lead, power.device, "spectral_shape")
    if planes and rows:
        _check(lib().vv_dsp_spectral_shape_device(_vp(power.data_ptr()), rows, pitch, rows_per_group,
                                                  C.byref(params), C.byref(out), _stream(stream)),
               "spectral_shape_device")
    return planes


def _pvoc_rows(t, n_fft, who):
    """(t3, nch, rows, ch_stride) of complex64 device rows (rows, n_fft) or (nch, rows, n_fft):
    unit bin stride, rows n_fft apart, channels t.stride(0) >= rows * n_fft apart"""
    if t.dim() not in (2, 3) or t.dtype != torch.complex64 or not t.is_cuda:
        raise VvError(f"{who}: complex64 device rows (rows, n_fft) or (nch, rows, n_fft)")
    t3 = t if t.dim() == 3 else t.unsqueeze(0)
    nch, rows, width = t3.shape
    if width != n_fft or (width > 1 and t3.stride(2) != 1) or (rows > 1 and t3.stride(1) != n_fft):
        raise VvError(f"{who}: rows of {width} bins, {t3.stride(1)} apart, for n_fft {n_fft}")
    ch_stride = t3.stride(0) if nch > 1 else rows * n_fft
    if ch_stride < rows * n_fft:
        raise VvError(f"{who}: channels {ch_stride} apart, below rows x n_fft")
    return t3, nch, rows, ch_stride


def phase_vocoder(spec, n_fft, start=0.0, step=1.0, m=None, pos=None, out=None, stream=None):
    """Phase vocoder (vv_dsp/spectral/phase_vocoder.h): complex64 device rows spec (T, n_fft)
    or (nch, T, n_fft), as Stft.spectrogram(complex_out=True) gives them, -> (m, n_fft) or
    (nch, m, n_fft), output row j at analysis position start + j * step, or at pos[j] when
    pos (m float32 on the device, shared by the channels) is given.  m defaults to the
    number of positions below T.  The rows feed Stft.reconstruct as they are."""
    n_fft = int(n_fft)
    if n_fft < 2:
        raise VvError(f"phase_vocoder: n_fft {n_fft}")
    spec3, nch, T, in_stride = _pvoc_rows(spec, n_fft, "phase_vocoder input")
    if pos is not None:
        if pos.dim() != 1 or m not in (None, pos.shape[0]):
            raise VvError("phase_vocoder: pos must be one row of m positions")
        m = pos.shape[0]
        _expect(pos, torch.float32, m, "phase_vocoder positions")
    elif m is None:
        if not step > 0.0:
            raise VvError("phase_vocoder: m is needed when step is not positive")
        m = max(0, int((T - start) / step))
        while start + m * step < T:
            m += 1
        while m > 0 and not start + (m - 1) * step < T:
            m -= 1
    m = int(m)
    if m < 0:
        raise VvError(f"phase_vocoder: m {m}")
    if out is None:
        out = torch.empty((nch, m, n_fft), dtype=torch.complex64, device=spec.device)
        if spec.dim() == 2:
            out = out[0]
    out3, och, om, out_stride = _pvoc_rows(out, n_fft, "phase_vocoder output")
    if och != nch or om != m or out.dim() != spec.dim():
        raise VvError(f"phase_vocoder output: shape {tuple(out.shape)} for {nch} channels of {m} rows")
    if m == 0 or nch == 0:          # nothing to write (and the empty tensors have no storage to point at)
        return out
    if pos is None:
        st = lib().vv_dsp_phase_vocoder_uniform_device(_vp(spec3.data_ptr()), T, n_fft, nch, in_stride, float(start),
                                                       float(step), m, _vp(out3.data_ptr()), out_stride,
                                                       _stream(stream))
    else:
        st = lib().vv_dsp_phase_vocoder_device(_vp(spec3.data_ptr()), T, n_fft, nch, in_stride, _ptr(pos), m,
                                               _vp(out3.data_ptr()), out_stride, _stream(stream))
    _check(st, "phase_vocoder_device")
    return out


def autocorrelation(x, r_len, biased=False, stream=None):
    """r[lag] = sum x[i] x[i + lag] in f64 over n (biased) or over the n - lag terms
    (stats.c:106-122): float32 rows (..., n) -> (..., r_len); lags >= n give 0"""
    x2 = _rows(x, "autocorrelation input")
    b, n = x2.shape
    if r_len <= 0:
        raise VvError(f"autocorrelation: r_len {r_len}")
    r = torch.empty((b, r_len), dtype=torch.float32, device=x.device)
    if b:
        _check(lib().vv_dsp_autocorrelation_device(_ptr(x2), n, b, r_len, int(bool(biased)), _ptr(r),
                                                   _stream(stream)), "autocorrelation_device")
    return r if x.dim() == 2 else r[0]


def cross_correlation(x, y, r_len, stream=None):
    """r[lag] = mean of x[i] y[i + lag] over the overlapping samples (stats.c:124-139):
    float32 rows x (..., nx), y (..., ny) -> (..., r_len); lags with no overlap give 0"""
    x2 = _rows(x, "cross_correlation x")
    y2 = _rows(y, "cross_correlation y")
    if x.dim() != y.dim() or x2.shape[0] != y2.shape[0]:
        raise VvError(f"cross_correlation: x {tuple(x.shape)} and y {tuple(y.shape)} differ in rows")
    if r_len <= 0:
        raise VvError(f"cross_correlation: r_len {r_len}")
    b = x2.shape[0]
    r = torch.empty((b, r_len), dtype=torch.float32, device=x.device)
    if b:
        _check(lib().vv_dsp_cross_correlation_device(_ptr(x2), x2.shape[1], _ptr(y2), y2.shape[1], b, r_len, _ptr(r),
                                                     _stream(stream)), "cross_correlation_device")
    return r if x.dim() == 2 else r[0]


def _strided_rows(x, what):
    """float32 device rows (b, n) of a (n,) or (b, n) tensor with unit sample
    stride; the rows may be x.stride(0) floats apart (a view of a wider buffer)"""
    if x.dim() not in (1, 2):
        raise VvError(f"{what}: rows of shape (n,) or (batch, n), got {tuple(x.shape)}")
    x2 = x if x.dim() == 2 else x.unsqueeze(0)
    if x2.dtype != torch.float32 or not x2.is_cuda or (x2.shape[1] > 1 and x2.stride(1) != 1):
        raise VvError(f"{what}: float32 device rows with unit sample stride")
    if x2.shape[0] > 1 and x2.stride(0) < x2.shape[1]:
        raise VvError(f"{what}: rows {x2.stride(0)} floats apart overlap")
    return x2


def iir(x, sos, state=None, out=None, stream=None):
    """Biquad cascade over float32 rows (iir.c:21-43): x (..., n) -> y (..., n).
    sos: (stages, 5) float32 device rows b0 b1 b2 a1 a2, one cascade for all
    rows.  state: (batch, stages, 2) float32 z1 z2 per row and stage (or
    (stages, 2) for one row), read as the incoming state and updated in place;
    None: zero state.  out may be x.  Rows up to 8192 samples are bit-identical
    to the reference; longer rows are chunked (vv_dsp_iir_apply_device)."""
    x2 = _strided_rows(x, "iir input")
    b, n = x2.shape
    if sos.dim() != 2 or sos.shape[1] != 5:
        raise VvError(f"iir sos: shape (stages, 5), got {tuple(sos.shape)}")
    stages = sos.shape[0]
    _expect(sos, torch.float32, 5 * stages, "iir sos")
    if state is not None:
        _expect(state, torch.float32, b * stages * 2, "iir state")
    y = torch.empty((b, n), dtype=torch.float32, device=x.device) if out is None else out
    y2 = _strided_rows(y, "iir output")
    if tuple(y2.shape) != (b, n):
        raise VvError(f"iir output: shape {tuple(y2.shape)}, expected {(b, n)}")
    _check(lib().vv_dsp_iir_apply_device(_vp(sos.data_ptr()) if stages else None, stages,
                                         None if state is None or stages == 0 else _ptr(state), _vp(x2.data_ptr()),
                                         _vp(y2.data_ptr()), n, b, x2.stride(0) if b > 1 else n,
                                         y2.stride(0) if b > 1 else n, _stream(stream)), "iir_apply_device")
    return y if out is not None or x.dim() == 2 else y[0]


def savgol_coeffs(window_length, polyorder, deriv=0, delta=1.0):
    """The Savitzky-Golay window (host setup, bit-identical to the reference's
    coefficients, no GPU needed): a float32 CPU tensor of window_length values."""
    h = torch.empty(max(int(window_length), 1), dtype=torch.float32)
    _check(lib().vv_dsp_savgol_coeffs(window_length, polyorder, deriv, delta, _vp(h.data_ptr())), "savgol_coeffs")
    return h


def savgol(x, window_length, polyorder, deriv=0, delta=1.0, mode=0, out=None, stream=None):
    """Savitzky-Golay smoothing / differentiation of float32 rows (savgol.c:219-287),
    bit-identical to the reference: x (..., n) -> (..., n).  mode: 0 reflect,
    1 constant, 2 nearest, 3 wrap (vv_dsp_savgol_mode).  out may be x."""
    x2 = _strided_rows(x, "savgol input")
    b, n = x2.shape
    y = torch.empty((b, n), dtype=torch.float32, device=x.device) if out is None else out
    y2 = _strided_rows(y, "savgol output")
    if tuple(y2.shape) != (b, n):
        raise VvError(f"savgol output: shape {tuple(y2.shape)}, expected {(b, n)}")
    _check(lib().vv_dsp_savgol_device(_vp(x2.data_ptr()), n, b, x2.stride(0) if b > 1 else n, window_length, polyorder,
                                      deriv, delta, int(mode), _vp(y2.data_ptr()), y2.stride(0) if b > 1 else n,
                                      _stream(stream)), "savgol_device")
    return y if out is not None or x.dim() == 2 else y[0]


def medfilt(x, window_length, mode=0, out=None, stream=None):
    """Running median of float32 rows (vv_dsp/filter/median.h): x (..., n) -> (..., n),
    y[i] the value of rank window_length // 2 of x[i - h .. i + h] in the order
    -inf < .. < -0 < +0 < .. < +inf < NaN, bit for bit one of its inputs.  mode: 0
    reflect, 1 nearest, 2 zero (MEDFILT_*).  out must not overlap x."""
    x2 = _strided_rows(x, "medfilt input")
    b, n = x2.shape
    y = torch.empty((b, n), dtype=torch.float32, device=x.device) if out is None else out
    y2 = _strided_rows(y, "medfilt output")
    if tuple(y2.shape) != (b, n):
        raise VvError(f"medfilt output: shape {tuple(y2.shape)}, expected {(b, n)}")
    _check(lib().vv_dsp_medfilt_device(_vp(x2.data_ptr()), n, b, x2.stride(0) if b > 1 else n, int(window_length),
                                       int(mode), _vp(y2.data_ptr()), y2.stride(0) if b > 1 else n, _stream(stream)),
           "medfilt_device")
    return y if out is not None or x.dim() == 2 else y[0]


def hpss(power, params, what, rows_per_group=0, stream=None):
    """Harmonic-percussive separation of float32 device power rows
    (vv_dsp/spectral/hpss.h): power (rows, pitch) or (ch, frames, pitch), the rows
    power.stride(-2) >= n_fft//2 + 1 floats apart (bins 0..n_fft//2 of each are read) ->
    {name: tensor (rows, n_fft//2 + 1) or (ch, frames, n_fft//2 + 1)} for the names in
    `what` (HPSS_NAMES: harm, perc, mask_harm, mask_perc).  A (ch, frames, pitch) tensor is
    ch groups of `frames` rows; for (rows, pitch), rows_per_group rows form a group (0: one)."""
    if not isinstance(params, HpssParams):
        raise VvError("hpss: params must be an HpssParams")
    if power.dim() not in (2, 3) or power.dtype != torch.float32 or not power.is_cuda:
        raise VvError("hpss: float32 device rows (rows, pitch) or (ch, frames, pitch)")
    nb = params.n_fft // 2 + 1
    lead = tuple(power.shape[:-1])
    rows = 1
    for d in lead:
        rows *= d
    pitch = power.stride(-2) if power.shape[-2] > 1 else power.shape[-1]
    if power.shape[-1] < nb or (power.shape[-1] > 1 and power.stride(-1) != 1) or pitch < nb:
        raise VvError(f"hpss: rows of {power.shape[-1]} floats, pitch {pitch}, for {nb} bins")
    if power.dim() == 3:
        if power.shape[0] > 1 and power.stride(0) != power.shape[1] * pitch:
            raise VvError("hpss: channels must follow each other, frames x pitch floats apart")
        rows_per_group = power.shape[1]
    if isinstance(what, str):
        what = (what,)
    planes, out = {}, HpssOut()
    for name in what:
        if name not in HPSS_NAMES:
            raise VvError(f"hpss: unknown output {name!r} (one of {', '.join(HPSS_NAMES)})")
        if name not in planes:
            planes[name] = torch.empty(lead + (nb,), dtype=torch.float32, device=power.device)
            setattr(out, name, planes[name].data_ptr())
    if planes and rows:
        _check(lib().vv_dsp_hpss_device(_vp(power.data_ptr()), rows, pitch, rows_per_group, C.byref(params),
                                        C.byref(out), nb, _stream(stream)), "hpss_device")
    return planes


def denoise_params(n_fft, **fields):
    """the default parameters for rows of n_fft//2 + 1 bins (vv_dsp_denoise_params_default:
    smooth_len 8, back 48, ahead 48, bias 4, floor 0.1, WIENER; host arithmetic, needs no
    device), with the fields given by name replaced"""
    prm = DenoiseParams()
    _check(lib().vv_dsp_denoise_params_default(n_fft, C.byref(prm)), "denoise_params_default")
    for name, value in fields.items():
        if name not in dict(DenoiseParams._fields_):
            raise VvError(f"denoise_params: unknown field {name!r}")
        setattr(prm, name, value)
    return prm


def denoise(power, params, what="gain", rows_per_group=0, stream=None):
    """Minimum-statistics noise floor and gain of float32 device power rows
    (vv_dsp/spectral/denoise.h): power (rows, pitch) or (ch, frames, pitch), the rows
    power.stride(-2) >= n_fft//2 + 1 floats apart (bins 0..n_fft//2 of each are read) ->
    {name: tensor (rows, n_fft//2 + 1) or (ch, frames, n_fft//2 + 1)} for the names in
    `what` (DENOISE_NAMES: smooth, noise, gain), one launch.  A (ch, frames, pitch) tensor
    is ch groups of `frames` rows; for (rows, pitch), rows_per_group rows form a group (0: one)."""
    if not isinstance(params, DenoiseParams):
        raise VvError("denoise: params must be a DenoiseParams")
    if power.dim() not in (2, 3) or power.dtype != torch.float32 or not power.is_cuda:
        raise VvError("denoise: float32 device rows (rows, pitch) or (ch, frames, pitch)")
    nb = params.n_fft // 2 + 1
    lead = tuple(power.shape[:-1])
    rows = 1
    for d in lead:
        rows *= d
    pitch = power.stride(-2) if power.shape[-2] > 1 else power.shape[-1]
    if power.shape[-1] < nb or (power.shape[-1] > 1 and power.stride(-1) != 1) or pitch < nb:
        raise VvError(f"denoise: rows of {power.shape[-1]} floats, pitch {pitch}, for {nb} bins")
    if power.dim() == 3:
        if power.shape[0] > 1 and power.stride(0) != power.shape[1] * pitch:
            raise VvError("denoise: channels must follow each other, frames x pitch floats apart")
        rows_per_group = power.shape[1]
    if isinstance(what, str):
        what = (what,)
    planes, out = {}, DenoiseOut()
    for name in what:
        if name not in DENOISE_NAMES:
            raise VvError(f"denoise: unknown output {name!r} (one of {', '.join(DENOISE_NAMES)})")
        if name not in planes:
            planes[name] = torch.empty(lead + (nb,), dtype=torch.float32, device=power.device)
            setattr(out, name, planes[name].data_ptr())
    if planes and rows:
        _check(lib().vv_dsp_denoise_device(_vp(power.data_ptr()), rows, pitch, rows_per_group, C.byref(params),
                                           C.byref(out), nb, _stream(stream)), "denoise_device")
    return planes


INTERP_LINEAR, INTERP_CUBIC = 0, 1
INTERP_METHODS = {"linear": INTERP_LINEAR, "cubic": INTERP_CUBIC}


def _interp_method(method):
    if method in INTERP_METHODS:
        return INTERP_METHODS[method]
    if method in (INTERP_LINEAR, INTERP_CUBIC) and not isinstance(method, bool):
        return int(method)
    raise VvError(f"interpolate method: 'linear' or 'cubic', got {method!r}")


def _interp_rows(x, m, out, who):
    """the checked signal rows (b, n) and output rows (b, m) of an interpolation call"""
    x2 = _strided_rows(x, f"{who} input")
    b, n = x2.shape
    if n == 0:
        raise VvError(f"{who} input: rows of no samples")
    y = torch.empty((b, m), dtype=torch.float32, device=x.device) if out is None else out
    y2 = _strided_rows(y, f"{who} output")
    if tuple(y2.shape) != (b, m):
        raise VvError(f"{who} output: shape {tuple(y2.shape)}, expected {(b, m)}")
    if y2.device != x2.device:
        raise VvError(f"{who} output: on {y2.device}, the input is on {x2.device}")
    return x2, y, y2


def interpolate(x, pos, method="linear", out=None, stream=None):
    """Rows read at arbitrary fractional positions (interpolate.c:4-64, bit-identical
    to the reference per output): x (..., n) float32 device rows with unit sample
    stride, which may be x.stride(0) floats apart -> (..., m).  pos: (m,) float32,
    one curve shared by every row, or (batch, m), one per row; contiguous, on x's
    device.  method: "linear" or "cubic" (Catmull-Rom).  Positions at or beyond the
    ends give the end samples; a NaN position gives NaN.  out may not overlap x or pos."""
    meth = _interp_method(method)
    if pos.dim() not in (1, 2) or pos.dtype != torch.float32 or not pos.is_cuda or not pos.is_contiguous():
        raise VvError("interpolate positions: a contiguous float32 device tensor of shape (m,) or (batch, m)")
    m = pos.shape[-1]
    x2, y, y2 = _interp_rows(x, m, out, "interpolate")
    b, n = x2.shape
    if pos.device != x2.device:
        raise VvError(f"interpolate positions: on {pos.device}, the input is on {x2.device}")
    if pos.dim() == 2 and pos.shape[0] != b:
        raise VvError(f"interpolate positions: {pos.shape[0]} rows for {b} signal rows")
    if m and b:
        _check(lib().vv_dsp_interpolate_device(_vp(x2.data_ptr()), n, b, x2.stride(0) if b > 1 else n,
                                               _vp(pos.data_ptr()), m, m if pos.dim() == 2 else 0, meth,
                                               _vp(y2.data_ptr()), y2.stride(0) if b > 1 else m, _stream(stream)),
               "interpolate_device")
    return y if out is not None or x.dim() == 2 else y[0]


def interpolate_uniform(x, start, step, m, method="linear", out=None, stream=None):
    """interpolate() at positions (float)(start + k * step), k < m, formed in f64 on
    the device with the product and the sum rounded separately; no position array
    is read.  step may be negative (reverse playback) or zero."""
    meth = _interp_method(method)
    m = int(m)
    if m < 0:
        raise VvError(f"interpolate_uniform: m = {m}")
    x2, y, y2 = _interp_rows(x, m, out, "interpolate_uniform")
    b, n = x2.shape
    if m and b:
        _check(lib().vv_dsp_interpolate_uniform_device(_vp(x2.data_ptr()), n, b, x2.stride(0) if b > 1 else n,
                                                       float(start), float(step), m, meth, _vp(y2.data_ptr()),
                                                       y2.stride(0) if b > 1 else m, _stream(stream)),
               "interpolate_uniform_device")
    return y if out is not None or x.dim() == 2 else y[0]


def interp_run_length():
    """consecutive outputs of one row that one workgroup of the interpolation kernel takes"""
    return lib().vvhip_interp_run_length()


def _ptrs(xs):
    """per-local-rank pointer array (vv_dsp_dist.h): tensors, raw ints or None"""
    return (_vp * len(xs))(*[None if x is None else (x if isinstance(x, int) else x.data_ptr()) for x in xs])


def _streams(streams, n, devices=None):
    """per-slot hipStream_t array; default: each slot's device's current stream"""
    if streams is None:
        streams = [torch.cuda.current_stream(d) for d in devices] if devices is not None else \
            [torch.cuda.current_stream()] * n
    if len(streams) != n:
        raise VvError(f"{len(streams)} streams for {n} local ranks")
    return (_vp * n)(*[s if (s is None or isinstance(s, int)) else s.cuda_stream for s in streams])


class Dist:
    """Multi-GPU layout of the spectral path over RCCL (include/vv_dsp/vv_dsp_dist.h):
    Dist.all([0, 1, ...]) -- every rank in this process (ncclCommInitAll);
    Dist.from_comm(ptr)   -- one rank of a caller's ncclComm_t;
    Dist.rank(world, r, id, device) -- one rank per process (ncclCommInitRank;
                             id = Dist.unique_id() on rank 0, shared by the caller);
    Dist.loopback(world)  -- `world` ranks on one device, transfers as device copies.
    Per-rank list arguments have one element per local rank (slot); streams
    default to each slot's device's current stream."""

    def __init__(self, handle):
        self.h = handle
        self.slots = lib().vv_dsp_dist_local_ranks(self.h)
        self.devices = [self.rank_info(s)[2] for s in range(self.slots)]

    @staticmethod
    def unique_id():
        """VV_DSP_DIST_ID_BYTES (128) bytes naming a new communicator (ncclGetUniqueId)"""
        buf = C.create_string_buffer(128)
        _check(lib().vv_dsp_dist_unique_id(buf), "dist_unique_id")
        return buf.raw

    @classmethod
    def rank(cls, world, rank, uid, device):
        if len(uid) != 128:
            raise VvError("a communicator id is 128 bytes")
        h = _vp()
        _check(lib().vv_dsp_dist_init_rank(world, rank, bytes(uid), device, C.byref(h)), "dist_init_rank")
        return cls(h)

    def comm_count(self, slot=0):
        """ranks RCCL reports for slot's communicator (ncclCommCount)"""
        n = C.c_int()
        _check(lib().vv_dsp_dist_comm_count(self.h, slot, C.byref(n)), "dist_comm_count")
        return n.value

    @classmethod
    def all(cls, devices):
        h = _vp()
        arr = (C.c_int * len(devices))(*devices)
        _check(lib().vv_dsp_dist_init_all(len(devices), arr, C.byref(h)), "dist_init_all")
        return cls(h)

    @classmethod
    def loopback(cls, world, device=0):
        h = _vp()
        _check(lib().vv_dsp_dist_init_loopback(world, device, C.byref(h)), "dist_init_loopback")
        return cls(h)

    @classmethod
    def from_comm(cls, comm_ptr):
        h = _vp()
        _check(lib().vv_dsp_dist_from_comm(comm_ptr, C.byref(h)), "dist_from_comm")
        return cls(h)

    def rank_info(self, slot):
        r, w, d = C.c_int(), C.c_int(), C.c_int()
        _check(lib().vv_dsp_dist_rank_info(self.h, slot, C.byref(r), C.byref(w), C.byref(d)), "dist_rank_info")
        return r.value, w.value, d.value

    def stft(self, st, sigs, n, total_ch, ch_stride, rows, out_kind=0, streams=None):
        nf = _sz(0)
        _check(lib().vv_dsp_dist_stft(self.h, st.h, _ptrs(sigs), n, total_ch, ch_stride, out_kind, _ptrs(rows),
                                      _streams(streams, self.slots, self.devices), C.byref(nf)), "dist_stft")
        return nf.value

    def gather_rows(self, local, total_items, rows_per_item, row_floats, out, root=0, half=False, streams=None):
        """items (channels) of rows_per_item rows of row_floats floats; rank r's
        items from vv_dsp_shard_range(total_items, world, r)"""
        _check(lib().vv_dsp_dist_gather_rows(self.h, _ptrs(local), total_items, rows_per_item, row_floats,
                                             1 if half else 0,
                                             None if out is None else _ptr(out), root,
                                             _streams(streams, self.slots, self.devices)), "dist_gather_rows")

    def fft(self, n, kind, direction, total_batch, ins, outs, streams=None):
        _check(lib().vv_dsp_dist_fft(self.h, n, kind, direction, total_batch, _ptrs(ins), _ptrs(outs),
                                     _streams(streams, self.slots, self.devices)), "dist_fft")

    def fir(self, plans, n, total_ch, xs, x_stride, ys, y_stride, streams=None):
        arr = (_vp * len(plans))(*[p.h for p in plans])
        _check(lib().vv_dsp_dist_fir_apply_fft(self.h, arr, n, total_ch, _ptrs(xs), x_stride, _ptrs(ys), y_stride,
                                               _streams(streams, self.slots, self.devices)), "dist_fir_apply_fft")

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.vv_dsp_dist_destroy(self.h)
            self.h = None
