// stft_kernels.hip -- fused STFT analysis for gfx950: the router.
//
// For every (channel, frame) of the reference's spectrogram (stft.c:112-144):
// gather the frame (zero past the end of the signal, stft.c:124-130), apply the
// window (vectorized_math_fallback.c:13-29), FFT, and write either magnitudes
// sqrtf(re^2+im^2) for all nfft bins (stft.c:133-139), the full complex
// spectrum (stft_process semantics, stft.c:74-92), or the power of bins 0..nfft/2.
//
// The kernels live one family per unit, each with its launcher:
//   stft_pair.hip    k_stft_pair (stft_pair.hpp): the mirror-paired sizes
//   stft_small.hip   k_stft_pair_lds, k_stft_one, k_stft_stage: nfft 256 and 4096
//   stft_mel.hip     launch_stft_mel: the fused log-mel / MFCC rows, and the
//                    power rows of nfft 1024 they must equal
// (k_stft_r32, stft_r32.hpp, is the A/B alternative of both at nfft 1024 / hop 256),
//   stft_generic.hip any nfft: gather, magnitude, power, half-row packing
// and stft_launch.hpp holds the launch rules they share.
#include "fft_core.hpp"
#include "stft_launch.hpp"

namespace vvh {

bool stft_fused_supported(long long nfft) {
    return nfft >= 2 && nfft <= 8192 && (nfft & (nfft - 1)) == 0;
}

// the family of size N: mirror-paired last pass or not
template <int N, int MODE>
static hipError_t run_stft(const StftJob& j) {
    if constexpr (Geo<N>::CAN_PAIR) return run_stft_pair<N, MODE>(j);
    else return run_stft_small<N, MODE>(j);
}

hipError_t launch_stft(long long nfft, long long hop, int mode, const float* sig, long long n,
                       long long nch, long long ch_stride, long long frames, const float* win,
                       void* out, long long out_ch_stride, hipStream_t s, long long row_pitch) {
    // floats (mode 1: complex values) from one row's start to the next: only power rows may be pitched (<= 0: packed)
    row_pitch = mode == 2 ? (row_pitch > 0 ? row_pitch : nfft / 2 + 1) : nfft;
    const StftJob j{sig, n, nch, ch_stride, frames, hop, win, out, out_ch_stride, row_pitch, s};
#define CALL(NN) (mode == 0 ? run_stft<NN, 0>(j) : mode == 1 ? run_stft<NN, 1>(j) : run_stft<NN, 2>(j))
    switch (nfft) {
        case 2: return CALL(2); case 4: return CALL(4); case 8: return CALL(8); case 16: return CALL(16);
        case 32: return CALL(32); case 64: return CALL(64); case 128: return CALL(128);
        case 256: return CALL(256); case 512: return CALL(512); case 1024: return CALL(1024);
        case 2048: return CALL(2048); case 4096: return CALL(4096); case 8192: return CALL(8192);
        default: return hipErrorInvalidValue;
    }
#undef CALL
}

// stft_process over explicit frames [count][nfft] (no overlap): same kernels, hop = nfft.
hipError_t launch_stft_frames(long long nfft, const float* frames_in, const float* win, float2* out,
                              long long count, hipStream_t s) {
    return launch_stft(nfft, nfft, 1, frames_in, nfft * count, 1, 0, count, win, out, 0, s);
}

}  // namespace vvh
