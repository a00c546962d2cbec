// stft_mel.hip -- signal -> log-mel / MFCC rows in one launch: modes 3 / 4 of
// k_stft_pair (N = 1024) and, on knob MEL_R32, of k_stft_r32 -- and the power
// rows of nfft 1024 (k_stft_pair mode 2) those fused rows must equal.
#include "stft_pair_launch.hpp"

namespace vvh {

// Signal -> log-mel (MODE 3) / MFCC (MODE 4) rows.  The launch follows
// run_stft_pair's bulk path (pair_walk: the chunked non-persistent grid, or the
// dynamic walk for large jobs); the plan's tables ride in dynamic LDS, so the
// occupancy is computed per call.
template <int MODE>
static hipError_t run_stft_mel(const StftJob& j, const MelArgs& mel_in) {
    constexpr int N = 1024, WG = Wg<N>::value, F = Wg<N>::F;
    const float2* tN = twiddle_table(N);
    const float2* pN = pass_twiddles(N);
    float* sink = store_sink();
    if (!tN || !pN || !sink) return hipErrorOutOfMemory;
    const long long ppc = (j.frames + 1) / 2, pairs = j.nch * ppc;
    if (pairs <= 0) return hipSuccess;
    // the plan's tables in dynamic LDS (the kernel's layout); occupancy per call
    auto dyn_of = [&](const MelArgs& a) {
        const long long dp = (a.nnz + (long long)a.cw * a.nc + a.M + 1 + 3) & ~3LL;
        return sizeof(float) * (size_t)(dp + (MODE == 4 ? (long long)a.C * a.M + a.C : 0));
    };
    // log-mel (MODE 3): the chunk windows (cw = 0); MFCC: the windows too when
    // they keep the packed table's workgroups per CU, else the packed chunks
    MelArgs mel = mel_in;
    auto windows = [&](MelArgs& a) {
        a.W = mel_in.Ww;
        a.chunks = nullptr;
        a.cw = 0;
        a.lc = mel_in.lcw;
        a.lcs = MelArgs::window_stride(mel_in.lcw);
        a.nnz = mel_in.nc * a.lcs;
    };
    auto per_cu = [](const void* kern, int wg, size_t dyn) {   // resident workgroups per CU (0: none, or no answer)
        int r = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, kern, wg, dyn) == hipSuccess ? r : 0;
    };
    const bool have_w = mel_in.Ww && mel_in.lcw > 0 && mel_in.lcw % 4 == 0;
    if constexpr (MODE == 3) {
        if (!have_w) return hipErrorNotSupported;
        windows(mel);
    } else if (have_w && knob(KNOB_MFCC_WIN, 1) != 0) {   // knob MFCC_WIN = 0: the packed chunks (A/B)
        MelArgs mw = mel_in;
        windows(mw);
        int pw = 0, pp = 0;
        const void* const kp = (const void*)k_stft_pair<N, MODE, 0>;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pw, kp, WG, dyn_of(mw)) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&pp, kp, WG, dyn_of(mel_in)) == hipSuccess && pw >= pp)
            mel = mw;
    }
    const size_t dyn = dyn_of(mel);
    // knob MEL_R32 = 1 (with POW_R32 = 1, so the fused rows stay bit-identical to
    // the power rows + launch_mel_grp): the 32 x 32 split (A/B; round 5, same
    // buffers: log-mel 3.38 / MFCC 4.02 ms against 3.21 / 3.52 for 32 ch x 10 min
    // -- two serial mel tails per wave at two waves per SIMD)
    if (stft_r32_ok(j) && knob(KNOB_MEL_R32, 0) == 1 && knob(KNOB_POW_R32, 0) == 1 &&
        per_cu((const void*)k_stft_r32<MODE>, 512, dyn) >= 1)
        return launch_r32<MODE>(k_stft_r32<MODE>, 512, 8, dyn, STAT_MEL_R32, j, tN, mel);
    const void* const k0 = (const void*)k_stft_pair<N, MODE, 0>;
    const int cap = persistent_grid(k0, WG, dyn, 1LL << 40);
    if (per_cu(k0, WG, dyn) < 1) return hipErrorNotSupported;
    // the walk of the power rows' bulk launch, sized by this kernel with its tables (VAR 0's grid for either walk)
    const PairWalk w = pair_walk(pairs, F, cap, cap, knob(KNOB_STFT_DYN, -1) != 0, 0, j.s);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)w.grid), dim3(WG), dyn, j.s, j.sig, j.n, j.nch, j.ch_stride, j.frames,
                           j.hop, 0LL, ppc, j.win, j.out, j.out_ch_stride, 0LL, pN, tN, w.chunk, sink, w.ctrs, mel);
    };
    if (w.dyn) launch(k_stft_pair<N, MODE, 4>);
    else launch(k_stft_pair<N, MODE, 0>);
    return hipGetLastError();
}

hipError_t launch_stft_mel(int kind, long long nfft, long long hop, const float* sig, long long n, long long nch,
                           long long ch_stride, long long frames, const float* win, const MelArgs& mel, float* out,
                           long long out_ch_stride, hipStream_t s) {
    // the LDS-DMA span path's input conditions, as run_stft_pair's `aligned` but
    // hop <= 256, not N / 2: beside the tables a span holds N + 256 floats;
    // one store instruction per 64 output values, and power rows of this nfft
    const StftJob j{sig, n, nch, ch_stride, frames, hop, win, out, out_ch_stride, 0, s};
    const bool shape_ok = nfft == 1024 && stft_span_ok(j, 256) && mel.M >= 1 && mel.M <= 128 &&
                          mel.nc <= 64 * MEL_MAX_ROUNDS && mel.cw == 3 &&
                          (kind == 0 || (mel.C >= 1 && mel.C <= 64 && 2 * mel.M <= ri_floats<1024>() - MEL_LM_OFF));
    if (!shape_ok || (kind != 0 && kind != 1)) return hipErrorNotSupported;
    return kind == 0 ? run_stft_mel<3>(j, mel) : run_stft_mel<4>(j, mel);
}

// The power rows of nfft 1024 are instantiated in this unit, not in
// stft_pair.hip: the compiler's instruction order inside the fused kernels'
// power step (pair_post<2>) depends on the power-row kernels being compiled in
// the same module (scripts/isadiff.py against a build without them shows it).
template hipError_t run_stft_pair<1024, 2>(const StftJob&);

}  // namespace vvh
