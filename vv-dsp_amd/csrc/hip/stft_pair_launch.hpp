// stft_pair_launch.hpp -- run_stft_pair<N, MODE>: the launch of k_stft_pair for
// magnitude, complex and power rows (modes 0..2), and of their nfft 1024 / hop
// 256 A/B alternative k_stft_r32 (modes 0 / 2).  A template in a header
// because its instantiations are spread over two units: stft_pair.hip holds all
// of them but the power rows of nfft 1024, which stft_mel.hip instantiates
// beside the fused log-mel / MFCC kernels that must equal them.
#pragma once
#include "stft_launch.hpp"
#include "stft_pair.hpp"
#include "stft_r32.hpp"

namespace vvh {

template <int N, int MODE>
hipError_t run_stft_pair(const StftJob& j) {
    static_assert(Geo<N>::CAN_PAIR, "the other sizes: stft_small.hip");
    const float* const sig = j.sig;
    void* const out = j.out;
    const long long n = j.n, nch = j.nch, ch_stride = j.ch_stride, frames = j.frames, hop = j.hop,
                    out_ch_stride = j.out_ch_stride;
    const float2* tN = twiddle_table(N);
    const float2* pN = pass_twiddles(N);
    if (!tN || !pN) return hipErrorOutOfMemory;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    // pairs whose two frames lie inside the signal, then the zero-padded tail
    const long long nfull = n >= N ? (n - N) / hop + 1 : 0;
    const long long ppc = (frames + 1) / 2;
    long long mpc = (nfull < frames ? nfull : frames) / 2;
    if (mpc > ppc) mpc = ppc;
    const long long tpc = ppc - mpc;
    static std::atomic<int> capc[7];   // zero-initialised (static storage)
    const long long bulk_pairs = nch * ppc;
    float* sink = store_sink();
    if (!sink) return hipErrorOutOfMemory;
    // 16 B aligned output rows allow the staged 16 B/lane stores
    // (power rows are n/2+1 floats: their direct stores are dwords, 4 B suffice;
    // complex rows are stored 8 B per lane)
    bool aligned = MODE == 2   ? ((uintptr_t)out & 3) == 0
                   : MODE == 1 ? ((uintptr_t)out & 7) == 0
                               : ((uintptr_t)out & 15) == 0 && (out_ch_stride & 3) == 0 && N >= 4;
    // T >= 64: VAR 0 also reads its input spans by 16 B LDS-DMA (spans of N + N / 2 floats)
    if (Geo<N>::T >= 64) aligned = aligned && stft_span_ok(j, N / 2);
    if (MODE != 0 && knob(KNOB_POW_OLD, 0) == 1) aligned = false;   // A/B: register loads, per-bin stores
    // the VAR 0 kernels that read spans by LDS-DMA run the tail pairs too:
    // one launch for the whole job
    constexpr bool FUSE_TAIL = (MODE == 0 || Geo<N>::T == 64) && Geo<N>::NPASS > 1 && Geo<N>::T >= 64;
    // ring spans (VAR 3) when the span is whole 256-float chunks: power rows only
    // (2.74 vs 2.84 ms for 32 ch x 10 min; magnitude and complex rows measured
    // 1-2 % slower than with VAR 0's interleaved walk, profiles/r02_kbench_ring.jsonl).
    // knob STFT_RING = 0 / 1 forces VAR 0 / VAR 3 (A/B)
    const long long kring = knob(KNOB_STFT_RING, -1);
    const bool ring = Geo<N>::T == 64 && hop == 256 && (kring >= 0 ? kring == 1 : MODE == 2);
    // power rows, nfft 1024 / hop 256, 8 B aligned channels: the 32 x 32 split
    // (k_stft_r32) on knob POW_R32 = 1 (A/B; round 5, same buffers: 3.02 ms
    // against the ring walk's 2.70 for 32 ch x 10 min -- its 128 B half-wave
    // stores leave in a burst at two waves per SIMD)
    if constexpr (N == 1024 && MODE == 2) {
        if (stft_r32_ok(j) && knob(KNOB_POW_R32, 0) == 1)
            return launch_r32<2>(k_stft_r32<2>, 256, 4, 0, STAT_POW_R32, j, tN, MelArgs{});
    }
    if constexpr (N == 1024 && MODE == 0) {   // magnitude rows: the same split on knob MAG_R32 = 1 (A/B), whole-line rows
        if (knob(KNOB_MAG_R32, 0) == 1 && stft_r32_ok(j) && ((uintptr_t)out & 127) == 0 && (out_ch_stride & 31) == 0)
            return launch_r32<0>(k_stft_r32<0>, 256, 4, 0, STAT_MAG_R32, j, tN, MelArgs{});
    }
    // Magnitude and complex rows of large jobs: the persistent dynamic walk (VAR 4) --
    // each wave takes its next pair from a per-(XCD group, slot) counter, so
    // the chip sweeps one moving band of pairs with the load balanced on the
    // fly (-1.6 % against the chunked launch in two same-buffer measurements,
    // profiles/r03_kbench_ablation_samebuf.jsonl lab8192; bit-identical rows).
    // Knob STFT_DYN = 0 keeps the chunked VAR 0 (A/B).
    // Complex rows take it too (1.629 -> 1.579 ms for 8 ch x 10 min, -3.1 %);
    // power rows keep the ring walk (2.689 ring vs 2.730 dynamic vs
    // 2.760 chunked, profiles/r03_kbench_dyn_modes.jsonl).  Knob STFT_DYN =
    // 1 forces it for every row kind (A/B).
    const long long kdyn = knob(KNOB_STFT_DYN, -1);
    int capd = 0;   // T != 64: no dynamic kernel
    if constexpr (Geo<N>::T == 64) capd = cached_grid(capc[4], (const void*)k_stft_pair<N, MODE, 4>, WG, 0, 1LL << 40);
    const bool want = kdyn >= 0 ? kdyn != 0 : (MODE == 0 || MODE == 1);
    // knob STFT_CPS (scripts/kbench.py stftcps*): an upper bound on the chunked walk's pairs per slot
    const PairWalk w = pair_walk(bulk_pairs, F, cached_grid(capc[0], (const void*)k_stft_pair<N, MODE, 0>, WG, 0, 1LL << 40),
                                 capd, aligned && FUSE_TAIL && want, knob(KNOB_STFT_CPS, 0), j.s);
    auto launch = [&](auto kern, int var, long long pair0, long long cnt) {
        const int capv = cached_grid(capc[var], (const void*)kern, WG, 0, 1LL << 40);
        long long grid = capped_grid(capv, (nch * cnt + F - 1) / F);   // VAR 1 / 2: the persistent XCD walk
        long long chunk = 0;
        if (var == 0 || var == 3) {   // the walk's chunk over this launch's pairs (the split launches cover fewer)
            chunk = w.chunk;
            grid = (nch * cnt + chunk - 1) / chunk;
        }
        if (var == 4 || var == 5) grid = dyn_grid(capv);
        if (var == 5) {   // pairs per counter value; knob STFT_RUN overrides (A/B)
            long long rl = knob(KNOB_STFT_RUN, 2);
            if (rl < 1 || rl > 64) rl = 2;
            long long dbs = knob(KNOB_STFT_DBS, 6);   // band: 2^dbs runs per (XCD group, slot) stream (A/B)
            if (dbs < 0 || dbs > 12) dbs = 6;
            chunk = (rl << 40) | dbs;
        }
        if (var == 3) {   // run length (pairs), a divisor of cps; knob STFT_RUN overrides (A/B)
            const long long cps = w.chunk / F;
            long long rl = knob(KNOB_STFT_RUN, cps);
            if (rl < 1 || cps % rl) rl = cps;
            chunk |= rl << 40;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(WG), 0, j.s, sig, n, nch, ch_stride, frames, hop, pair0,
                           cnt, j.win, out, out_ch_stride, j.row_pitch, pN, tN, chunk, sink, w.ctrs, MelArgs{});
    };
    // Magnitude rows with whole-chunk hops: the dynamic walk in runs of 2
    // pairs on a ring (VAR 5): 3.357 vs 3.440 ms (VAR 4) vs 3.501 ms (chunked)
    // for 32 ch x 10 min, runs of 1 / 3 / 4 / 8 / 16 slower; power and complex
    // rows measured 1-4 % slower with it (profiles/r03_kbench_dynring.jsonl).
    // knob STFT_DYN = 1 / 2 forces VAR 4 / VAR 5 (A/B)
    const bool dring = kdyn >= 0 ? kdyn == 2 : MODE == 0;
    if (w.dyn) stat_inc(STAT_STFT_DYN);
    if (w.dyn && dring && hop == 256) {
        if constexpr (Geo<N>::T == 64) launch(k_stft_pair<N, MODE, 5>, 5, 0LL, ppc);
    } else if (w.dyn) {
        if constexpr (Geo<N>::T == 64) launch(k_stft_pair<N, MODE, 4>, 4, 0LL, ppc);
    } else if (aligned && FUSE_TAIL && ring) {
        if constexpr (Geo<N>::T == 64) launch(k_stft_pair<N, MODE, 3>, 3, 0LL, ppc);
    } else if (aligned && FUSE_TAIL) {
        launch(k_stft_pair<N, MODE, 0>, 0, 0LL, ppc);
    } else {
        if (mpc > 0) {
            if (aligned) launch(k_stft_pair<N, MODE, 0>, 0, 0LL, mpc);
            else launch(k_stft_pair<N, MODE, 1>, 1, 0LL, mpc);
        }
        if (tpc > 0) launch(k_stft_pair<N, MODE, 2>, 2, mpc, tpc);
    }
    return hipGetLastError();
}

}  // namespace vvh
