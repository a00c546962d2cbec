// stft_launch.hpp -- what the STFT launch units (stft_kernels.hip, the router,
// and stft_pair / stft_small / stft_mel.hip) share: the family
// launchers they call in each other, and the one copy of every launch rule
// that more than one of them follows.  Host code only; private to these units.
#pragma once
#include "vvhip_internal.hpp"

namespace vvh {

// launch_stft's arguments; row_pitch as the kernels take it (floats from one row's start to the next)
struct StftJob {
    const float* sig;
    long long n, nch, ch_stride, frames, hop;
    const float* win;
    void* out;
    long long out_ch_stride, row_pitch;
    hipStream_t s;
};
// The family launchers (mode 0 magnitude, 1 complex, 2 power rows).  Each is
// instantiated in one unit only, so every kernel and grid cache exists once.
template <int N, int MODE> hipError_t run_stft_pair(const StftJob& j);    // Geo<N>::CAN_PAIR: stft_pair.hip (<1024, 2>: stft_mel.hip)
template <int N, int MODE> hipError_t run_stft_small(const StftJob& j);   // nfft 256 and 4096: stft_small.hip

// The 32 x 32 kernels' shape (k_stft_r32): hop 256, 8 B aligned channel starts.
// Power rows and the fused log-mel / MFCC rows share this rule, so the fused
// rows always come from the same FFT as the power rows they must equal.
inline bool stft_r32_ok(const StftJob& j) {
    return j.hop == 256 && ((uintptr_t)j.sig & 7) == 0 && (j.nch == 1 || (j.ch_stride & 1) == 0);
}

// The input side of k_stft_pair's LDS-DMA span path (T >= 64): 16 B aligned
// spans of N + hop floats, hop at most hop_max (what the kernel's span buffer holds).
inline bool stft_span_ok(const StftJob& j, long long hop_max) {
    return j.hop % 4 == 0 && j.hop <= hop_max && ((uintptr_t)j.sig & 15) == 0 && (j.ch_stride & 3) == 0;
}

// One k_stft_r32<MODE> launch (kern): `wg` threads walking `cpb` frame-pair
// couples at a time (4 on 256 threads; the mel modes 8 on 512, one copy of the
// tables), persistent grid.  With dynamic LDS (the mel plan's tables) the
// occupancy changes from call to call and the grid is not cached.
template <int MODE, class K>
hipError_t launch_r32(K kern, int wg, int cpb, size_t dyn_lds, Stat stat, const StftJob& j, const float2* tw1024,
                      const MelArgs& mel) {
    static std::atomic<int> cache;   // per MODE: per kernel
    const long long couples = (j.nch * ((j.frames + 1) / 2) + 1) / 2, need = (couples + cpb - 1) / cpb;
    const int grid = dyn_lds ? capped_grid(persistent_grid((const void*)kern, wg, dyn_lds, 1LL << 40), need)
                             : capped_grid(cache, (const void*)kern, wg, need);
    if (grid < 1) return hipSuccess;
    stat_inc(stat);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(wg), dyn_lds, j.s, j.sig, j.n, j.nch, j.ch_stride, j.frames, j.win,
                       (float*)j.out, j.out_ch_stride, j.row_pitch, tw1024, mel);
    return hipGetLastError();
}

// How a bulk k_stft_pair launch walks `pairs` frame pairs, F transform slots per
// workgroup.  The power rows and the fused mel rows must follow one rule to stay
// bit-identical, and this is it.
//   chunked (VAR 0 / 3): NOT persistent -- one workgroup per `cps` pairs per slot
//     (chunk = cps * F), so the hardware dispatcher balances the CUs and the
//     launch has no straggler tail (measured 8-13 % faster than the persistent
//     walk at 16-64 pairs per slot; profiles/r01_kbench_chunk.jsonl).  Small jobs
//     use fewer pairs per slot: just enough that the grid fits the `cap` resident
//     workgroups once (one round, every wave pipelining its pairs) instead of a
//     few long chains or several short rounds.  cps_max > 0 bounds cps (A/B).
//   dynamic (VAR 4 / 5), when wanted and the job has >= 16 pairs per resident
//     wave of the dynamic kernel (capd: at least a workgroup per XCD group):
//     persistent, the same number of blocks per XCD group, counters from
//     stream_counters.  No counter block (pool exhausted, or first use inside
//     a capture): the chunked walk, bit-identical.
struct PairWalk {
    bool dyn;
    long long grid, chunk;
    unsigned* ctrs;
};
inline PairWalk pair_walk(long long pairs, int F, int cap, int capd, bool want_dyn, long long cps_max,
                          hipStream_t s) {
    PairWalk w{false, 0, 0, nullptr};
    if (want_dyn && capd >= 8 && pairs >= 16LL * F * capd) w.ctrs = stream_counters(s);
    w.dyn = w.ctrs != nullptr;
    if (w.dyn) {
        w.grid = dyn_grid(capd);
        return w;
    }
    long long cps = (pairs + (long long)F * cap - 1) / ((long long)F * cap);
    cps = cps < 1 ? 1 : (cps > 16 ? 16 : cps);
    if (cps_max > 0 && cps > cps_max) cps = cps_max;
    w.chunk = cps * F;
    w.grid = (pairs + w.chunk - 1) / w.chunk;
    return w;
}

}  // namespace vvh
