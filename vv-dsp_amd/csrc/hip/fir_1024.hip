// fir_1024.hip -- the two overlap-save routes of N = 1024 with le = 256 (taps <=
// 257, config 4): k_fir_r32 (fir_r32.hpp), the default, and k_fir_bulk_reg
// (fir_bulk_reg.hpp) behind knob FIR_R32 = 0.
#include "fir_bulk_reg.hpp"
#include "fir_launch.hpp"
#include "fir_r32.hpp"

#include <cstdint>

namespace vvh {

// The 32 x 32 transform split: one LDS transpose per FFT instead of two.
hipError_t fir_route_r32(const FirJob& j, const FirGeo& g) {
    // 8 B pairs (PAIRED) for 8 B aligned channels; dword loads and stores otherwise
    const bool paired = ((uintptr_t)j.x & 7) == 0 && ((uintptr_t)j.y & 7) == 0 && (j.x_stride & 1) == 0 &&
                        (j.y_stride & 1) == 0;
    static std::atomic<int> capc_32;
    const long long couples = (j.nch * g.ppc + 1) / 2;
    const int grid = capped_grid(capc_32, (const void*)k_fir_r32<true>, 256, (couples + 3) / 4);
    const float2* t1024 = twiddle_table(1024);
    if (!t1024) return hipErrorOutOfMemory;
    if (grid < 1) return hipSuccess;
    stat_inc(STAT_FIR_R32);
    hipLaunchKernelGGL((paired ? k_fir_r32<true> : k_fir_r32<false>), dim3(grid), dim3(256), 0, j.s, j.H, j.x, j.y,
                       j.nch, j.x_stride, j.y_stride, g.ppc, t1024, j.n, j.prefix, j.taps - 1, g.qf, g.ql);
    return hipGetLastError();
}

// The edge pairs [0, qf) and [ql, ppc) take the kernel's bounds-checked branch
// (round 2 ran them as a second, latency-bound launch: 11 us of config 4's 237).
hipError_t fir_route_bulk_reg(const FirJob& j, const FirGeo& g) {
    constexpr int N = 1024;
    const float2* pN = pass_twiddles(N);
    if (!pN) return hipErrorOutOfMemory;
    static std::atomic<int> capc_r, capc_rd;
    const long long pairs = j.nch * g.ppc;
    // the dynamic band walk (k_fir_bulk_reg<N, true>): 0.2385 -> 0.2323 ms
    // for config 4, same buffers, bit-identical (profiles/r03_kbench_fir_dyn.jsonl);
    // knob FIR_DYN = 0 keeps the static XCD walk (A/B)
    // Small jobs (< 8 pairs per wave slot of the persistent grid), a grid
    // too small for 8 XCD groups, or no counter block (pool exhausted, a
    // first use inside a graph capture) take the static walk.
    unsigned* ctrs = nullptr;
    int cap_d = 0;
    if (knob(KNOB_FIR_DYN, -1) != 0) {
        cap_d = cached_grid(capc_rd, (const void*)k_fir_bulk_reg<N, true>, 256, 0, 1LL << 40);
        if (cap_d >= 8 && pairs >= 8LL * 4 * cap_d) ctrs = stream_counters(j.s);
    }
    const long long grid =
        ctrs ? dyn_grid(cap_d) : capped_grid(capc_r, (const void*)k_fir_bulk_reg<N>, 256, (pairs + 3) / 4);
    stat_inc(ctrs ? STAT_FIR_DYN : STAT_FIR_STATIC);
    hipLaunchKernelGGL((ctrs ? k_fir_bulk_reg<N, true> : k_fir_bulk_reg<N, false>), dim3((unsigned)grid), dim3(256), 0,
                       j.s, j.H, j.x, j.y, j.nch, j.x_stride, j.y_stride, g.ppc, 0LL, pN, j.n, j.prefix, j.taps - 1, g.qf, g.ql,
                       ctrs);
    return hipGetLastError();
}

}  // namespace vvh
