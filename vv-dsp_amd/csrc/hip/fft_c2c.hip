// fft_c2c.hip -- launches of the batched power-of-two C2C kernel (k_c2c,
// fft_c2c.hpp), N = 2..8192.
#include "fft_c2c.hpp"
#include "pow2_launch.hpp"

namespace vvh {

template <int N, bool FWD>
static hipError_t run_c2c(const float2* in, float2* out, long long batch, long long in_dist,
                          long long out_dist, float scale, hipStream_t s) {
    const Pow2Tables tb(N);
    if (!tb.ok()) return hipErrorOutOfMemory;
    constexpr int WG = Wg<N>::value, F = Wg<N>::F;
    static std::atomic<int> capc;
    const int grid_cap = cached_grid(capc, (const void*)k_c2c<N, FWD>, WG, 0, 1LL << 40);
    // 256 <= N <= 4096: one transform per wave slot, a grid of batch / F workgroups
    // (not persistent), so the dispatcher hands out the next workgroup as one ends:
    // config 2 (65536 x 1024) 0.1847 -> 0.1766 ms on the same buffers, 256 / 2048
    // points -3.6 / -4.5 %, 4096 -0.5 %; 64 points +10 % and 8192 +32 % keep the
    // persistent grid (profiles/r05_ab2_c2c_grid.jsonl).  Knob C2C_TPW = t > 0:
    // t transforms per wave slot; 0: the persistent grid (A/B)
    // 16..128 points with dense rows: the same one-transform grid, each wave's
    // 1024-point block moved as 16 B per lane and re-laid through LDS (k_c2c ONE,
    // G::T < 16): 32 / 64 / 128 points 0.650 / 0.332 / 0.230 -> 0.177 ms for 2^26
    // points (0.21 / 0.40 / 0.58 -> 0.76; profiles/r05_ab2_c2c_small.jsonl), bit-identical;
    // knob C2C_SMALL = 0 keeps the persistent grid (A/B)
    const bool small = N >= 16 && N <= 128 && in_dist == N && out_dist == N && ((uintptr_t)in & 15) == 0 &&
                       ((uintptr_t)out & 15) == 0 && knob(KNOB_C2C_SMALL, 1) == 1;
    const long long tpw = knob(KNOB_C2C_TPW, (N >= 256 && N <= 4096) || small ? 1 : -1);
    const int grid = tpw > 0 ? slot_grid(batch, F * tpw, 0, false) : slot_grid(batch, F, grid_cap, true);
    if (grid < 1) return hipSuccess;
    // one transform per slot: the loop-free kernel (no prefetch registers: 58 instead
    // of 98 VGPRs at 1024 points, 6 workgroups per CU): equal at 256 / 1024 points,
    // -1.3 % at 2048, -6.4 % at 4096 (profiles/r05_ab2_c2c_grid.jsonl); knob C2C_ONE = 0
    // keeps the looping kernel (A/B)
    // (two consecutive transforms per slot on this kernel measured +0.4 / +11 / +22 %
    // at 1024 / 2048 / 4096 points)
    if (tpw == 1 && (long long)grid * F >= batch && knob(KNOB_C2C_ONE, 1) == 1 && (N >= 256 || small)) {   // (every slot's one transform in the grid)
        hipLaunchKernelGGL((k_c2c<N, FWD, true>), dim3(grid), dim3(WG), 0, s, in, out, batch, in_dist, out_dist,
                           tb.pass, tb.tab, scale);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_c2c<N, FWD>), dim3(grid), dim3(WG), 0, s, in, out, batch, in_dist, out_dist, tb.pass,
                       tb.tab, scale);
    return hipGetLastError();
}

// 8192: one workgroup of 512 threads per transform, the transform in 70 KB of
// LDS (gfx950 gives one workgroup up to 160 KB).  16384 would need 1024
// threads at <= 128 VGPRs and spills: it stays on the two-pass four-step.
bool c2c_supported(long long n) {
    const long long mx = knob(KNOB_C2C_MAX, 8192);   // A/B: 4096 sends 8192 to the two-pass four-step
    return n >= 2 && n <= mx && n <= 8192 && (n & (n - 1)) == 0;
}

hipError_t launch_c2c(long long n, int fwd, const float2* in, float2* out, long long batch,
                      long long in_dist, long long out_dist, float scale, hipStream_t s) {
    return pow2_dispatch<2, 8192>(n, [&](auto nn) {
        constexpr int N = decltype(nn)::value;
        return fwd ? run_c2c<N, true>(in, out, batch, in_dist, out_dist, scale, s)
                   : run_c2c<N, false>(in, out, batch, in_dist, out_dist, scale, s);
    });
}

}  // namespace vvh
