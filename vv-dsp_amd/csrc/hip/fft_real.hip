// fft_real.hip -- launches of the fused power-of-two R2C and C2R kernels
// (k_r2c, k_r2c_small, k_c2r, k_c2r_small; fft_real.hpp), real length 4..16384.
// One unit for both directions: compiled apart, k_r2c<M> and k_c2r<M> at
// M = 2, 4, 8, 512, 1024 come out as other device code.
#include "fft_real.hpp"
#include "pow2_launch.hpp"

namespace vvh {

template <int M>
static hipError_t run_r2c(const float* in, float2* out, long long batch, long long in_dist,
                          long long out_dist, hipStream_t s) {
    const Pow2Tables tb(M, true);
    if (!tb.ok()) return hipErrorOutOfMemory;
    constexpr int WG = Wg<M>::value, F = Wg<M>::F;
    static std::atomic<int> capc;
    // one resident workgroup per CU: measured 15-20 % faster than the 3 the
    // LDS/VGPR budget allows (the partial-line n/2+1 rows combine better with
    // fewer concurrent writers; profiles/r01_kbench_occupancy.jsonl)
    const int cap = cached_grid(capc, (const void*)k_r2c<M>, WG, 0, 1LL << 40, 1);
    // knob REAL_TPW = 1: one transform per slot, not persistent (A/B; 3.6 % slower
    // at 256 points, 9.8 % at 4096, equal at 1024: profiles/r05_ab2_real_grid.jsonl)
    const int grid = slot_grid(batch, F, cap, knob(KNOB_REAL_TPW, 0) != 1);
    if (grid < 1) return hipSuccess;
    if constexpr (M >= 16 && M <= 64) {
        // 32..128 real points, dense rows: the staged kernel -- 0.404 / 0.479 / 0.285 ->
        // 0.198 / 0.215 / 0.221 ms for 2^27 points, bit-identical
        // (profiles/r05_ab2_r2c_small.jsonl); knob R2C_SMALL = 0 keeps k_r2c (A/B)
        if (in_dist == 2 * M && out_dist == M + 1 && ((uintptr_t)in & 15) == 0 && knob(KNOB_R2C_SMALL, 1) == 1) {
            hipLaunchKernelGGL(k_r2c_small<M>, dim3(slot_grid(batch, 256 / Geo<M>::T, 0, false)), dim3(256), 0, s, in,
                               out, batch, tb.pass, tb.tab, tb.post2M);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL(k_r2c<M>, dim3(grid), dim3(WG), 0, s, in, out, batch, in_dist, out_dist, tb.pass, tb.tab,
                       tb.post2M);
    return hipGetLastError();
}

template <int M>
static hipError_t run_c2r(const float2* in, float* out, long long batch, long long in_dist,
                          long long out_dist, hipStream_t s) {
    const Pow2Tables tb(M, true);
    if (!tb.ok()) return hipErrorOutOfMemory;
    constexpr int WG = Wg<M>::value, F = Wg<M>::F;
    static std::atomic<int> capc;
    const int cap = cached_grid(capc, (const void*)k_c2r<M>, WG, 0, 1LL << 40);
    // n <= 1024: one transform per slot, not persistent -- 256 points -6.1 %, 1024
    // -4.4 %, 4096 equal, bit-identical (profiles/r05_ab2_real_grid.jsonl); knob
    // REAL_TPW = 0 / 1 forces the persistent / one-per-slot grid (A/B)
    const int grid = slot_grid(batch, F, cap, knob(KNOB_REAL_TPW, M <= 512 ? 1 : 0) != 1);
    if (grid < 1) return hipSuccess;
    if constexpr (M >= 16 && M <= 64) {
        // 32..128 real points, dense rows: the staged kernel (knob REAL_SMALL = 0 keeps k_c2r, A/B)
        if (in_dist == M + 1 && out_dist == 2 * M && ((uintptr_t)out & 15) == 0 && knob(KNOB_REAL_SMALL, 1) == 1) {
            hipLaunchKernelGGL(k_c2r_small<M>, dim3(slot_grid(batch, 256 / Geo<M>::T, 0, false)), dim3(256), 0, s, in,
                               out, batch, tb.pass, tb.tab, tb.post2M, 1.0f / (float)M);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL(k_c2r<M>, dim3(grid), dim3(WG), 0, s, in, out, batch, in_dist, out_dist, tb.pass, tb.tab,
                       tb.post2M, 1.0f / (float)M);
    return hipGetLastError();
}

// real 16384: the 8192-point complex kernel geometry (512 threads, 70 KB of LDS)
bool r2c_supported(long long n) {
    const long long mx = 2 * knob(KNOB_C2C_MAX, 8192);   // A/B: 4096 keeps real 16384 on the promote + four-step path
    return n >= 4 && n <= mx && n <= 16384 && (n & (n - 1)) == 0;
}

hipError_t launch_r2c(long long n, const float* in, float2* out, long long batch, long long in_dist,
                      long long out_dist, hipStream_t s) {
    return pow2_dispatch<2, 8192>(n / 2, [&](auto m) {
        return run_r2c<decltype(m)::value>(in, out, batch, in_dist, out_dist, s);
    });
}

hipError_t launch_c2r(long long n, const float2* in, float* out, long long batch, long long in_dist,
                      long long out_dist, hipStream_t s) {
    return pow2_dispatch<2, 8192>(n / 2, [&](auto m) {
        return run_c2r<decltype(m)::value>(in, out, batch, in_dist, out_dist, s);
    });
}

}  // namespace vvh
