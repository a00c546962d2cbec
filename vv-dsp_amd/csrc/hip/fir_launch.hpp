// fir_launch.hpp -- what the overlap-save launch units (fir_ols.hip, the router
// and the route of every block size; fir_1024.hip, the two N = 1024 routes)
// share.  Host code only; private to these units.
#pragma once
#include "vvhip_internal.hpp"

namespace vvh {

// launch_fir_ols's arguments
struct FirJob {
    long long taps;
    const float2* H;
    const float* x;
    float* y;
    long long n, nch, x_stride, y_stride;
    const float* prefix;
    hipStream_t s;
};

// 16 B aligned channels: only then do the 16 x 16 x 4 kernels (k_fir_pair<N, true>'s
// 16 B LDS-DMA spans, k_fir_bulk_reg) run bulk pairs
inline bool fir_span_aligned(const FirJob& j) { return ((uintptr_t)j.x & 15) == 0 && (j.x_stride & 3) == 0; }

// The N = 1024, le = 256 routes (fir_1024.hip); every pair of every channel,
// edge pairs included, in one launch.
// k_fir_r32: the 32 x 32 transform split; bulk pairs need no alignment.
hipError_t fir_route_r32(const FirJob& j, const FirGeo& g);
// k_fir_bulk_reg with its dynamic or static walk: 16 B aligned channels with bulk pairs.
hipError_t fir_route_bulk_reg(const FirJob& j, const FirGeo& g);

}  // namespace vvh
