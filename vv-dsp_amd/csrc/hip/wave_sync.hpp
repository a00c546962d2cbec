// wave_sync.hpp -- the barrier between LDS writes and reads of one wave, for
// every kernel in which a wave reads only what its own lanes wrote (fft_core.hpp's
// xsync of a transform owned by one wave, the LPC and pitch row kernels).
#pragma once
#include <hip/hip_runtime.h>

namespace vvh {

// LDS ops of one wave execute in order; only the compiler must not move them.
// No memory fence and no s_barrier: see xsync (fft_core.hpp).
__device__ __forceinline__ void wave_sync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

}  // namespace vvh
