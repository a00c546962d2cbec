// framing_index.hpp -- the reflection rule of centred frames (framing.c:21-56),
// shared by the frame gather (framing_kernels.hip) and the fused framed LPC
// (lpc_kernels.hip): one copy, so both read the same sample for an index.
#pragma once
#include <hip/hip_runtime.h>

namespace vvh {

// reflection about the ends, period 2n for far indices
__host__ __device__ __forceinline__ long long reflect_index(long long idx, long long n) {
    if (idx < 0) {
        long long a = -idx - 1;
        if (a >= n) {
            const long long period = 2 * n;
            a %= period;
            if (a >= n) a = period - 1 - a;
        }
        return a;
    }
    if (idx >= n) {
        long long r = n - 1 - (idx - n);
        if (r < 0) {
            r = -r - 1;
            if (r >= n) {
                const long long period = 2 * n;
                r %= period;
                if (r >= n) r = period - 1 - r;
            }
        }
        return r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
    }
    return idx;
}

}  // namespace vvh
