// interp_rule.hpp -- the reference's interpolation rules between neighbouring
// samples (src/resample/interpolate.c:15-19, :44-62), one copy for the fixed-ratio
// resampler (resample_kernels.hip) and the arbitrary-position kernel
// (interp_kernels.hip).  Every product and every sum is rounded to f32 on its
// own, as the reference's build (-ffp-contract=off) rounds them.
#pragma once
#include <hip/hip_runtime.h>

namespace vvh {

// (1 - t) a + t b: an empty asm on each product keeps hipcc from contracting them into the sum
__device__ inline float interp_linear_rule(float t, float a, float b) {
    float u = 1.0f - t;
    asm volatile("" : "+v"(u));
    float pa = u * a;
    asm volatile("" : "+v"(pa));
    float pb = t * b;
    asm volatile("" : "+v"(pb));
    return pa + pb;
}

// a product that must reach the sum after it as a rounded f32 (the same idiom)
__device__ inline float interp_product(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// The four Hermite basis values of the fraction t (interpolate.c:54-60), in the
// reference's operation order: h00 = (2 t3 - 3 t2) + 1, h10 = (t3 - 2 t2) + t,
// h01 = -2 t3 + 3 t2, h11 = t3 - t2.
struct CubicBasis {
    float h00, h10, h01, h11;
};
__device__ inline CubicBasis interp_cubic_basis(float t) {
    const float t2 = interp_product(t, t);
    const float t3 = interp_product(t2, t);
    const float a2 = interp_product(2.0f, t3);
    const float b3 = interp_product(3.0f, t2);
    const float b2 = interp_product(2.0f, t2);
    const float n2 = interp_product(-2.0f, t3);
    CubicBasis h;
    h.h00 = (a2 - b3) + 1.0f;
    h.h10 = (t3 - b2) + t;
    h.h01 = n2 + b3;
    h.h11 = t3 - t2;
    return h;
}

// Catmull-Rom between p1 and p2 with tangents m1 = (p2 - p0) / 2, m2 = (p3 - p1) / 2
// (interpolate.c:51-62): ((h00 p1 + h10 m1) + h01 p2) + h11 m2
__device__ inline float interp_cubic_rule(const CubicBasis& h, float p0, float p1, float p2, float p3) {
    const float m1 = interp_product(0.5f, p2 - p0);
    const float m2 = interp_product(0.5f, p3 - p1);
    const float s0 = interp_product(h.h00, p1);
    const float s1 = interp_product(h.h10, m1);
    const float s2 = interp_product(h.h01, p2);
    const float s3 = interp_product(h.h11, m2);
    return ((s0 + s1) + s2) + s3;
}

}  // namespace vvh
