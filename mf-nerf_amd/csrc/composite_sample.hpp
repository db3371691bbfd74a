// composite_sample.hpp -- test-time compositing of one sample onto a ray's running sums
// (volumerendering.cu:206-249), shared by composite_test_kernel (vren_composite.hip) and the fused
// test-time renderer (render.hip).
#pragma once
#include "common.hpp"

namespace mfn {

struct RaySums { float T, O, D, R, G, B; };  // transmittance; opacity, depth and rgb so far

// Adds the sample (sigma, delta, t, rgb c0 c1 c2); true when the ray's transmittance has fallen to thr.
__device__ __forceinline__ bool composite_sample(RaySums& s, float sigma, float delta, float t, float c0, float c1,
                                                 float c2, float thr) {
    const float a = 1.0f - fast_exp(-sigma * delta);
    const float w = a * s.T;
    s.R = fmaf(w, c0, s.R); s.G = fmaf(w, c1, s.G); s.B = fmaf(w, c2, s.B);
    s.D = fmaf(w, t, s.D);
    s.O += w;
    s.T *= 1.0f - a;
    return s.T <= thr;
}

}  // namespace mfn
