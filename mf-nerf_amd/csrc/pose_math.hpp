// pose_math.hpp -- Rodrigues' formula as the reference writes it (datasets/ray_utils.py
// axisangle_to_R: R(w) = I + sin(t)/t K + (1 - cos t)/t^2 K^2, K the skew matrix of w,
// t = |w| + 1e-7) and the transposed Jacobian of w -> R(w) u, in fp32.  Host and device: the same
// text is what pose.hip's kernels run and what a host program can check against fp64.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MFN_HD __host__ __device__ __forceinline__
#else
#define MFN_HD inline
#endif

namespace mfn_pose {

constexpr float GUARD = 1e-7f;          // the reference's guard at w = 0
constexpr float SERIES_BELOW = 0.25f;   // t under which the coefficient derivatives use their series

// The coefficients of R(w) and their derivatives with respect to t.
//   a = sin(t)/t,  b = (1 - cos t)/t^2 = 0.5 (sin(t/2)/(t/2))^2 (no cancellation at small t),
//   a' = (t cos t - sin t)/t^2,  b' = (t sin t - 2(1 - cos t))/t^3.
// Both derivatives cancel in fp32 at small t (a' is a difference of O(t) terms that leaves O(t^3)),
// so under SERIES_BELOW they are the Taylor series
//   a' = -t/3 + t^3/30 - t^5/840,   b' = -t/12 + t^3/180 - t^5/6720
// whose first dropped terms (t^7/45360, t^7/403200) are under 2e-8 of the leading one at t = 0.25;
// from there up the closed forms lose at most ~3e-6 relative, on terms that enter J^T g scaled by
// |w| (a') and |w|^2 (b').
struct Coef { float a, b, da, db; };

MFN_HD Coef coefficients(float t) {
    Coef c;
    const float h = 0.5f * t;
    const float sh = sinf(h) / h;
    c.a = sinf(t) / t;
    c.b = 0.5f * (sh * sh);
    if (t < SERIES_BELOW) {
        const float t2 = t * t;
        c.da = t * (-1.0f / 3.0f + t2 * (1.0f / 30.0f - t2 * (1.0f / 840.0f)));
        c.db = t * (-1.0f / 12.0f + t2 * (1.0f / 180.0f - t2 * (1.0f / 6720.0f)));
    } else {
        const float s = sinf(t), co = cosf(t), sh2 = sinf(h);
        c.da = (t * co - s) / (t * t);
        c.db = (t * s - 4.0f * (sh2 * sh2)) / (t * t * t);
    }
    return c;
}

MFN_HD void cross3(const float* x, const float* y, float* o) {
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}
MFN_HD float dot3(const float* x, const float* y) { return fmaf(x[2], y[2], fmaf(x[1], y[1], x[0] * y[0])); }

// What one image's rays share: w, the coefficients at t = |w| + GUARD and dt/dw = w/|w| (0 at w = 0,
// the subgradient torch autograd takes for the norm).
struct Axis {
    float w[3], n[3];
    Coef c;
};

MFN_HD Axis axis_of(const float* w) {
    Axis A;
    const float len = sqrtf(fmaf(w[2], w[2], fmaf(w[1], w[1], w[0] * w[0])));
    const float inv = len > 0.0f ? 1.0f / len : 0.0f;
    for (int k = 0; k < 3; ++k) { A.w[k] = w[k]; A.n[k] = w[k] * inv; }
    A.c = coefficients(len + GUARD);
    return A;
}

// J(w, u)^T g for f(w) = R(w) u = u + a w x u + b w x (w x u):
//   a (u x g) + b ((w x u) x g + u x (g x w)) + (w/|w|) (a' g.(w x u) + b' g.(w x (w x u)))
MFN_HD void jt_g(const Axis& A, const float* u, const float* g, float* out) {
    float c[3], ug[3], cg[3], gw[3], ugw[3], wc[3];
    cross3(A.w, u, c);
    cross3(u, g, ug);
    cross3(c, g, cg);
    cross3(g, A.w, gw);
    cross3(u, gw, ugw);
    cross3(A.w, c, wc);
    const float radial = fmaf(A.c.db, dot3(g, wc), A.c.da * dot3(g, c));
    for (int k = 0; k < 3; ++k) out[k] = fmaf(A.n[k], radial, fmaf(A.c.b, cg[k] + ugw[k], A.c.a * ug[k]));
}

// R(w) (row-major 3x3).  K^2 = w w^T - |w|^2 I.  At w = 0 it is the identity exactly.
MFN_HD void rotation(const Axis& A, float* R) {
    const float x = A.w[0], y = A.w[1], z = A.w[2], a = A.c.a, b = A.c.b;
    const float xx = x * x, yy = y * y, zz = z * z;
    R[0] = 1.0f - b * (yy + zz); R[1] = fmaf(b, x * y, -(a * z)); R[2] = fmaf(b, x * z, a * y);
    R[3] = fmaf(b, x * y, a * z); R[4] = 1.0f - b * (xx + zz); R[5] = fmaf(b, y * z, -(a * x));
    R[6] = fmaf(b, x * z, -(a * y)); R[7] = fmaf(b, y * z, a * x); R[8] = 1.0f - b * (xx + yy);
}

}  // namespace mfn_pose
