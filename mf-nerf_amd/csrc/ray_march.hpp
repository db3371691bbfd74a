// ray_march.hpp -- one ray against the occupancy grid (intersection.cu, raymarching.cu): the slab
// test, the per-sample march step and the skip past an empty cell.  The training marchers and the
// test-time marcher (vren_march.hip), the ray/box kernel (vren_rays.hip) and the fused test-time
// renderer (render.hip) all call these, so "the same arithmetic" (the renderer's contract is bit-for-bit
// equality with the staged path) is one piece of source.  fp contract: common.hpp.
#pragma once
#include "common.hpp"

namespace mfn {

// raymarching.cu:11-13
__device__ __forceinline__ float calc_dt(float t, float exp_step_factor, int max_samples, int grid_size, float scale) {
    return clampf(t * exp_step_factor, MFN_SQRT3 / (float)max_samples, MFN_SQRT3 * 2 * scale / (float)grid_size);
}

// One occupancy lookup (raymarching.cu:205-220).  Returns the occupancy bit and the cell.
struct Cell { int nx, ny, nz; float mip_bound; bool occ; };

__device__ __forceinline__ Cell lookup_cell(float x, float y, float z, float dt, int cascades, int grid_size,
                                            float scale, const uint8_t* __restrict__ bitfield) {
    const uint32_t g3 = (uint32_t)grid_size * grid_size * grid_size;
    const int mip = max(mip_from_pos(x, y, z, cascades), mip_from_dt(dt, grid_size, cascades));
    Cell c;
    c.mip_bound = fminf(scalbnf(1.0f, mip - 1), scale);
    const float inv = 1 / c.mip_bound;
    const float gs = (float)grid_size, gm1 = (float)grid_size - 1.0f;
    c.nx = (int)clampf(0.5f * fmaf(x, inv, 1.0f) * gs, 0.0f, gm1);
    c.ny = (int)clampf(0.5f * fmaf(y, inv, 1.0f) * gs, 0.0f, gm1);
    c.nz = (int)clampf(0.5f * fmaf(z, inv, 1.0f) * gs, 0.0f, gm1);
    const uint32_t idx = (uint32_t)mip * g3 + morton3((uint32_t)c.nx, (uint32_t)c.ny, (uint32_t)c.nz);
    c.occ = (bitfield[idx >> 3] >> (idx & 7)) & 1u;
    return c;
}

// A ray: origin, direction and the direction's reciprocal.
struct Ray { float ox, oy, oz, dx, dy, dz, dxi, dyi, dzi; };

template <typename Index>
__device__ __forceinline__ Ray load_ray(const float* __restrict__ o, const float* __restrict__ d, Index r) {
    Ray ray;
    ray.ox = o[3 * r]; ray.oy = o[3 * r + 1]; ray.oz = o[3 * r + 2];
    ray.dx = d[3 * r]; ray.dy = d[3 * r + 1]; ray.dz = d[3 * r + 2];
    ray.dxi = 1.0f / ray.dx; ray.dyi = 1.0f / ray.dy; ray.dzi = 1.0f / ray.dz;
    return ray;
}

// The slab test of one box (intersection.cu:30-40): entry t1 and exit t2, both -1 on a miss.  What a
// caller makes of an exit behind the origin or an entry before the near plane is its own.
__device__ __forceinline__ void slab_test(const Ray& ray, float cx, float cy, float cz, float hx, float hy, float hz,
                                          float& t1, float& t2) {
    const float tminx = (cx - hx - ray.ox) * ray.dxi, tminy = (cy - hy - ray.oy) * ray.dyi,
                tminz = (cz - hz - ray.oz) * ray.dzi;
    const float tmaxx = (cx + hx - ray.ox) * ray.dxi, tmaxy = (cy + hy - ray.oy) * ray.dyi,
                tmaxz = (cz + hz - ray.oz) * ray.dzi;
    t1 = fmaxf(fmaxf(fminf(tminx, tmaxx), fminf(tminy, tmaxy)), fminf(tminz, tmaxz));
    t2 = fminf(fminf(fmaxf(tminx, tmaxx), fmaxf(tminy, tmaxy)), fmaxf(tminz, tmaxz));
    if (t1 > t2) { t1 = -1.0f; t2 = -1.0f; }
}

// DDA skip target (raymarching.cu:225-229)
__device__ __forceinline__ float skip_target(float t, const Cell& c, float x, float y, float z, const Ray& ray,
                                             float gsi) {
    const float tx = fmaf(fmaf(fmaf(0.5f, signf(ray.dx), (float)c.nx + 0.5f) * gsi, 2.0f, -1.0f), c.mip_bound, -x) * ray.dxi;
    const float ty = fmaf(fmaf(fmaf(0.5f, signf(ray.dy), (float)c.ny + 0.5f) * gsi, 2.0f, -1.0f), c.mip_bound, -y) * ray.dyi;
    const float tz = fmaf(fmaf(fmaf(0.5f, signf(ray.dz), (float)c.nz + 0.5f) * gsi, 2.0f, -1.0f), c.mip_bound, -z) * ray.dzi;
    return t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
}

// What a march needs of the occupancy grid, built once per thread from the kernel's parameters (any
// struct with these field names) before its loop.
struct MarchGrid {
    const uint8_t* bitfield; int cascades; float scale; float exp_step; int grid_size; int max_samples;
    float gsi;       // 1 / grid_size
    float dt_scale;  // what calc_dt gets as `scale`
};
// training (raymarching.cu:190-279): calc_dt gets the scene's scale
template <typename P>
__device__ __forceinline__ MarchGrid train_grid(const P& p) {
    return {p.bitfield, p.cascades, p.scale, p.exp_step, p.grid_size, p.max_samples, 1.0f / (float)p.grid_size,
            p.scale};
}
// test time (raymarching.cu:335-404): the reference's quirk, cascades passed as calc_dt's `scale`
template <typename P>
__device__ __forceinline__ MarchGrid test_grid(const P& p) {
    return {p.bitfield, p.cascades, p.scale, p.exp_step, p.grid_size, p.max_samples, 1.0f / (float)p.grid_size,
            (float)p.cascades};
}

__device__ __forceinline__ float march_dt(const MarchGrid& g, float t) {
    return calc_dt(t, g.exp_step, g.max_samples, g.grid_size, g.dt_scale);
}

// The march step at t (raymarching.cu:205-220): the point, its step and its cell.
struct MarchPoint { float x, y, z, dt; Cell c; };

__device__ __forceinline__ MarchPoint march_point(const MarchGrid& g, const Ray& ray, float t) {
    MarchPoint m;
    m.x = fmaf(t, ray.dx, ray.ox); m.y = fmaf(t, ray.dy, ray.oy); m.z = fmaf(t, ray.dz, ray.oz);
    m.dt = march_dt(g, t);
    m.c = lookup_cell(m.x, m.y, m.z, m.dt, g.cascades, g.grid_size, g.scale, g.bitfield);
    return m;
}

// Past the empty cell of m, the march step at t (raymarching.cu:225-232): steps of dt up to the first
// chain point at or beyond the DDA target.  Returns the new t.
__device__ __forceinline__ float skip_empty(const MarchGrid& g, const Ray& ray, const MarchPoint& m, float t) {
    const float tt = skip_target(t, m.c, m.x, m.y, m.z, ray, g.gsi);
    do { t += march_dt(g, t); } while (t < tt);
    return t;
}

// The same chain, left as soon as it reaches t2 (a march ends there whatever t is), and ended at t2 by
// a step below t's resolution (a degenerate ray): the trip count has a bound that no far target moves.
__device__ __forceinline__ float skip_empty_to(const MarchGrid& g, const Ray& ray, const MarchPoint& m, float t,
                                               float t2) {
    const float tt = skip_target(t, m.c, m.x, m.y, m.z, ray, g.gsi);
    do {
        const float tp = t;
        t += march_dt(g, t);
        if (t == tp) t = t2;
    } while (t < tt && t < t2);
    return t;
}

}  // namespace mfn
