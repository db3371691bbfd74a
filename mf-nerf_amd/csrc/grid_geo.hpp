// grid_geo.hpp -- one level's cell geometry, corner index and corner weight of the multiresolution
// grid encoding (tcnn HashGrid semantics plus the MixedFeature shared tables), shared by the grid_*.hip
// and render.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfnerf.h"

namespace mfn_grid {

constexpr uint32_t PRIME1 = 2654435761u, PRIME2 = 805459861u;

struct LevelGeo {
    uint32_t g[3];  // floor(pos)
    float w[3];     // pos - floor(pos)
};

// tcnn pos_fract (grid.h): pos = fmaf(scale, x, 0.5f); g = floor(pos); w = pos - g  (Linear)
__device__ __forceinline__ LevelGeo level_geo(float scale, float x, float y, float z) {
    LevelGeo L;
    const float px = fmaf(scale, x, 0.5f), py = fmaf(scale, y, 0.5f), pz = fmaf(scale, z, 0.5f);
    const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    L.g[0] = (uint32_t)(int)fx; L.g[1] = (uint32_t)(int)fy; L.g[2] = (uint32_t)(int)fz;
    L.w[0] = px - fx; L.w[1] = py - fy; L.w[2] = pz - fz;
    return L;
}

// tcnn grid_index: dense strides while res^3 <= size, else the coherent prime hash; `% size`.
// MixedFeature shared tables hash the point's coordinates on the canonical grid.
// floor(x * rc / res) exactly, for x * rc < 2^31 (check_desc): the float quotient is within one of
// it (relative error ~2^-22 on a quotient <= 2^16), one integer correction each way.  A 64-bit
// division here (24 of them per sample-level, inlined) made the scatter kernels' code outgrow the
// instruction cache.
__device__ __forceinline__ uint32_t canon_coord(uint32_t x, uint32_t rc, uint32_t res, float inv) {
    const uint32_t n = x * rc;
    uint32_t q = (uint32_t)((float)n * inv);
    if (q * res > n) --q;
    else if ((q + 1) * res <= n) ++q;
    return q;
}

__device__ __forceinline__ uint32_t corner_index(const mfnerf_grid_desc& D, int l, uint32_t x, uint32_t y,
                                                 uint32_t z) {
    const uint32_t res = D.res[l], size = D.size[l];
    uint32_t idx;
    if (D.table_kind[l] == 1) {
        const uint32_t rc = (uint32_t)D.canon_res;
        const float inv = 1.0f / (float)res;  // one per level after CSE over the corners
        x = canon_coord(x, rc, res, inv);
        y = canon_coord(y, rc, res, inv);
        z = canon_coord(z, rc, res, inv);
        idx = (x * 1u) ^ (y * PRIME1) ^ (z * PRIME2);
    } else if ((uint64_t)res * res * res <= size) {
        idx = x + y * res + z * res * res;
    } else {
        idx = (x * 1u) ^ (y * PRIME1) ^ (z * PRIME2);
    }
    if ((size & (size - 1)) == 0) return idx & (size - 1);
    return idx < size ? idx : idx % size;
}

__device__ __forceinline__ float corner_weight(const LevelGeo& L, int c) {
    float w = 1.0f;
    w *= (c & 1) ? L.w[0] : (1.0f - L.w[0]);
    w *= (c & 2) ? L.w[1] : (1.0f - L.w[1]);
    w *= (c & 4) ? L.w[2] : (1.0f - L.w[2]);
    return w;
}

}  // namespace mfn_grid
