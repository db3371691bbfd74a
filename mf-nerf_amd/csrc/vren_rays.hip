// vren_rays.hip -- the ray-level utilities of the reference's `vren` op set and their C-ABI entry
// points: ray/box intersection (intersection.cu), Morton codes and the occupancy bitfield's packing
// (raymarching.cu:62-161).
#include "ray_march.hpp"
#include "vren_launch.hpp"

using namespace mfn;
using namespace mfn_vren;

namespace {

// ------------------------------------------------------------------ ray / AABB (intersection.cu:5-56)
__global__ void ray_aabb_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                const float* __restrict__ centers, const float* __restrict__ half_sizes,
                                int64_t n_rays, int64_t n_vox, int max_hits, int32_t* __restrict__ hit_cnt,
                                float* __restrict__ hits_t, int64_t* __restrict__ hits_idx) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const Ray ray = load_ray(o, d, r);
    float* ht = hits_t + r * max_hits * 2;
    int64_t* hi = hits_idx + r * max_hits;
    for (int k = 0; k < max_hits; ++k) { ht[2 * k] = -1.0f; ht[2 * k + 1] = -1.0f; hi[k] = -1; }
    int cnt = 0;
    for (int64_t v = 0; v < n_vox; ++v) {
        const float cx = centers[3 * v], cy = centers[3 * v + 1], cz = centers[3 * v + 2];
        const float hx = half_sizes[3 * v], hy = half_sizes[3 * v + 1], hz = half_sizes[3 * v + 2];
        float t1, t2;
        slab_test(ray, cx, cy, cz, hx, hy, hz, t1, t2);
        if (t2 > 0) {
            if (cnt < max_hits) { ht[2 * cnt] = fmaxf(t1, 0.0f); ht[2 * cnt + 1] = t2; hi[cnt] = v; }
            cnt++;
        }
    }
    hit_cnt[r] = cnt;
    // the reference sorts all max_hits slots by t1 (intersection.cu:95-97): unfilled slots (t1=-1)
    // come first, then the real hits ascending.  Insertion sort of the k real hits, then shift right.
    const int k = min(cnt, max_hits);
    for (int i = 1; i < k; ++i) {
        const float a = ht[2 * i], b = ht[2 * i + 1]; const int64_t c = hi[i];
        int j = i - 1;
        while (j >= 0 && ht[2 * j] > a) { ht[2 * j + 2] = ht[2 * j]; ht[2 * j + 3] = ht[2 * j + 1]; hi[j + 1] = hi[j]; --j; }
        ht[2 * j + 2] = a; ht[2 * j + 3] = b; hi[j + 1] = c;
    }
    const int sh = max_hits - k;
    if (sh > 0 && k > 0) {
        for (int i = k - 1; i >= 0; --i) {
            ht[2 * (i + sh)] = ht[2 * i]; ht[2 * (i + sh) + 1] = ht[2 * i + 1]; hi[i + sh] = hi[i];
        }
        for (int i = 0; i < sh; ++i) { ht[2 * i] = -1.0f; ht[2 * i + 1] = -1.0f; hi[i] = -1; }
    }
}

// ------------------------------------------------------------------ morton / packbits (raymarching.cu:62-161)
__global__ void morton_kernel(const int32_t* __restrict__ c, int64_t n, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (int32_t)morton3((uint32_t)c[3 * i], (uint32_t)c[3 * i + 1], (uint32_t)c[3 * i + 2]);
}

__global__ void morton_invert_kernel(const int32_t* __restrict__ idx, int64_t n, int32_t* __restrict__ c) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = (uint32_t)idx[i];
    c[3 * i] = (int32_t)morton3_invert(v);
    c[3 * i + 1] = (int32_t)morton3_invert(v >> 1);
    c[3 * i + 2] = (int32_t)morton3_invert(v >> 2);
}

// one thread per output byte: two 16-B loads of the 8 floats, one byte store
__global__ void packbits_kernel(const float* __restrict__ grid, int64_t n_bytes, float thr,
                                const float* __restrict__ thr_dev, uint8_t* __restrict__ bits) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_bytes) return;
    const float t = thr_dev ? *thr_dev : thr;
    const float4 a = reinterpret_cast<const float4*>(grid)[2 * n];
    const float4 b = reinterpret_cast<const float4*>(grid)[2 * n + 1];
    uint32_t v = (a.x > t) | ((a.y > t) << 1) | ((a.z > t) << 2) | ((a.w > t) << 3) |
                 ((b.x > t) << 4) | ((b.y > t) << 5) | ((b.z > t) << 6) | ((b.w > t) << 7);
    bits[n] = (uint8_t)v;
}

}  // namespace

extern "C" {

int mfnerf_ray_aabb_intersect(const float* rays_o, const float* rays_d, const float* centers,
                              const float* half_sizes, int64_t n_rays, int64_t n_voxels, int max_hits,
                              int32_t* hit_cnt, float* hits_t, int64_t* hits_voxel_idx, mfnerf_stream_t stream) {
    if (n_rays < 0 || n_voxels < 0 || max_hits <= 0) { mfn_set_error("ray_aabb_intersect: bad sizes"); return MFN_ERR_INVALID; }
    if (n_rays == 0) return MFN_OK;
    if (!rays_o || !rays_d || !centers || !half_sizes || !hit_cnt || !hits_t || !hits_voxel_idx) {
        mfn_set_error("ray_aabb_intersect: null pointer"); return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(ray_aabb_kernel, dim3(blocks_for(n_rays, RAY_BLOCK)), dim3(RAY_BLOCK), 0, stream,
                       rays_o, rays_d, centers, half_sizes, n_rays, n_voxels, max_hits, hit_cnt, hits_t,
                       hits_voxel_idx);
    return mfn_check_launch("ray_aabb_intersect");
}

int mfnerf_morton3d(const int32_t* coords, int64_t n, int32_t* out, mfnerf_stream_t stream) {
    if (n < 0) { mfn_set_error("morton3D: bad size"); return MFN_ERR_INVALID; }
    if (n == 0) return MFN_OK;
    if (!coords || !out) { mfn_set_error("morton3D: null pointer"); return MFN_ERR_INVALID; }
    hipLaunchKernelGGL(morton_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, coords, n, out);
    return mfn_check_launch("morton3D");
}

int mfnerf_morton3d_invert(const int32_t* idx, int64_t n, int32_t* coords, mfnerf_stream_t stream) {
    if (n < 0) { mfn_set_error("morton3D_invert: bad size"); return MFN_ERR_INVALID; }
    if (n == 0) return MFN_OK;
    if (!idx || !coords) { mfn_set_error("morton3D_invert: null pointer"); return MFN_ERR_INVALID; }
    hipLaunchKernelGGL(morton_invert_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, stream, idx, n, coords);
    return mfn_check_launch("morton3D_invert");
}

int mfnerf_packbits(const float* grid, int64_t n_bytes, float thr, const float* thr_dev, uint8_t* bitfield,
                    mfnerf_stream_t stream) {
    if (n_bytes < 0) { mfn_set_error("packbits: bad size"); return MFN_ERR_INVALID; }
    if (n_bytes == 0) return MFN_OK;
    if (!grid || !bitfield) { mfn_set_error("packbits: null pointer"); return MFN_ERR_INVALID; }
    if (((uintptr_t)grid) & 15) { mfn_set_error("packbits: density grid must be 16-byte aligned"); return MFN_ERR_INVALID; }
    hipLaunchKernelGGL(packbits_kernel, dim3(blocks_for(n_bytes, 256)), dim3(256), 0, stream, grid, n_bytes, thr,
                       thr_dev, bitfield);
    return mfn_check_launch("packbits");
}

}  // extern "C"

