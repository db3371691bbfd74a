// frame.hip -- the two ends of a viewer frame around the test-time renderer (render.hip): a camera
// pose to one whole view's rays (datasets/ray_utils.py:8-47 + :50-70 as show_gui.py:74-75 runs them
// per frame), and the renderer's sums to a displayable 8-bit frame -- the background blend
// (rendering.py:93-94), the colour quantisation of train.py:223 and depth2img (train.py:48-53) with
// the Turbo table of turbo_table.hpp.  Pose, rays and frames stay on the device and nothing is
// decided on the host, so camera_rays -> mfnerf_render_test_fused -> frame_finish is one linear
// chain that a graph captures once and replays per pose.
//
// Both are bandwidth-trivial beside the render (about 40 B per pixel in, 3-15 B out), so they are
// written for plain coalescing, not tuned: camera_rays takes one output float per lane, frame_finish
// one 32-bit word of the 8-bit frame (four consecutive channel values, which straddle two pixels) per
// lane, so a wave's stores are contiguous in every output.
#include <cmath>

#include "common.hpp"
#include "turbo_table.hpp"
#include "../../include/mfnerf.h"

using namespace mfn;

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = 2048;         // grid cap; the kernels stride over the rest
constexpr int RANGE_PARTS = 256;         // at most this many workgroups' (min, max) pairs in the workspace
constexpr int64_t MAX_PIXELS = 1 << 29;  // 3 * n and the stride past it stay below 2^31

unsigned grid_for(int64_t items) {
    const int64_t want = div_up<int64_t>(items, BLOCK);
    return (unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
}

// ray_utils.py:35 + :62,68 for the whole view: element e = 3 * pixel + axis of rays_o / rays_d
__global__ __launch_bounds__(BLOCK)
void camera_rays_kernel(float fx, float fy, float cx, float cy, const float* __restrict__ pose, uint32_t W,
                        uint32_t n3, float* __restrict__ rays_o, float* __restrict__ rays_d) {
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t e = blockIdx.x * BLOCK + threadIdx.x; e < n3; e += stride) {
        const uint32_t i = e / 3u, a = e - 3u * i;
        const uint32_t v = i / W, u = i - v * W;
        const float dx = (((float)u - cx) + 0.5f) / fx;
        const float dy = (((float)v - cy) + 0.5f) / fy;
        const float* r = pose + 4 * a;  // row a of the (3,4) camera-to-world matrix
        // rays_d = directions @ c2w[:, :3].T with the camera z = 1 (data.hip's order of the sum)
        rays_d[e] = fmaf(1.0f, r[2], fmaf(dy, r[1], dx * r[0]));
        rays_o[e] = r[3];
    }
}

// (x * 255).astype(uint8) of train.py:223 / :50: the product in fp32, truncated toward zero; where
// numpy's cast is undefined or wraps (a product outside [0, 256), NaN) the value is clamped to
// [0, 255] and NaN gives 0
__device__ __forceinline__ uint32_t quantise(float x) { return (uint32_t)(int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f); }

// one word of the 8-bit frame; the last word of a frame whose 3 * n is no multiple of 4 byte by byte
__device__ __forceinline__ void store_word(uint8_t* __restrict__ u8, uint32_t w, uint32_t n3, uint32_t packed) {
    if (4u * w + 3u < n3) {
        reinterpret_cast<uint32_t*>(u8)[w] = packed;
    } else {
        for (uint32_t e = 4u * w; e < n3; ++e) u8[e] = (uint8_t)(packed >> (8u * (e - 4u * w)));
    }
}

// mode 0: the blend of rendering.py:93-94, rgb + bg * (1 - opacity), and its quantisation
__global__ __launch_bounds__(BLOCK)
void frame_colour_kernel(const float* __restrict__ opacity, const float* __restrict__ rgb, uint32_t n3, float bg,
                         uint8_t* __restrict__ u8, float* __restrict__ f32) {
    const uint32_t words = div_up(n3, 4u), stride = gridDim.x * BLOCK;
    for (uint32_t w = blockIdx.x * BLOCK + threadIdx.x; w < words; w += stride) {
        uint32_t packed = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t e = 4u * w + j;
            if (e < n3) {
                const float c = rgb[e] + bg * (1.0f - opacity[e / 3u]);
                if (f32) f32[e] = c;
                packed |= quantise(c) << (8u * j);
            }
        }
        store_word(u8, w, n3, packed);
    }
}

// min and max of this lane's values over the workgroup (every lane gets them); sh holds 8 floats
__device__ __forceinline__ void block_range(float& mn, float& mx, float* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[wave] = mn; sh[4 + wave] = mx; }
    __syncthreads();
    mn = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
    mx = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
}

// depth.min(), depth.max() of train.py:49, first stage: workgroup b's pair into parts[2b], parts[2b+1].
// Every workgroup of the launch holds at least one pixel and writes its pair, so the second stage
// reads nothing this call did not write; min and max do not depend on the order they are taken in.
__global__ __launch_bounds__(BLOCK)
void depth_range_kernel(const float* __restrict__ depth, uint32_t n, float* __restrict__ parts) {
    __shared__ float sh[8];
    float mn = INFINITY, mx = -INFINITY;
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const float d = depth[i];
        mn = fminf(mn, d);
        mx = fmaxf(mx, d);
    }
    block_range(mn, mx, sh);
    if (threadIdx.x == 0) { parts[2 * blockIdx.x] = mn; parts[2 * blockIdx.x + 1] = mx; }
}

// mode 1, depth2img (train.py:48-53): x = (depth - mn) / (mx - mn), one IEEE division;
// k = uint8(x * 255); the pixel is TURBO_RGB[k], red first.  mx == mn (the reference's 0 / 0): k = 0.
__global__ __launch_bounds__(BLOCK)
void frame_depth_kernel(const float* __restrict__ depth, uint32_t n, const float* __restrict__ parts, int n_parts,
                        uint8_t* __restrict__ u8, float* __restrict__ f32) {
    __shared__ float sh[8];
    float mn = INFINITY, mx = -INFINITY;
    if ((int)threadIdx.x < n_parts) { mn = parts[2 * threadIdx.x]; mx = parts[2 * threadIdx.x + 1]; }
    block_range(mn, mx, sh);
    const float range = mx - mn;
    const bool flat = !(range > 0.0f);
    const uint32_t n3 = 3u * n, words = div_up(n3, 4u), stride = gridDim.x * BLOCK;
    for (uint32_t w = blockIdx.x * BLOCK + threadIdx.x; w < words; w += stride) {
        // the word's four values belong to pixel p0 and, past its last channel, to p0 + 1
        const uint32_t p0 = (4u * w) / 3u, p1 = p0 + 1u < n ? p0 + 1u : p0;
        const uint32_t k0 = flat ? 0u : quantise((depth[p0] - mn) / range);
        const uint32_t k1 = flat ? 0u : quantise((depth[p1] - mn) / range);
        uint32_t packed = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t e = 4u * w + j;
            if (e < n3) {
                const uint32_t p = e / 3u, c = e - 3u * p;
                const uint32_t b = mfn_frame::TURBO_RGB[p == p0 ? k0 : k1][c];
                if (f32) f32[e] = (float)b / 255.0f;  // show_gui.py:99
                packed |= b << (8u * j);
            }
        }
        store_word(u8, w, n3, packed);
    }
}

}  // namespace

extern "C" {

int mfnerf_camera_rays(const float* K4, const float* pose, int64_t W, int64_t H, float* rays_o, float* rays_d,
                       mfnerf_stream_t stream) {
    if (W <= 0 || H <= 0 || W > MAX_PIXELS || H > MAX_PIXELS || W * H > MAX_PIXELS) {
        mfn_set_error("camera_rays: bad image size W=%lld H=%lld (W * H must be in 1..2^29)", (long long)W,
                      (long long)H);
        return MFN_ERR_INVALID;
    }
    if (!K4 || !pose || !rays_o || !rays_d) { mfn_set_error("camera_rays: null pointer"); return MFN_ERR_INVALID; }
    if (!(K4[0] != 0.0f) || !(K4[1] != 0.0f)) {
        mfn_set_error("camera_rays: bad focal length fx=%g fy=%g", (double)K4[0], (double)K4[1]);
        return MFN_ERR_INVALID;
    }
    const uint32_t n3 = (uint32_t)(3 * W * H);
    hipLaunchKernelGGL(camera_rays_kernel, dim3(grid_for(n3)), dim3(BLOCK), 0, stream, K4[0], K4[1], K4[2], K4[3],
                       pose, (uint32_t)W, n3, rays_o, rays_d);
    return mfn_check_launch("camera_rays");
}

int64_t mfnerf_frame_finish_workspace(void) { return (int64_t)RANGE_PARTS * 2 * sizeof(float); }

int mfnerf_frame_finish(const float* opacity, const float* depth, const float* rgb, int64_t n, int mode, float bg,
                        void* workspace, uint8_t* frame_u8, float* frame_f32, mfnerf_stream_t stream) {
    if (mode != 0 && mode != 1) {
        mfn_set_error("frame_finish: unknown mode %d (0 = colour, 1 = depth)", mode); return MFN_ERR_INVALID;
    }
    if (n < 0 || n > MAX_PIXELS) {
        mfn_set_error("frame_finish: bad n=%lld (0..2^29 pixels)", (long long)n); return MFN_ERR_INVALID;
    }
    if (n == 0) return MFN_OK;
    if (!frame_u8 || (mode == 0 ? (!opacity || !rgb) : (!depth || !workspace))) {
        mfn_set_error("frame_finish: null pointer"); return MFN_ERR_INVALID;
    }
    if (((uintptr_t)frame_u8 & 3u) || ((uintptr_t)workspace & 3u)) {
        mfn_set_error("frame_finish: frame_u8 and workspace must be 4-byte aligned"); return MFN_ERR_INVALID;
    }
    const uint32_t n3 = (uint32_t)(3 * n);
    const unsigned grid = grid_for(div_up<int64_t>(n3, 4));
    if (mode == 0) {
        hipLaunchKernelGGL(frame_colour_kernel, dim3(grid), dim3(BLOCK), 0, stream, opacity, rgb, n3, bg, frame_u8,
                           frame_f32);
    } else {
        const int64_t want = div_up<int64_t>(n, BLOCK);
        const int parts = (int)(want < RANGE_PARTS ? want : RANGE_PARTS);
        hipLaunchKernelGGL(depth_range_kernel, dim3(parts), dim3(BLOCK), 0, stream, depth, (uint32_t)n,
                           (float*)workspace);
        hipLaunchKernelGGL(frame_depth_kernel, dim3(grid), dim3(BLOCK), 0, stream, depth, (uint32_t)n,
                           (const float*)workspace, parts, frame_u8, frame_f32);
    }
    return mfn_check_launch("frame_finish");
}

}  // extern "C"
