// input_grad.hip -- the loss gradient with respect to the field's inputs: dL/dx through the
// multiresolution grid encoding (tcnn's input gradient of GridEncoding, Linear interpolation) and
// its per-ray reduction to dL/drays_o, dL/drays_d (custom_functions.py:103-112, the backward of
// RayMarcher) for camera-pose refinement (train.py:91-94, --optimize_ext).
//
// With pos = fmaf(scale_l, x01, 0.5), g = floor(pos), w = pos - g (level_geo) and the corner c of
// level l at table index idx_c (corner_index), the encoding's output is
//     out[l,f] = sum_c prod_e wt_e(c) table[idx_c][f],   wt_e(c) = w_e if bit e of c else 1 - w_e,
// so
//     dL/dx_d = (1/x_range) sum_l scale_l sum_f dL_dout[l,f] sum_c sgn_d(c) prod_{e != d} wt_e(c) table[idx_c][f]
// with sgn_d(c) = +1 where bit d of c is set, else -1.  The corner sum is taken as four differences
// along d (corner pairs c, c ^ (1 << d)), each weighted by the other two axes' weights.
//
// Lane mapping: as grid_fw_kernel, 4 lanes per sample, each lane 4 consecutive levels -- its 8
// incoming gradients are two 16-B loads, and all 32 of its corner gathers are issued before any is
// used (the encode is bound by per-lane gather addresses, grid_fw.hip).  The four lanes' partial
// 3-vectors are added by two xor-shuffles (a fixed order).
#include "common.hpp"
#include "grid_geo.hpp"
#include "../../include/mfnerf.h"

using namespace mfn;
using namespace mfn_grid;

int mfn_check_grid_desc(const mfnerf_grid_desc* d, const char* what);  // grid_fw.hip

namespace {

constexpr int IG_BLOCK = 256;
constexpr int IG_LEVELS = 4;  // levels per lane

// One (sample, level), shared by both kernels, in two phases: the gathers ...
struct LevelCorners {
    LevelGeo L;
    __half2 v[8];
};

__device__ __forceinline__ LevelCorners level_gather(const mfnerf_grid_desc& D, const __half2* __restrict__ table,
                                                     int l, float x, float y, float z) {
    LevelCorners G;
    G.L = level_geo(D.scale[l], x, y, z);
    const __half2* tab = table + D.offset[l];
#pragma unroll
    for (int c = 0; c < 8; ++c)
        G.v[c] = tab[corner_index(D, l, G.L.g[0] + (c & 1), G.L.g[1] + ((c >> 1) & 1), G.L.g[2] + ((c >> 2) & 1))];
    return G;
}

// ... and the derivative of the level's contribution sum_f g_f out[l,f] with respect to pos
// (3 values, fp32; the caller multiplies by scale_l / x_range).
__device__ __forceinline__ void level_dpos(const LevelCorners& G, float g0, float g1, float* d) {
    float t[8];  // the corner's value contracted with the incoming gradient
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float2 f = __half22float2(G.v[c]);
        t[c] = fmaf(g1, f.y, g0 * f.x);
    }
    const float wx = G.L.w[0], wy = G.L.w[1], wz = G.L.w[2];
    const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
    d[0] = fmaf(wy * wz, t[7] - t[6], fmaf(uy * wz, t[5] - t[4], fmaf(wy * uz, t[3] - t[2], (uy * uz) * (t[1] - t[0]))));
    d[1] = fmaf(wx * wz, t[7] - t[5], fmaf(ux * wz, t[6] - t[4], fmaf(wx * uz, t[3] - t[1], (ux * uz) * (t[2] - t[0]))));
    d[2] = fmaf(wx * wy, t[7] - t[3], fmaf(ux * wy, t[6] - t[2], fmaf(wx * uy, t[5] - t[1], (ux * uy) * (t[4] - t[0]))));
}

// One lane's share of a sample: levels 4 grp .. 4 grp + 3, all gathers first.  acc += scale_l * d.
__device__ __forceinline__ void sample_group_dx(const mfnerf_grid_desc& D, const __half2* __restrict__ table, int grp,
                                                float x, float y, float z, const float* __restrict__ dy_row,
                                                float* acc) {
    const float4 ga = reinterpret_cast<const float4*>(dy_row)[2 * grp];
    const float4 gb = reinterpret_cast<const float4*>(dy_row)[2 * grp + 1];
    const float g[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
    LevelCorners G[IG_LEVELS];
#pragma unroll
    for (int k = 0; k < IG_LEVELS; ++k) G[k] = level_gather(D, table, grp * IG_LEVELS + k, x, y, z);
#pragma unroll
    for (int k = 0; k < IG_LEVELS; ++k) {
        float d[3];
        level_dpos(G[k], g[2 * k], g[2 * k + 1], d);
        const float sc = D.scale[grp * IG_LEVELS + k];
        acc[0] = fmaf(sc, d[0], acc[0]);
        acc[1] = fmaf(sc, d[1], acc[1]);
        acc[2] = fmaf(sc, d[2], acc[2]);
    }
}

// (a) per-sample gradient.  4 lanes per sample (a sample's lanes are consecutive: xor 1, 2 stay in it).
__global__ __launch_bounds__(IG_BLOCK) void grid_bw_input_kernel(const float* __restrict__ X, int64_t n,
                                                                 const int32_t* __restrict__ n_dev, float x_min,
                                                                 float x_range, const mfnerf_grid_desc D,
                                                                 const __half2* __restrict__ table,
                                                                 const float* __restrict__ dL_dout,
                                                                 float* __restrict__ dL_dx) {
    const int groups = D.n_levels / IG_LEVELS, row = 2 * D.n_levels;
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const float inv_range = 1.0f / x_range;
    const int sub = threadIdx.x & 3;
    // the wave's 16 samples stay together through the loop (the shuffles need all four lanes of a
    // sample); lanes past the end work on a clamped sample and store nothing
    const int64_t per_pass = (int64_t)gridDim.x * (IG_BLOCK / 4);
    for (int64_t i0 = (int64_t)blockIdx.x * (IG_BLOCK / 4); i0 < nn; i0 += per_pass) {
        const int64_t i = i0 + (threadIdx.x >> 2);
        const int64_t ic = min<int64_t>(i, nn - 1);
        const float x = (X[3 * ic] - x_min) / x_range;
        const float y = (X[3 * ic + 1] - x_min) / x_range;
        const float z = (X[3 * ic + 2] - x_min) / x_range;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int grp = sub; grp < groups; grp += 4) sample_group_dx(D, table, grp, x, y, z, dL_dout + ic * row, acc);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[k] += __shfl_xor(acc[k], 1, 64);
            acc[k] += __shfl_xor(acc[k], 2, 64);
        }
        if (sub == 0 && i < nn) {
            dL_dx[3 * i] = acc[0] * inv_range;
            dL_dx[3 * i + 1] = acc[1] * inv_range;
            dL_dx[3 * i + 2] = acc[2] * inv_range;
        }
    }
}

// (c) per-ray reduction: one wave per ray, 16 samples x 4 level groups per pass over the ray's
// segment.  Every lane keeps its own running sums (its samples in order), and the 64 lanes' sums are
// folded by a fixed xor tree: no float atomics, the same bits on every run.  One wave per workgroup:
// rays run from 0 to several hundred samples, and with four rays per workgroup the longest held
// the other three waves' slots (281 -> 245 us at the Lego step, profiles/r08_input_grad.json).
constexpr int RAY_BLOCK = 64, RAY_WAVES = RAY_BLOCK / 64;

__global__ __launch_bounds__(RAY_BLOCK) void rays_input_grad_kernel(const float* __restrict__ X,
                                                                   const float* __restrict__ ts,
                                                                   const float* __restrict__ dL_dfeat,
                                                                   const float* __restrict__ dL_ddirs,
                                                                   const int64_t* __restrict__ rays_a, int64_t n_rays,
                                                                   int64_t n_samples, float x_min, float x_range,
                                                                   const mfnerf_grid_desc D,
                                                                   const __half2* __restrict__ table,
                                                                   float* __restrict__ dL_drays_o,
                                                                   float* __restrict__ dL_drays_d) {
    const int groups = D.n_levels / IG_LEVELS, row = 2 * D.n_levels;
    const int lane = threadIdx.x & 63, sub = lane & 3, slot = lane >> 2;
    const float inv_range = 1.0f / x_range;
    const int64_t r = (int64_t)blockIdx.x * RAY_WAVES + (threadIdx.x >> 6);
    if (r >= n_rays) return;  // (wave-uniform)
    const int64_t ray = rays_a[3 * r];
    int64_t start = rays_a[3 * r + 1], cnt = rays_a[3 * r + 2];
    if (ray < 0 || ray >= n_rays) return;
    // a segment is clamped into the sample buffers: nothing is read out of bounds on a malformed row
    if (start < 0 || start > n_samples) { start = 0; cnt = 0; }
    cnt = max<int64_t>(0, min<int64_t>(cnt, n_samples - start));
    float o[3] = {0.f, 0.f, 0.f}, dd[3] = {0.f, 0.f, 0.f};
    for (int64_t s0 = 0; s0 < cnt; s0 += 16) {
        const bool live = s0 + slot < cnt;
        const int64_t s = start + min<int64_t>(s0 + slot, cnt - 1);
        const float x = (X[3 * s] - x_min) / x_range;
        const float y = (X[3 * s + 1] - x_min) / x_range;
        const float z = (X[3 * s + 2] - x_min) / x_range;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int grp = sub; grp < groups; grp += 4) sample_group_dx(D, table, grp, x, y, z, dL_dfeat + s * row, acc);
        const float t = ts[s];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = live ? acc[k] * inv_range : 0.0f;
            const float e = (live && sub == 0) ? dL_ddirs[3 * s + k] : 0.0f;
            o[k] += a;
            dd[k] += live ? fmaf(t, a, e) : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            o[k] += __shfl_xor(o[k], off, 64);
            dd[k] += __shfl_xor(dd[k], off, 64);
        }
    if (lane < 3) {
        const float vo = lane == 0 ? o[0] : lane == 1 ? o[1] : o[2];
        const float vd = lane == 0 ? dd[0] : lane == 1 ? dd[1] : dd[2];
        dL_drays_o[3 * ray + lane] = vo;
        dL_drays_d[3 * ray + lane] = vd;
    }
}

}  // namespace

extern "C" {

int mfnerf_grid_encode_bw_input(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                const mfnerf_grid_desc* desc, const void* table_f16, const float* dL_dout,
                                float* dL_dx, mfnerf_stream_t stream) {
    int st = mfn_check_grid_desc(desc, "grid_encode_bw_input");
    if (st) return st;
    if (n < 0) { mfn_set_error("grid_encode_bw_input: bad size"); return MFN_ERR_INVALID; }
    if (n == 0) return MFN_OK;
    if (!x || !table_f16 || !dL_dout || !dL_dx) {
        mfn_set_error("grid_encode_bw_input: null pointer"); return MFN_ERR_INVALID;
    }
    const int64_t want = div_up<int64_t>(n, IG_BLOCK / 4);
    const int64_t blocks = want < 8192 ? want : 8192;
    hipLaunchKernelGGL(grid_bw_input_kernel, dim3((unsigned)blocks), dim3(IG_BLOCK), 0, stream, x, n, n_dev, x_min,
                       x_range, *desc, (const __half2*)table_f16, dL_dout, dL_dx);
    return mfn_check_launch("grid_encode_bw_input");
}

int mfnerf_rays_input_grad(const float* xyzs, const float* ts, const float* dL_dfeat, const float* dL_ddirs,
                           const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float x_min, float x_range,
                           const mfnerf_grid_desc* desc, const void* table_f16, float* dL_drays_o,
                           float* dL_drays_d, mfnerf_stream_t stream) {
    int st = mfn_check_grid_desc(desc, "rays_input_grad");
    if (st) return st;
    if (n_rays < 0 || n_samples < 0) { mfn_set_error("rays_input_grad: bad size"); return MFN_ERR_INVALID; }
    if (n_rays == 0) return MFN_OK;
    if (!rays_a || !dL_drays_o || !dL_drays_d || !table_f16 ||
        (n_samples > 0 && (!xyzs || !ts || !dL_dfeat || !dL_ddirs))) {
        mfn_set_error("rays_input_grad: null pointer"); return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(rays_input_grad_kernel, dim3((unsigned)div_up<int64_t>(n_rays, RAY_WAVES)), dim3(RAY_BLOCK), 0,
                       stream, xyzs, ts, dL_dfeat, dL_ddirs, rays_a, n_rays, n_samples, x_min, x_range, *desc,
                       (const __half2*)table_f16, dL_drays_o, dL_drays_d);
    return mfn_check_launch("rays_input_grad");
}

}  // extern "C"
