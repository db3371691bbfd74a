// render.hip -- the test-time renderer in one persistent launch (rendering.py:46-118 without its
// host loop): ray/box test, occupancy march, grid encode, MFMA field head and compositing, from ray
// origin and direction to opacity / depth / rgb.  No intermediate reaches memory and nothing is
// decided on the host, so the call is legal inside a captured graph.
//
// A wave is one 32-row field tile exactly as in field_fw_kernel (row r = lane & 31, feature half
// h = lane >> 5).  The lane pair (r, 0), (r, 1) owns one ray at a time: both lanes march it with the
// same instructions on the same values (the pair agrees on every decision without a shuffle), lane
// (r, h) interpolates its half of the grid levels straight into the tile's B operands, and lane
// (r, 0) holds the compositing sums.  One trip = every live pair advances to its next occupied
// sample, the wave evaluates the tile, the pairs composite one sample.  A pair whose ray ends
// (terminated, left the box, budget reached) writes it out and takes the next ray index from a
// global counter, one atomic per wave-instruction; it keeps refilling inside the trip until it holds
// a ray with a sample, so rays that miss the box or cross no occupied cell cost a march and no MFMA.
// Every ray's arithmetic is a function of that ray alone (an MFMA column depends on its own B column
// only), so its outputs do not depend on the lane, the wave or the rest of the batch.
#include <cmath>

#include "ray_march.hpp"
#include "composite_sample.hpp"
#include "grid_geo.hpp"
#include "field_fwd.hpp"
#include "../../include/mfnerf.h"

using namespace mfn;
using namespace mfn_grid;
using namespace mfn_field;

namespace {

constexpr float NEAR_DISTANCE = 0.01f;  // rendering.py:8

struct RenderParams {
    const float* o; const float* d; int32_t n_rays;
    const float* center; const float* half_size;
    const uint8_t* bitfield; int cascades; float scale; float exp_step; int grid_size; int max_samples;
    int ray_budget; float T_thr; float x_min, x_range;
    const __half2* table; const _Float16* packed;
    int32_t* queue; float* opacity; float* depth; float* rgb; int32_t* samples; unsigned long long* total;
};

#ifdef MFN_RENDER_PROBE
// probe build only (tools/build_variant.sh EXTRA=-DMFN_RENDER_PROBE=1): MFMA rows issued / valid
__device__ unsigned long long g_probe_rows[2];
#endif

// the queue counter and the sample total start every launch at zero (a kernel, not a memset node:
// see mfn_zero_async)
__global__ void render_init_kernel(int32_t* queue, unsigned long long* total) {
    if (threadIdx.x == 0) *queue = 0;
    if (threadIdx.x == 1) *total = 0ull;
}

// Waves per SIMD = resident workgroups per CU (one wave of each per SIMD).  Unconstrained the kernel
// takes 178 VGPRs + 38 AGPRs at either width (the eight levels' 64 corner gathers in flight): two
// waves.  W = 64: held to three waves (168 registers, 9 spilled) it renders 61.8 instead of 50.5
// frames/s -- the trip is bound by the gathers' latency, which a third wave hides; four waves (128
// registers, 53 spilled): 55.7.  W = 128: two workgroups' fragments (56 KB each) are all a CU's LDS
// holds, and the three-wave register budget without a third wave is slower (49.1 vs 51.0).
constexpr int waves_per_simd(int W) { return W == 64 ? 3 : 2; }

template <int W>
__global__ __launch_bounds__(FIELD_BLOCK) __attribute__((amdgpu_waves_per_eu(waves_per_simd(W), waves_per_simd(W))))
void render_test_kernel(const RenderParams p, const mfnerf_grid_desc D) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* lds = reinterpret_cast<_Float16*>(smem);
    load_frags(lds, p.packed, Geo<W>::N_FW);
    const int lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const uint32_t below = (1u << r) - 1u;
    const MarchGrid g = test_grid(p);
    const float cx = p.center[0], cy = p.center[1], cz = p.center[2];
    const float hx = p.half_size[0], hy = p.half_size[1], hz = p.half_size[2];

    // the pair's ray (identical on both lanes) and, on lanes h == 0, its compositing sums.  They live
    // across trips as plain floats and are handed to the shared functions as a Ray / RaySums made on
    // the spot: as struct members the compiler carries them through the loops in another order, and
    // this kernel's register allocation (three waves, 9 spills) follows that order
    bool have = false;
    int32_t ray = 0, n = 0;
    float ox = 0.f, oy = 0.f, oz = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, dxi = 0.f, dyi = 0.f, dzi = 0.f;
    float t = 0.f, t2 = 0.f;
    float T = 1.f, O = 0.f, Dp = 0.f, R = 0.f, G = 0.f, B = 0.f;
    bool drained = false;             // (wave-uniform) every ray index has been handed out
    unsigned long long evaluated = 0; // (wave-uniform) samples this wave put through the field
#ifdef MFN_RENDER_PROBE
    unsigned long long trips = 0;
#endif

    auto finish = [&]() {
        if (h == 0) {
            p.opacity[ray] = O; p.depth[ray] = Dp;
            p.rgb[3 * (int64_t)ray] = R; p.rgb[3 * (int64_t)ray + 1] = G; p.rgb[3 * (int64_t)ray + 2] = B;
            if (p.samples) p.samples[ray] = n;
        }
        have = false;
    };

    for (;;) {
        // ---- every pair: a ray with its next occupied sample, or no ray and an empty queue
        bool ready = false;
        float sx = 0.f, sy = 0.f, sz = 0.f, sdt = 0.f, st = 0.f;
        for (;;) {
            if (have && !ready) {
                // the test-time march step; the skip also stops at t2, past which the ray ends whatever
                // t is (same samples, and no trip count that depends on a far skip target)
                const Ray ry{ox, oy, oz, dx, dy, dz, dxi, dyi, dzi};
                while (t < t2) {
                    const MarchPoint m = march_point(g, ry, t);
                    if (m.c.occ) {
                        sx = m.x; sy = m.y; sz = m.z; sdt = m.dt; st = t;
                        t += m.dt;
                        ready = true;
                        break;
                    }
                    t = skip_empty_to(g, ry, m, t, t2);
                }
                if (!ready) finish();  // left the box
            }
            const bool need = !have && !drained;
            const uint32_t m = (uint32_t)__ballot(need);  // (both halves carry the same bits)
            if (m == 0) break;
            const int cnt = __popc(m);
            int base = 0;
            if (lane == 0) base = atomicAdd(p.queue, cnt);
            base = __builtin_amdgcn_readfirstlane(base);
            if (base >= p.n_rays - cnt) drained = true;
            if (need) {
                const int32_t idx = base + (int)__popc(m & below);
                if (idx < p.n_rays) {
                    ray = idx;
                    const Ray ry = load_ray(p.o, p.d, (int64_t)idx);
                    ox = ry.ox; oy = ry.oy; oz = ry.oz;
                    dx = ry.dx; dy = ry.dy; dz = ry.dz;
                    dxi = ry.dxi; dyi = ry.dyi; dzi = ry.dzi;
                    float t1, te;
                    slab_test(ry, cx, cy, cz, hx, hy, hz, t1, te);
                    // an exit behind the origin is a miss, as in ray_aabb_kernel; the near clamp of rendering.py:28
                    if (te > 0) t1 = fmaxf(t1, 0.0f);
                    else { t1 = -1.0f; te = -1.0f; }
                    if (t1 >= 0 && t1 < NEAR_DISTANCE) t1 = NEAR_DISTANCE;
                    n = 0;
                    T = 1.f; O = 0.f; Dp = 0.f; R = 0.f; G = 0.f; B = 0.f;
                    t = t1; t2 = te;
                    have = true;
                    // a miss (and a box exit at infinity, which no march would reach): zeros
                    if (!(t1 >= 0) || !(te < INFINITY)) finish();
                }
            }
        }
        const uint32_t live = (uint32_t)__ballot(ready);
        if (live == 0) break;  // the queue is empty and no pair holds a ray
        evaluated += (unsigned)__popc(live);
#ifdef MFN_RENDER_PROBE
        trips += 1;
#endif

        // ---- this lane's half of the levels (grid_fw_kernel's arithmetic), straight into the operands
        TileIn I;
        if (ready) {
            const float x = (sx - p.x_min) / p.x_range;
            const float y = (sy - p.x_min) / p.x_range;
            const float z = (sz - p.x_min) / p.x_range;
            uint32_t u[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                // x[0] element j = feature 8h+j = level 4h + j/2; x[1]: level 8 + 4h + j/2 (load_tile_in)
                const int l = (k < 4 ? 4 * h : 4 + 4 * h) + k;
                const LevelGeo L = level_geo(D.scale[l], x, y, z);
                const __half2* tab = p.table + D.offset[l];
                __half2 v[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    v[c] = tab[corner_index(D, l, L.g[0] + (c & 1), L.g[1] + ((c >> 1) & 1), L.g[2] + ((c >> 2) & 1))];
                float a0 = 0.f, a1 = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float w = corner_weight(L, c);
                    const float2 f = __half22float2(v[c]);
                    a0 = fmaf(w, f.x, a0);
                    a1 = fmaf(w, f.y, a1);
                }
                __half2 hv = __floats2half2_rn(a0, a1);
                u[k] = *reinterpret_cast<uint32_t*>(&hv);
            }
            I.x[0] = *reinterpret_cast<const half8*>(&u[0]);
            I.x[1] = *reinterpret_cast<const half8*>(&u[4]);
            I.d[0] = dx; I.d[1] = dy; I.d[2] = dz;
        } else {
            I.x[0] = half8{}; I.x[1] = half8{};
            I.d[0] = I.d[1] = I.d[2] = 0.0f;
        }

        // ---- the field head on the tile (all 64 lanes)
        FwdTile<W> F;
        forward_tiles<W, false, 1, true>(lds, lane, &I, &ready, &F);

        // ---- the pair's one sample onto its sums
        bool term = false;
        if (ready && h == 0) {
            const float sigma = __expf(F.h0);  // TruncExp forward, as field_fw_kernel stores it
            const float c0 = (float)(_Float16)F.rgb[0], c1 = (float)(_Float16)F.rgb[1], c2 = (float)(_Float16)F.rgb[2];
            RaySums S{T, O, Dp, R, G, B};
            term = composite_sample(S, sigma, sdt, st, c0, c1, c2, p.T_thr);
            T = S.T; O = S.O; Dp = S.D; R = S.R; G = S.G; B = S.B;
        }
        const uint32_t tb = (uint32_t)__ballot(term);  // lanes h == 0 decide for their pairs
        if (ready) {
            n += 1;
            if (((tb >> r) & 1u) || n >= p.ray_budget) finish();
        }
    }
    if (lane == 0 && evaluated) atomicAdd(p.total, evaluated);
#ifdef MFN_RENDER_PROBE
    if (lane == 0) { atomicAdd(&g_probe_rows[0], 32ull * trips); atomicAdd(&g_probe_rows[1], evaluated); }
#endif
}


int cu_count() {
    static const int n = [] {
        int dev = 0, cu = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 256;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu <= 0) return 256;
        return cu;
    }();
    return n;
}

template <int W>
void launch_render(const RenderParams& p, const mfnerf_grid_desc& D, mfnerf_stream_t stream) {
    const int64_t want = div_up<int64_t>(p.n_rays, 32 * (FIELD_BLOCK / 64));
    const int64_t cap = (int64_t)cu_count() * waves_per_simd(W);
    hipLaunchKernelGGL(render_test_kernel<W>, dim3((unsigned)(want < cap ? want : cap)), dim3(FIELD_BLOCK),
                       (size_t)Geo<W>::N_FW * FRAG_HALFS * 2, stream, p, D);
}

}  // namespace

extern "C" {

int mfnerf_render_test_fused(const float* rays_o, const float* rays_d, int64_t n_rays, const float* center,
                             const float* half_size, const uint8_t* bitfield, int cascades, float scale,
                             float exp_step_factor, int grid_size, int max_samples_dt, int ray_budget,
                             float T_threshold, float x_min, float x_range, const mfnerf_grid_desc* desc,
                             const void* table_f16, const void* packed, int rgb_width, int32_t* queue,
                             float* opacity, float* depth, float* rgb, int32_t* samples, int64_t* total_samples,
                             mfnerf_stream_t stream) {
    if (rgb_width != 64 && rgb_width != 128) {
        mfn_set_error("render_test_fused: rgb_width=%d is not supported (64 or 128)", rgb_width);
        return MFN_ERR_INVALID;
    }
    if (!desc) { mfn_set_error("render_test_fused: null grid desc"); return MFN_ERR_INVALID; }
    if (desc->n_levels * desc->n_features != 32 || desc->n_features != 2) {
        mfn_set_error("render_test_fused: the field head takes n_levels * F = 32 grid features with F = 2 "
                      "(n_levels=%d, F=%d)", desc->n_levels, desc->n_features);
        return MFN_ERR_INVALID;
    }
    for (int l = 0; l < desc->n_levels; ++l)
        if (desc->size[l] == 0 || desc->res[l] == 0 || desc->table_kind[l] < 0 || desc->table_kind[l] > 1 ||
            (desc->table_kind[l] == 1 && ((uint64_t)desc->res[l] + 2) * (uint64_t)desc->canon_res >= (1ull << 31))) {
            mfn_set_error("render_test_fused: bad level %d", l); return MFN_ERR_INVALID;
        }
    // (the queue counter overshoots n_rays by at most 32 per resident wave)
    if (n_rays < 0 || n_rays > (int64_t)INT32_MAX - (1 << 24)) {
        mfn_set_error("render_test_fused: bad n_rays=%lld", (long long)n_rays); return MFN_ERR_INVALID;
    }
    if (ray_budget < 1) {
        mfn_set_error("render_test_fused: ray_budget=%d must be at least 1", ray_budget); return MFN_ERR_INVALID;
    }
    if (cascades < 1 || grid_size < 1 || max_samples_dt < 1 || !(x_range > 0.0f)) {
        mfn_set_error("render_test_fused: bad cascades, grid_size, max_samples_dt or x_range"); return MFN_ERR_INVALID;
    }
    if (n_rays == 0) return MFN_OK;
    if (!rays_o || !rays_d || !center || !half_size || !bitfield || !table_f16 || !packed || !queue || !opacity ||
        !depth || !rgb || !total_samples) {
        mfn_set_error("render_test_fused: null pointer"); return MFN_ERR_INVALID;
    }
    RenderParams p;
    p.o = rays_o; p.d = rays_d; p.n_rays = (int32_t)n_rays;
    p.center = center; p.half_size = half_size;
    p.bitfield = bitfield; p.cascades = cascades; p.scale = scale; p.exp_step = exp_step_factor;
    p.grid_size = grid_size; p.max_samples = max_samples_dt;
    p.ray_budget = ray_budget; p.T_thr = T_threshold; p.x_min = x_min; p.x_range = x_range;
    p.table = (const __half2*)table_f16; p.packed = (const _Float16*)packed;
    p.queue = queue; p.opacity = opacity; p.depth = depth; p.rgb = rgb; p.samples = samples;
    p.total = (unsigned long long*)total_samples;
    hipLaunchKernelGGL(render_init_kernel, dim3(1), dim3(64), 0, stream, queue, p.total);
    if (rgb_width == 64) launch_render<64>(p, *desc, stream);
    else launch_render<128>(p, *desc, stream);
    return mfn_check_launch("render_test_fused");
}

#ifdef MFN_RENDER_PROBE
// probe build only: (MFMA rows issued, rows valid) since the last call; synchronises
int mfnerf_render_probe_rows(int64_t* out2) {
    const unsigned long long zero[2] = {0, 0};
    if (hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_probe_rows), 16) != hipSuccess) return MFN_ERR_LAUNCH;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_probe_rows), zero, 16) != hipSuccess) return MFN_ERR_LAUNCH;
    return MFN_OK;
}
#endif

}  // extern "C"
