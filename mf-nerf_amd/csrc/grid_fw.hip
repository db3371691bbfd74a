// grid_fw.hip -- multiresolution grid encoding (tiny-cuda-nn HashGrid semantics, plus this repo's
// MixedFeature shared-table variant), forward, on gfx950.  The table gradient: grid_bw_atomic.hip
// (request-shaped atomics, the dense levels), grid_bw_binned.hip (partitioned scatter and accumulate,
// the convert pass and the optimizer on the fixed-point sums).
//
// Forward: 4 lanes per point, each lane owns 4 consecutive levels (8 f16 features = one 16-B
// store), so the 4 lanes of a point write its 64-B output row with one coalesced 64-B burst and
// every lane keeps 32 independent 4-B corner gathers in flight.  Accumulation is fp32 (tcnn
// accumulates in half; the difference is inside the fp16 output rounding).
#include "grid_common.hpp"

using namespace mfn;
using namespace mfn_grid;

namespace {

constexpr int LEVELS_PER_LANE = 4;

// out row = 32 halfs (L=16, F=2); requires n_levels % 4 == 0 and F == 2.
__global__ __launch_bounds__(ENC_BLOCK) void grid_fw_kernel(const float* __restrict__ X, int64_t n,
                                                             const int32_t* __restrict__ n_dev, float x_min,
                                                             float x_range, const mfnerf_grid_desc D,
                                                             const __half2* __restrict__ table,
                                                             __half* __restrict__ out) {
    const int groups = D.n_levels / LEVELS_PER_LANE;
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int64_t total = nn * groups;
    for (int64_t t = (int64_t)blockIdx.x * ENC_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * ENC_BLOCK) {
    const int64_t i = t / groups;
    const int grp = (int)(t - i * groups);
    const float x = (X[3 * i] - x_min) / x_range;
    const float y = (X[3 * i + 1] - x_min) / x_range;
    const float z = (X[3 * i + 2] - x_min) / x_range;
    float acc[2 * LEVELS_PER_LANE];
#pragma unroll
    for (int k = 0; k < LEVELS_PER_LANE; ++k) {
        const int l = grp * LEVELS_PER_LANE + k;
        const LevelGeo L = level_geo(D.scale[l], x, y, z);
        const __half2* tab = table + D.offset[l];
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
        acc[2 * k] = a0; acc[2 * k + 1] = a1;
    }
    __half2 h[LEVELS_PER_LANE];
#pragma unroll
    for (int k = 0; k < LEVELS_PER_LANE; ++k) h[k] = __floats2half2_rn(acc[2 * k], acc[2 * k + 1]);
    uint4 pk;
    pk.x = *reinterpret_cast<uint32_t*>(&h[0]); pk.y = *reinterpret_cast<uint32_t*>(&h[1]);
    pk.z = *reinterpret_cast<uint32_t*>(&h[2]); pk.w = *reinterpret_cast<uint32_t*>(&h[3]);
    reinterpret_cast<uint4*>(out + i * (2 * D.n_levels))[grp] = pk;
    }
}

// Planar (level-major) forward, XCD-partitioned: blocks b and b+8 share an XCD (round-robin
// dispatch), so block group b % 8 owns the levels {l : snake(l % 16) == b % 8} (levels p and 15-p
// for L = 16) for every sample.  Each XCD's L2 then holds only its levels' tables (<= 4 MB of
// fp16 features), instead of every XCD streaming the whole 23 MB table through its 4 MB L2.
// out: n_levels planes of plane_stride half2 (features of level l of sample i at out[l*stride+i]),
// so each group's stores are contiguous.  Placement only affects speed, never the result.

// One (sample, level) of the planar forward in two phases: the gathers (issued for both of the
// lane's levels before any is used) and the interpolation.  Per (y,z) row every lane loads the 8 B
// holding its x-corner -- at idx (dense levels: idx+1 is the x+1 corner unless the index wraps) or
// at idx & ~1 (hashed power-of-two levels: the x+1 corner is idx ^ 1 when x is even), clamped into
// the table -- and loads the x+1 corner singly only where those 8 B miss it, so most rows cost one
// gather lane instead of two (the kernel is bound by per-lane gather addresses).  No branch chooses
// a load shape: round 4 did, per row, and used the row's values inside the branch, so each row's
// gather was waited for before the next one issued -- 8 dependent L2 round trips per lane and
// sample, 0.05 VMEM instructions in flight per wave (PMC r05_v22); and any merge of two shapes'
// results into one register (the compiler's phi copies) waits for the pending load as well.
struct PlanarGather {
    LevelGeo L;
    uint2 u[4];      // row yz: the 8 B holding the x-corner's half2
    uint32_t s[4];   // the x+1 corner's half2 where u misses it
    uint32_t f;      // row yz, bits 3 yz + {0: x-corner is u.y, 1: x+1 corner is in u, 2: ... as u.y}
};

__device__ __forceinline__ PlanarGather planar_gather(const mfnerf_grid_desc& D, const __half2* __restrict__ table,
                                                      int l, float x, float y, float z) {
    PlanarGather G;
    G.L = level_geo(D.scale[l], x, y, z);
    const uint32_t* __restrict__ tab = reinterpret_cast<const uint32_t*>(table + D.offset[l]);
    const uint32_t size = D.size[l], res = D.res[l];
    const bool dense = D.table_kind[l] == 0 && (uint64_t)res * res * res <= size;
    G.f = 0u;
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        const uint32_t gy = G.L.g[1] + (yz & 1), gz = G.L.g[2] + (yz >> 1);
        const uint32_t i0 = corner_index(D, l, G.L.g[0], gy, gz);
        const uint32_t i1 = corner_index(D, l, G.L.g[0] + 1, gy, gz);
        const uint32_t a = min(dense ? i0 : (i0 & ~1u), size - 2u);  // i0 is a or a + 1
        G.u[yz] = *reinterpret_cast<const uint2*>(tab + a);
        const bool in_u = i1 - a < 2u;
        G.s[yz] = 0u;
        if (!in_u) G.s[yz] = tab[i1];
        G.f |= ((i0 != a ? 1u : 0u) | (in_u ? 2u : 0u) | (i1 != a ? 4u : 0u)) << (3 * yz);
    }
    return G;
}

__device__ __forceinline__ __half2 planar_interp(const PlanarGather& G) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        // integer masks, not selects, on the loaded words (a select between two of the struct's
        // loaded values may become a load from a selected address, the struct then in scratch)
        const uint32_t f = G.f >> (3 * yz);
        const uint32_t m0 = 0u - (f & 1u), m1 = 0u - ((f >> 1) & 1u), m2 = 0u - ((f >> 2) & 1u);
        const uint32_t lo = (G.u[yz].x & ~m0) | (G.u[yz].y & m0);
        const uint32_t hu = (G.u[yz].x & ~m2) | (G.u[yz].y & m2);
        const uint32_t hi = (hu & m1) | (G.s[yz] & ~m1);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float w = corner_weight(G.L, 2 * yz + c);
            const float2 v = __half22float2(__builtin_bit_cast(__half2, c ? hi : lo));
            a0 = fmaf(w, v.x, a0);
            a1 = fmaf(w, v.y, a1);
        }
    }
    return __floats2half2_rn(a0, a1);
}

__global__ __launch_bounds__(ENC_BLOCK) void grid_fw_planar_kernel(const float* __restrict__ X, int64_t n,
                                                                    const int32_t* __restrict__ n_dev, float x_min,
                                                                    float x_range, const mfnerf_grid_desc D,
                                                                    const __half2* __restrict__ table,
                                                                    __half2* __restrict__ out, int64_t plane_stride) {
    const int grp = blockIdx.x & 7;
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int nj = 2 * ((D.n_levels + 15) >> 4);
    const int64_t stride = (int64_t)(gridDim.x >> 3) * ENC_BLOCK;
    for (int64_t i = (int64_t)(blockIdx.x >> 3) * ENC_BLOCK + threadIdx.x; i < nn; i += stride) {
        const float x = (X[3 * i] - x_min) / x_range;
        const float y = (X[3 * i + 1] - x_min) / x_range;
        const float z = (X[3 * i + 2] - x_min) / x_range;
        // this group's levels, visited directly: 16m + grp and 16m + 15 - grp (la < lb)
        for (int j = 0; j < nj; j += 2) {
            const int la = 16 * (j >> 1) + grp, lb = 16 * (j >> 1) + 15 - grp;
            if (la >= D.n_levels) continue;
            const bool has_b = lb < D.n_levels;  // (else level la is gathered twice, stored once)
            const PlanarGather Ga = planar_gather(D, table, la, x, y, z);
            const PlanarGather Gb = planar_gather(D, table, has_b ? lb : la, x, y, z);
            out[(int64_t)la * plane_stride + i] = planar_interp(Ga);
            if (has_b) out[(int64_t)lb * plane_stride + i] = planar_interp(Gb);
        }
    }
}

}  // namespace

// the layout limits of every grid kernel, for the other translation units (input_grad.hip)
int mfn_check_grid_desc(const mfnerf_grid_desc* d, const char* what) { return check_desc(d, what); }

extern "C" {

int mfnerf_grid_encode_fw(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                          const mfnerf_grid_desc* desc, const void* table_f16, void* out_f16,
                          mfnerf_stream_t stream) {
    int st = check_desc(desc, "grid_encode_fw");
    if (st) return st;
    if (n < 0) { mfn_set_error("grid_encode_fw: bad size"); return MFN_ERR_INVALID; }
    if (n == 0) return MFN_OK;
    if (!x || !table_f16 || !out_f16) { mfn_set_error("grid_encode_fw: null pointer"); return MFN_ERR_INVALID; }
    const int64_t want = div_up<int64_t>(n * (desc->n_levels / LEVELS_PER_LANE), ENC_BLOCK);
    const int64_t blocks = want < 8192 ? want : 8192;
    hipLaunchKernelGGL(grid_fw_kernel, dim3((unsigned)blocks), dim3(ENC_BLOCK), 0,
                       stream, x, n, n_dev, x_min, x_range, *desc, (const __half2*)table_f16, (__half*)out_f16);
    return mfn_check_launch("grid_encode_fw");
}

int mfnerf_grid_encode_fw_planar(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                 const mfnerf_grid_desc* desc, const void* table_f16, void* out_planes,
                                 int64_t plane_stride, mfnerf_stream_t stream) {
    int st = check_desc(desc, "grid_encode_fw_planar");
    if (st) return st;
    if (n < 0 || plane_stride < n) { mfn_set_error("grid_encode_fw_planar: bad size"); return MFN_ERR_INVALID; }
    // planar_gather loads 8 B at min(idx, size - 2): a one-entry level would wrap the clamp and read
    // past its table (grid_fw_kernel gathers entry by entry and takes such a level)
    for (int l = 0; l < desc->n_levels; ++l)
        if (desc->size[l] < 2u) {
            mfn_set_error("grid_encode_fw_planar: level %d has %u entries, the planar forward needs >= 2", l,
                          desc->size[l]);
            return MFN_ERR_INVALID;
        }
    if (n == 0) return MFN_OK;
    if (!x || !table_f16 || !out_planes) { mfn_set_error("grid_encode_fw_planar: null pointer"); return MFN_ERR_INVALID; }
    const int64_t want = div_up<int64_t>(n, ENC_BLOCK);
    const int64_t per_group = want < 2048 ? want : 2048;
    hipLaunchKernelGGL(grid_fw_planar_kernel, dim3((unsigned)(8 * per_group)), dim3(ENC_BLOCK), 0, stream, x, n, n_dev,
                       x_min, x_range, *desc, (const __half2*)table_f16, (__half2*)out_planes, plane_stride);
    return mfn_check_launch("grid_encode_fw_planar");
}

}  // extern "C"
