// grid_common.hpp -- what the hash-grid files (grid_fw.hip, grid_bw_atomic.hip, grid_bw_binned.hip with
// its grid_adam_fixed.hpp and grid_records.hpp) share: the block size, the DPP lane moves, the int32
// fixed-point scale of a table and its regions in the flat gradient, the fold of the packed private
// copies, and the host checks of a grid layout.
#pragma once
#include "common.hpp"
#include "grid_geo.hpp"

namespace mfn_grid {

constexpr int ENC_BLOCK = 256;
// private copies of the dense coarse levels' table gradient (grid_bw_atomic.hip), picked per wave: a
// power of two (8-64 copies measured the same; 1: grid_bw 0.300 -> 0.315 ms, 2: 0.306).  Round 6, the
// current dense kernel: 16 / 32 copies ran 0.538 / 0.638 vs 0.506 ms/step at Lego, 1.220 / 1.350 vs
// 1.184 at config 3's field (r6o: profiles/r06_v7_ab_dense_window.txt)
constexpr int GRAD_COPIES = 8;

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
#define DPP_ROW_SHL(d) (0x100 | (d))
#define DPP_ROW_SHR(d) (0x110 | (d))

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dppz_i(int v) {  // lanes without a source (or outside ROW_MASK) read 0
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}

// The int32 fixed-point scale of a table from l1, the L1 norm of the dL/dy adding into it (the
// gradient is summed as rint(v * scale), exact and order-free, and converted back by 1 / scale).
__device__ __forceinline__ float fixed_scale(float l1) {
    // |entry sum| <= sum over samples of |dL/dy| of the level = l1 < 2^e, so scale 2^(30-e) keeps
    // every entry (and every private copy of one) within 2^30: no int32 overflow is possible
    if (!(l1 > 0.0f)) return 0.0f;
    int e;
    frexpf(l1, &e);
    return ldexpf(1.0f, 30 - e);
}

// The scale of the table level l adds into.  A MixedFeature table shared by several levels takes
// the sum of their L1 bounds, so every level adding into it uses the table's one scale and the
// bound still holds for each entry.
__device__ __forceinline__ float table_fixed_scale(const mfnerf_grid_desc& D, const float* __restrict__ level_l1,
                                                   int l) {
    float l1 = 0.0f;
    for (int k = 0; k < D.n_levels; ++k)
        if (D.offset[k] == D.offset[l]) l1 += level_l1[k];
    return fixed_scale(l1);
}

__device__ __forceinline__ void load_fixed_scales(const mfnerf_grid_desc& D, const float* __restrict__ level_l1,
                                                  float* fs_s) {
    if ((int)threadIdx.x < D.n_levels) fs_s[threadIdx.x] = table_fixed_scale(D, level_l1, threadIdx.x);
}

// Fixed-point gradient regions (shared memory, built by the whole block): the tables in address
// order -- a level's own table, or a shared MixedFeature table counted once (the levels sharing it
// have its offset) -- each with its table's 1/scale; lo_v[r] = first value index of region r.
struct TableRegions {
    float lvl_inv[MFN_MAX_LEVELS], inv_s[MFN_MAX_LEVELS];
    int64_t lo_v[MFN_MAX_LEVELS + 1];
    int n_reg;
    __device__ void build(const mfnerf_grid_desc& D, const float* __restrict__ level_l1, int64_t total_vals) {
        if (threadIdx.x < D.n_levels) {
            const float sc = table_fixed_scale(D, level_l1, threadIdx.x);
            lvl_inv[threadIdx.x] = sc > 0.0f ? 1.0f / sc : 0.0f;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int nr = 0;
            int64_t last = -1;
            for (int k = 0; k < D.n_levels; ++k) {
                if ((int64_t)D.offset[k] <= last) continue;
                last = D.offset[k];
                inv_s[nr] = lvl_inv[k];
                lo_v[nr++] = 2 * (int64_t)D.offset[k];
            }
            lo_v[nr] = total_vals;
            n_reg = nr;
        }
        __syncthreads();
    }
};

// The private copies of the fixed-point path hold each entry's two features as ONE packed integer
// f1 * 2^32 + f0 (64-bit atomics carry both; grid_bw_dense_kernel, grid_bw_body): the sum of the
// copies is exact in int64, and f0 = int32(low word), f1 = int32(high word) + (f0 < 0) undoes the
// borrow of a negative f0.  Values i .. i+3 (entries i/2, i/2+1); the copies are zeroed.
__device__ __forceinline__ int4 fold_packed_copies(int* __restrict__ priv, int64_t dense_vals, int64_t i) {
    // every copy's load issued before the first zeroing store (a load-store pair per copy in turn
    // made the fold one memory round trip per copy: ~55 us of fixed cost in the optimizer pass)
    longlong2 c[GRAD_COPIES];
#pragma unroll
    for (int k = 0; k < GRAD_COPIES; ++k) c[k] = *reinterpret_cast<const longlong2*>(priv + k * dense_vals + i);
    long long a = 0, b = 0;
#pragma unroll
    for (int k = 0; k < GRAD_COPIES; ++k) {
        a += c[k].x;
        b += c[k].y;
        *reinterpret_cast<longlong2*>(priv + k * dense_vals + i) = make_longlong2(0, 0);
    }
    const int a0 = (int)(uint32_t)(unsigned long long)a, b0 = (int)(uint32_t)(unsigned long long)b;
    return make_int4(a0, (int)(a >> 32) + (a0 < 0), b0, (int)(b >> 32) + (b0 < 0));
}

// Host checks of a layout (static: internal to each file, as the library exports none of them).
static inline int64_t dense_entries_of(const mfnerf_grid_desc* d) {
    int64_t e = 0;  // dense own-table levels are laid out first (res grows with the level)
    for (int l = 0; l < d->n_levels; ++l) {
        const uint64_t r = d->res[l];
        if (d->table_kind[l] != 0 || r * r * r > d->size[l] || (int64_t)d->offset[l] != e) break;
        e += d->size[l];
    }
    return e;
}

// grid_bw's workgroup count cap (grid-stride beyond it; 4096 / 1024 / 512 / 256 / 128 measured
// 832 / 860 / 855 / 869 / 1166 us for the round-1 float scatter)
static inline int64_t grid_bw_block_cap() { return 4096; }

static inline int check_desc(const mfnerf_grid_desc* d, const char* what) {
    if (!d) { mfn_set_error("%s: null grid desc", what); return MFN_ERR_INVALID; }
    if (d->n_features != 2 || d->n_levels <= 0 || d->n_levels > MFN_MAX_LEVELS || d->n_levels % 4 != 0) {
        mfn_set_error("%s: unsupported grid (n_features=%d must be 2, n_levels=%d must be a multiple of 4 <= %d)",
                      what, d->n_features, d->n_levels, MFN_MAX_LEVELS);
        return MFN_ERR_INVALID;
    }
    for (int l = 0; l < d->n_levels; ++l)
        if (d->size[l] == 0 || d->res[l] == 0 || d->table_kind[l] < 0 || d->table_kind[l] > 1 ||
            // the canonical-grid map computes (coord + 1) * canon_res in 32 bits (canon_coord)
            (d->table_kind[l] == 1 && ((uint64_t)d->res[l] + 2) * (uint64_t)d->canon_res >= (1ull << 31))) {
            mfn_set_error("%s: bad level %d", what, l); return MFN_ERR_INVALID;
        }
    return MFN_OK;
}

// values (2 per entry) from the table's start to the end of its last level
static inline int64_t table_values_of(const mfnerf_grid_desc* d) {
    int64_t total = 0;
    for (int l = 0; l < d->n_levels; ++l) {
        const int64_t e = 2 * ((int64_t)d->offset[l] + d->size[l]);
        total = e > total ? e : total;
    }
    return total;
}

}  // namespace mfn_grid
