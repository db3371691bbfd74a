// grid_records.hpp -- the partitioned ("binned") table-gradient scatter's plan and its 8-B records:
// what bin_scatter_kernel emits per (sample, level) and bin_accum_kernel decodes.  Part of
// grid_bw_binned.hip, its only includer: BinPlan is an argument of that file's kernels, so it shares
// their anonymous namespace.
#pragma once
#include "grid_common.hpp"

namespace {

using namespace mfn_grid;

struct BinPlan {
    int n_binned;                    // levels routed through the bins
    int n_bins;                      // partitions over all their tables
    int n_tables;
    int shift;                       // partition = 2^shift entries of one table
    int pair_ok;                     // no x-pair can straddle two partitions (one record per row)
    int level[MFN_MAX_LEVELS];       // binned level list
    int pairable[MFN_MAX_LEVELS];    // per level: x+1's entry = x's entry ^ (x ^ (x+1)) (own power-of-two hash)
    int merge[MFN_MAX_LEVELS];       // per level: never a pair record -> runs merged (merged_level_records)
    int table_of[MFN_MAX_LEVELS];    // per level: its table
    uint32_t t_offset[MFN_MAX_LEVELS], t_size[MFN_MAX_LEVELS];
    int t_bin0[MFN_MAX_LEVELS + 1];  // first bin of each table; t_bin0[n_tables] = n_bins
    int t_level[MFN_MAX_LEVELS];     // a level of each table (its fixed-point scale)
};

__device__ __forceinline__ int bin_table(const BinPlan& P, int b) {
    int t = 0;
    while (t + 1 < P.n_tables && b >= P.t_bin0[t + 1]) ++t;
    return t;
}

// The records of one (sample, binned level j): up to 4 (y,z) rows x (1 or 2 records).  EMIT(bin,
// rec) is called per record; rec = {w0, a | b << 16} (8 B): a/b = wy*wz*dL/dy_f * scale * 2^-15 as
// fp16 (scale: the table's int32 fixed-point scale, so |wy*wz*dL/dy_f * scale| < 2^30 and the fp16
// value < 2^15 never overflows; rounded once to 11 significant bits -- the precision of the fp16
// operands field_bw computed dL/dy from, and of tcnn's own half-precision gradient, whose SUM is
// rounded to fp16 at every add) and
//   w0 = e0 (bits 0-10, entry in the bin) | t << 11 (4 bits) | single << 15 | sel << 16 | fx << 17,
// fx = the x weight as 15-bit unorm (exact for the fine levels, whose positions carry <= 13
// fraction bits).  A pair record adds (1-fx)(a,b) to e0 and fx(a,b) to e1 = e0 ^ ((2^(t+1) - 1) << s),
// s = bit 16 (sel has no meaning in a pair record): an own power-of-two hash table has idx(x+1) =
// idx(x) ^ (x ^ (x+1)), t = trailing ones of x, s = 0, and the two share a bin unless the carry
// reaches bit `shift` (1 x in 2^shift).  A shared MixedFeature table hashes the canonical coordinates
// c(x): where c(x+1) = c(x) + 1 the same holds with t = trailing ones of c(x); where c(x+1) = c(x) + 2
// (the levels one or two steps below the canonical resolution), c ^ (c + 2) = (c' ^ (c' + 1)) << 1 for
// c' = c >> 1: t = trailing ones of c', s = 1 (round 5).  Otherwise (larger steps, straddles, other
// tables) each entry gets a single record with weight sel ? fx : 1-fx.
// a record's two values: fp16 of v * 2^-15, round to nearest even (v in the table's int32 units)
constexpr float REC_DOWN = 1.0f / 32768.0f, REC_UP = 32768.0f;
typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t rec_values(float a, float b) {
    const _Float16 ha = (_Float16)(a * REC_DOWN), hb = (_Float16)(b * REC_DOWN);  // (exact scaling)
    return (uint32_t)__builtin_bit_cast(uint16_t, ha) | ((uint32_t)__builtin_bit_cast(uint16_t, hb) << 16);
}
// value k of a record (0: a, 1: b) times 2^-15 (scale it by 2^15 x the unit to use)
__device__ __forceinline__ float rec_value(uint32_t ab, int k) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(ab >> (16 * k)));
}

template <typename EMIT>
__device__ __forceinline__ void level_records_geo(const mfnerf_grid_desc& D, const BinPlan& P, int j,
                                                  const LevelGeo& Lg, float g0, float g1, float fs, EMIT&& emit) {
    const int l = P.level[j];
    const int t = P.table_of[l];
    const int bin0 = P.t_bin0[t];
    const uint32_t fxq = min(32767u, (uint32_t)rintf(Lg.w[0] * 32768.0f)) << 17;
    uint32_t ones = (uint32_t)__builtin_ctz(~Lg.g[0]);  // trailing ones of x
    uint32_t pflags = 0u;                               // s << 16
    bool pair_hash = P.pairable[l] && ones < 15;
    if (D.table_kind[l] == 1 && (D.size[l] & (D.size[l] - 1)) == 0) {
        // a shared MixedFeature table: the x-pair's canonical step (corner_index's canon_coord)
        const uint32_t rc = (uint32_t)D.canon_res, res = D.res[l];
        const float inv = 1.0f / (float)res;
        const uint32_t c0 = canon_coord(Lg.g[0], rc, res, inv), c1 = canon_coord(Lg.g[0] + 1, rc, res, inv);
        const uint32_t cs = c1 - c0 == 2u ? c0 >> 1 : c0;
        ones = (uint32_t)__builtin_ctz(~cs);
        pflags = c1 - c0 == 2u ? 1u << 16 : 0u;
        pair_hash = (c1 - c0 == 1u || c1 - c0 == 2u) && ones < 15;
    }
    // the accumulate decodes e1 = e0 ^ (((2^(t+1) - 1) << s): valid only if that mask lies inside the
    // table (corner_index masks both indices by size - 1; with a table of at most one partition, the
    // same-partition test below would pass for a mask reaching past it -- ADVICE r5)
    pair_hash = pair_hash && ((((2u << ones) - 1u) << (pflags >> 16)) < D.size[l]);
    const float s0 = g0 * fs, s1 = g1 * fs;  // in the table's int32 fixed-point units
    const uint32_t mask = (1u << P.shift) - 1;
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        const uint32_t gy = Lg.g[1] + (yz & 1), gz = Lg.g[2] + (yz >> 1);
        const float wy = (yz & 1) ? Lg.w[1] : 1.0f - Lg.w[1];
        const float wz = (yz >> 1) ? Lg.w[2] : 1.0f - Lg.w[2];
        const float wyz = wy * wz;
        const uint32_t i0 = corner_index(D, l, Lg.g[0], gy, gz);
        const uint32_t i1 = corner_index(D, l, Lg.g[0] + 1, gy, gz);
        const int b0 = bin0 + (int)(i0 >> P.shift), b1 = bin0 + (int)(i1 >> P.shift);
        const uint32_t ab = rec_values(wyz * s0, wyz * s1);
        // static record slots 2 yz, 2 yz + 1, both always emitted (bin -1: no record), so the
        // caller's per-slot register arrays see constant indices on every path and stay registers
        const bool pair = pair_hash && b0 == b1;
        emit(2 * yz, b0, make_uint2((i0 & mask) | (pair ? (ones << 11) | pflags : (1u << 15)) | fxq, ab));
        emit(2 * yz + 1, pair ? -1 : b1, make_uint2((i1 & mask) | (1u << 15) | (1u << 16) | fxq, ab));
    }
}

// The PAIR layout's records (BinPlan::pair_ok: every binned level an own power-of-two hash table and
// every x + 1 below 2^shift, so the x-pair never straddles a partition): one record per (y,z) row,
// the hash written out (corner_index's prime hash masked to the table size, no layout branches), the
// partition from the index's high bits, and s0 / s1 already scaled by the table unit x 2^-15 (exact:
// a power of two), so rec_values' own scaling is gone.  The same records as level_records_geo but
// for the fp16 rounding of a value: the compiler folds wyz * s0 and its conversion into one v_fma_mix
// (the exact product rounded once to f16), where level_records_geo rounds the product to f32 first
// (its last, exact scaling folds instead) -- the two differ only where that f32 rounding crosses an
// f16 rounding boundary.  Still deterministic.  EMIT(row, partition in the table, record).
template <typename EMIT>
__device__ __forceinline__ void pair_level_records(const mfnerf_grid_desc& D, const BinPlan& P, int l, float x,
                                                   float y, float z, float s0, float s1, EMIT&& emit) {
    const LevelGeo Lg = level_geo(D.scale[l], x, y, z);
    const uint32_t mask = D.size[l] - 1u, emask = (1u << P.shift) - 1u;
    const uint32_t fxq = min(32767u, (uint32_t)rintf(Lg.w[0] * 32768.0f)) << 17;
    // trailing ones of x (< shift for every x + 1 < 2^shift, which pair_ok guarantees inside the grid;
    // the clamp keeps a point outside it from naming an x-pair beyond its partition), and fx
    const uint32_t ones = min((uint32_t)__builtin_ctz(~Lg.g[0]), (uint32_t)P.shift - 1u);
    const uint32_t flags = (ones << 11) | fxq;
    const uint32_t hy0 = Lg.g[1] * PRIME1, hz0 = Lg.g[2] * PRIME2;
    const float wy1 = Lg.w[1], wy0 = 1.0f - wy1, wz1 = Lg.w[2], wz0 = 1.0f - wz1;
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {
        const uint32_t hy = (yz & 1) ? hy0 + PRIME1 : hy0, hz = (yz >> 1) ? hz0 + PRIME2 : hz0;
        const uint32_t i0 = (Lg.g[0] ^ hy ^ hz) & mask;
        const float wyz = ((yz & 1) ? wy1 : wy0) * ((yz >> 1) ? wz1 : wz0);
        // both values rounded to f32, then packed to f16 pairs by one v_cvt_pk_f16_f32 (the
        // rounding of level_records_geo; one conversion instead of two fma_mix + the packing)
        const float2v v = {wyz * s0, wyz * s1};
        const uint32_t ab = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, half2v));
        emit(yz, (int)(i0 >> P.shift), make_uint2((i0 & emask) | flags, ab));
    }
}

// Runs of one cell inside a 16-lane DPP row (a 16-sample chunk: consecutive samples of a ray, the
// scatter's lane order).  A dead lane (no gradient or no sample) is a run of its own.  suffix_sums
// leaves each run's sums in its first lane: a segmented suffix sum over the row, 4 DPP steps, one
// fixed order (every lane of the wave must call it).  keep[k]: 1 if the lane adds the values 2^k
// lanes on at step k (its run goes on past them) -- the same for every value, so computed once.
struct RunRow {
    bool same_prev, same_next;
    float keep[4];
    __device__ __forceinline__ void suffix_sums(float* v) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = fmaf(dpp_f<DPP_ROW_SHL(1)>(v[k]), keep[0], v[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaf(dpp_f<DPP_ROW_SHL(2)>(v[k]), keep[1], v[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaf(dpp_f<DPP_ROW_SHL(4)>(v[k]), keep[2], v[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaf(dpp_f<DPP_ROW_SHL(8)>(v[k]), keep[3], v[k]);
    }
};
__device__ __forceinline__ RunRow run_row(const LevelGeo& Lg, bool live) {
    // every DPP read is unconditional and combined with non-short-circuit operators: a DPP inside a
    // `&&` or `?:` runs under a narrowed EXEC, and a lane reading a disabled neighbour reads 0
    RunRow r;
    const int lr = (int)(threadIdx.x & 15);
    const int k0 = live ? (int)Lg.g[0] : -1, k1 = live ? (int)Lg.g[1] : -1, k2 = live ? (int)Lg.g[2] : -1;
    const int n0 = dpp_i<DPP_ROW_SHL(1)>(k0), n1 = dpp_i<DPP_ROW_SHL(1)>(k1), n2 = dpp_i<DPP_ROW_SHL(1)>(k2);
    const int p0 = dpp_i<DPP_ROW_SHR(1)>(k0), p1 = dpp_i<DPP_ROW_SHR(1)>(k1), p2 = dpp_i<DPP_ROW_SHR(1)>(k2);
    r.same_next = (lr < 15) & (n0 == k0) & (n1 == k1) & (n2 == k2);
    r.same_prev = (lr > 0) & (p0 == k0) & (p1 == k1) & (p2 == k2);
    int stop = r.same_next ? 0 : 1;  // this lane's run ends within the lanes summed so far
    int t;
    r.keep[0] = stop ? 0.0f : 1.0f;
    t = dpp_i<DPP_ROW_SHL(1)>(stop);
    stop |= t;
    r.keep[1] = stop ? 0.0f : 1.0f;
    t = dpp_i<DPP_ROW_SHL(2)>(stop);
    stop |= t;
    r.keep[2] = stop ? 0.0f : 1.0f;
    t = dpp_i<DPP_ROW_SHL(4)>(stop);
    stop |= t;
    r.keep[3] = stop ? 0.0f : 1.0f;
    return r;
}

template <typename EMIT>
__device__ __forceinline__ void level_records(const mfnerf_grid_desc& D, const BinPlan& P, int j, float x, float y,
                                              float z, float g0, float g1, float fs, EMIT&& emit) {
    level_records_geo(D, P, j, level_geo(D.scale[P.level[j]], x, y, z), g0, g1, fs, emit);
}

// The thread layout merged_level_records (run_row's DPP reads) depends on, in bin_scatter_kernel, its
// only caller.  The compiler checks the shape; that all 64 lanes are ACTIVE at the call is the
// caller's duty (count() must stay wave-uniform), and nothing checks it at run time.
constexpr int SC_THREADS = 1024;  // the scatter workgroup
static_assert(SC_THREADS % 64 == 0, "whole waves: a DPP read of a lane that does not exist returns 0");
static_assert(SC_THREADS % 16 == 0,
              "stage_tile puts sample k of a tile on thread k % SC_THREADS and in slot k & 15 of its 16-sample chunk: "
              "k & 15 == threadIdx.x & 15, so one chunk (consecutive samples of a ray) fills one 16-lane DPP row");

// Round 6: the records of a level that never forms a pair record (BinPlan::merge: a MixedFeature
// shared table whose canonical x-step is >= 3, an own table without the power-of-two hash), with the
// samples of one run merged.  A 16-lane DPP row holds a 16-sample chunk -- consecutive samples of a
// ray -- and at the coarse shared levels ~2-3 consecutive samples fall in one cell: same 8 corner
// entries, other weights.  Per (y,z) row each lane computes its 4 weighted values ({x, x+1} x 2
// features, the x weight applied: (1 - fx) wyz g and fx wyz g in table units), a segmented suffix
// sum over the row (RunRow, 4 DPP steps, a fixed order) leaves each run's sums in its first lane,
// and only that lane emits the run's 8 single records, weight 1 (fx = 0, sel = 0).  Every lane of
// the wave must call it (DPP reads its row neighbours); `live` false: no gradient / no sample.
// Measured (r6c, config 3's field): mf128 step 1.244 -> 1.204 ms, grid_bw 0.674 -> 0.637 ms.  The
// same merge for the Lego layout's coarse PAIR levels (runs of >= 2 as two single-record halves
// from the run's first two lanes) ran 0.5125 vs 0.4953 ms/step: with two samples per lane it
// spilled (62 VGPRs) and its records saved less -- a run of two is two records either way.
// The same entries and contributions as level_records_geo's singles; each value is now the run's
// fp32 sum rounded once to fp16 (the 2^-11 record bound holds for the sum), and the x weight exact
// instead of a 15-bit fx.
template <typename EMIT>
__device__ __forceinline__ void merged_level_records(const mfnerf_grid_desc& D, const BinPlan& P, int j, float x,
                                                     float y, float z, float g0, float g1, float fs, bool live,
                                                     EMIT&& emit) {
    const int l = P.level[j];
    const LevelGeo Lg = level_geo(D.scale[l], live ? x : 0.0f, live ? y : 0.0f, live ? z : 0.0f);
    const RunRow rr = run_row(Lg, live);
    const float s0 = live ? g0 * fs : 0.0f, s1 = live ? g1 * fs : 0.0f;  // table int32 units
    const float wx1 = Lg.w[0], wx0 = 1.0f - wx1, wy1 = Lg.w[1], wy0 = 1.0f - wy1, wz1 = Lg.w[2], wz0 = 1.0f - wz1;
    const bool head = live && !rr.same_prev;  // a run's first lane emits the run's records
    const int bin0 = P.t_bin0[P.table_of[l]];
    const uint32_t emask = (1u << P.shift) - 1u;
#pragma unroll
    for (int yz = 0; yz < 4; ++yz) {  // row by row: 4 values in flight
        const float wyz = ((yz & 1) ? wy1 : wy0) * ((yz >> 1) ? wz1 : wz0);
        const float a = wyz * s0, b = wyz * s1;
        float v[4] = {wx0 * a, wx0 * b, wx1 * a, wx1 * b};
        rr.suffix_sums(v);
        if (head) {
            const uint32_t gy = Lg.g[1] + (yz & 1), gz = Lg.g[2] + (yz >> 1);
            const uint32_t i0 = corner_index(D, l, Lg.g[0], gy, gz);
            const uint32_t i1 = corner_index(D, l, Lg.g[0] + 1, gy, gz);
            emit(2 * yz, bin0 + (int)(i0 >> P.shift), make_uint2((i0 & emask) | (1u << 15), rec_values(v[0], v[1])));
            emit(2 * yz + 1, bin0 + (int)(i1 >> P.shift), make_uint2((i1 & emask) | (1u << 15), rec_values(v[2], v[3])));
        }
    }
}

// A sample staged in registers for all its binned levels: normalised position and dL/dy of the
// binned levels (contiguous), loaded once before the level loop -- a load inside the loop would
// wait behind the previous level's record stores (one in-order vmcnt), serialising the levels.
constexpr int MAX_BINNED = 16;
template <int MAXB>
struct StagedSample {
    float x, y, z;
    float g[2 * MAXB];
};

template <int MAXB>
__device__ __forceinline__ void stage_sample(const mfnerf_grid_desc& D, const BinPlan& P, const float* __restrict__ X,
                                             float x_min, float x_range, const float* __restrict__ dy, int64_t i,
                                             StagedSample<MAXB>& S) {
    S.x = (X[3 * i] - x_min) / x_range;
    S.y = (X[3 * i + 1] - x_min) / x_range;
    S.z = (X[3 * i + 2] - x_min) / x_range;
    const float2* src = reinterpret_cast<const float2*>(dy + i * (2 * D.n_levels) + 2 * P.level[0]);
#pragma unroll
    for (int j = 0; j < MAXB; ++j) {
        const float2 v = j < P.n_binned ? src[j] : make_float2(0.f, 0.f);
        S.g[2 * j] = v.x;
        S.g[2 * j + 1] = v.y;
    }
}

// one sample's dL/dy pair at binned level j, selected once for both record passes (count, place)
struct SampleLevel {
    float g0, g1;
    bool live;
};

template <int MAXB>
__device__ __forceinline__ SampleLevel sample_level(const mfnerf_grid_desc& D, const BinPlan& P,
                                                    const StagedSample<MAXB>& S, int j) {
    float g0 = 0.f, g1 = 0.f;
#pragma unroll
    for (int k = 0; k < MAXB; ++k)  // register-indexed select (j is uniform: scalar compares)
        if (k == j) { g0 = S.g[2 * k]; g1 = S.g[2 * k + 1]; }
    SampleLevel r;
    r.g0 = g0;
    r.g1 = g1;
    r.live = !(r.g0 == 0.0f && r.g1 == 0.0f);  // terminated samples: nothing to add
    return r;
}

}  // namespace
