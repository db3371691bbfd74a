// grid_adam_fixed.hpp -- the table gradient's int32 fixed-point sums back into floats: the convert
// pass alone (fold_convert_kernel), or convert + Adam in one pass (adam_fixed_kernel, and
// adam_fixed_body for bin_accum_kernel's leading workgroups).  Part of grid_bw_binned.hip, its only
// includer, and ahead of that file's kernels on purpose: the compiler inlines fold_packed_copies
// and adam_fixed_body in the order the translation unit first names them, fold_convert_kernel names
// fold_packed_copies first, and adam_fixed_kernel and bin_accum_kernel compile to other (equivalent)
// code where adam_fixed_body comes first -- so the three kernels share one translation unit.
#pragma once
#include "field_pack.hpp"
#include "grid_common.hpp"

namespace {

using namespace mfn_grid;

// ShardFlag (the data-parallel step): the step's non-finite flag into the first value of every
// exchange shard (NaN; mfnerf_flag_to_shards's job, without its launch) -- values this pass writes
// get it as they are written, the others (written by earlier launches) from workgroup 0.
struct ShardFlag {
    const int32_t* flag;  // NULL: none
    int64_t world, shard_len, table_off;  // grad[i] is flat value table_off + i
};

// Fixed-point path: grad[p] (float) = sum_k priv[k][p] / scale for the dense prefix (copies zeroed),
// grad[p] = int(grad[p]) / scale for the rest; scale per level from the same level_l1 as grid_bw.
__global__ __launch_bounds__(256) void fold_convert_kernel(float* __restrict__ grad, int* __restrict__ priv,
                                                           int64_t dense_vals, int64_t total_vals,
                                                           const mfnerf_grid_desc D,
                                                           const float* __restrict__ level_l1,
                                                           const ShardFlag SF = ShardFlag{}) {
    // table regions in address order -- a level's own table, or a shared MixedFeature table counted
    // once (the levels sharing it have its offset) -- each with its table's scale
    __shared__ TableRegions R;
    R.build(D, level_l1, total_vals);
    const float* inv_s = R.inv_s;
    const int64_t* lo_v = R.lo_v;
    const int n_reg = R.n_reg;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const bool raise = SF.flag && *SF.flag;
    if (raise && blockIdx.x == 0 && (int64_t)threadIdx.x < SF.world) {
        const int64_t f = (int64_t)threadIdx.x * SF.shard_len - SF.table_off;  // relative to grad
        if (f < 0 || f >= total_vals) grad[f] = __int_as_float(0x7fc00000);
    }
    int l = 0;  // region of value i (i increases per thread: walk forward)
    for (int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; 4 * i4 < total_vals; i4 += stride) {
        const int64_t i = 4 * i4;  // region boundaries are multiples of 16 values
        while (l + 1 < n_reg && i >= lo_v[l + 1]) ++l;
        const float is = inv_s[l];
        int4 acc;
        if (i < dense_vals) {
            acc = fold_packed_copies(priv, dense_vals, i);
            // the dense prefix's own entries in grad received no contributions (all went to copies)
        } else {
            acc = *reinterpret_cast<const int4*>(grad + i);
        }
        float4 o = make_float4((float)acc.x * is, (float)acc.y * is, (float)acc.z * is, (float)acc.w * is);
        if (raise) {
            float* oc = &o.x;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if ((SF.table_off + i + c) % SF.shard_len == 0 && (SF.table_off + i + c) / SF.shard_len < SF.world)
                    oc[c] = __int_as_float(0x7fc00000);
        }
        *reinterpret_cast<float4*>(grad + i) = o;
    }
}

// fold_convert + Adam in one pass (the unsharded, collective-free step): g[0, off) are float
// gradients (the MLPs), g[off, off + total_vals) the table's int32 fixed-point sums (the dense
// prefix's in GRAD_COPIES private copies); each value is converted exactly as fold_convert_kernel
// does, fed to the same Adam update as adam_kernel, and its gradient word (and copies) zeroed for
// the next step -- one pass over the gradient instead of a convert pass + a read in Adam.
// The float4 groups [i4_first, i4_end) step `stride` (a grid-stride loop over the caller's threads).
__device__ __forceinline__ void adam_fixed_body(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, __half* __restrict__ p16, int64_t off,
                                                int* __restrict__ priv, int64_t dense_vals, int64_t total_vals,
                                                const TableRegions& R, float lr, float b1, float b2, float eps,
                                                float bc1, float bc2, bool skipped, int64_t i4_first,
                                                int64_t i4_end, int64_t stride) {
    int l = 0;
    for (int64_t i4 = i4_first; i4 < i4_end; i4 += stride) {
        const int64_t i = 4 * i4, j = i - off;  // off, dense_vals, region bounds: multiples of 4
        float4 gg;
        if (j < 0 || j >= total_vals) {
            gg = reinterpret_cast<const float4*>(g)[i4];
        } else {
            while (l + 1 < R.n_reg && j >= R.lo_v[l + 1]) ++l;
            const float is = R.inv_s[l];
            int4 acc;
            if (j < dense_vals) {
                acc = fold_packed_copies(priv, dense_vals, j);
            } else {
                acc = reinterpret_cast<const int4*>(g)[i4];
            }
            gg = make_float4((float)acc.x * is, (float)acc.y * is, (float)acc.z * is, (float)acc.w * is);
        }
        reinterpret_cast<float4*>(g)[i4] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (skipped) continue;
        float4 pp = mfn::nt_load4(p + 4 * i4);
        float4 mm = mfn::nt_load4(m + 4 * i4);
        float4 vv = mfn::nt_load4(v + 4 * i4);
        mfn::adam_elem(pp.x, mm.x, vv.x, gg.x, b1, b2, eps, lr, bc1, bc2);
        mfn::adam_elem(pp.y, mm.y, vv.y, gg.y, b1, b2, eps, lr, bc1, bc2);
        mfn::adam_elem(pp.z, mm.z, vv.z, gg.z, b1, b2, eps, lr, bc1, bc2);
        mfn::adam_elem(pp.w, mm.w, vv.w, gg.w, b1, b2, eps, lr, bc1, bc2);
        mfn::nt_store4(p + 4 * i4, pp);
        mfn::nt_store4(m + 4 * i4, mm);
        mfn::nt_store4(v + 4 * i4, vv);
        if (p16) {
            __half2 a = __floats2half2_rn(pp.x, pp.y), b = __floats2half2_rn(pp.z, pp.w);
            uint2 u; u.x = *reinterpret_cast<uint32_t*>(&a); u.y = *reinterpret_cast<uint32_t*>(&b);
            reinterpret_cast<uint2*>(p16)[i4] = u;
        }
    }
}

// the MLP weights' repack riding the optimizer's last pass (out = nullptr: none)
struct PackArgs {
    const _Float16* px;  // xyz MLP (fp16 compute copy)
    const _Float16* pr;  // rgb MLP
    _Float16* out;       // the field head's fragment blob (mfnerf_field_pack_weights_f16's layout)
    int width;           // rgb width, 64 or 128
};

// tail_mode 0: values [0, n), or [0, fused_from) when the fused partitioned accumulate updated the
// rest (fused_ovf given; overflowed records included -- the accumulate adds them).  tail_mode 1
// (mfnerf_grid_encode_bw_binned_adam_all, whose accumulate launch updated every value): nothing but
// the MLP repack and the step's bookkeeping.
__global__ __launch_bounds__(256) void adam_fixed_kernel(float* __restrict__ p, float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         __half* __restrict__ p16, int64_t n, int64_t off,
                                                         int* __restrict__ priv, int64_t dense_vals,
                                                         int64_t total_vals, const mfnerf_grid_desc D,
                                                         float* __restrict__ level_l1, float lr, float b1,
                                                         float b2, float eps, int32_t* __restrict__ step_dev,
                                                         const float* __restrict__ lr_dev,
                                                         mfnerf_amp_state* __restrict__ amp, int n_levels,
                                                         int64_t fused_from, const int32_t* __restrict__ fused_ovf,
                                                         int tail_mode, const PackArgs pk) {
    __shared__ TableRegions R;
    int64_t lo = 0;
    if (tail_mode == 1) n = 0;                 // the accumulate launch updated every value
    else if (fused_ovf) n = fused_from;        // values >= fused_from: updated by the accumulate
    if (n > lo) {  // (uniform)
        R.build(D, level_l1, total_vals);
        const bool skipped = amp && amp->nonfinite;  // GradScaler: no update on a non-finite gradient, only the zeroing
        const int st = *step_dev + 1;
        if (lr_dev) lr = *lr_dev;
        const float bc1 = 1.0f - powf(b1, (float)st);
        const float bc2 = 1.0f - powf(b2, (float)st);
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        adam_fixed_body(p, g, m, v, p16, off, priv, dense_vals, total_vals, R, lr, b1, b2, eps, bc1, bc2, skipped,
                        lo / 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n / 4, stride);
    }
    // tail_mode 1: the MLP weights' repack (their p16 was written by the accumulate launch)
    if (pk.out) {
        const int total = (pk.width == 64 ? mfn_field::Geo<64>::N : mfn_field::Geo<128>::N) * mfn_field::FRAG_HALFS;
        for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
            if (pk.width == 64) mfn_field::pack_elem<_Float16, 64>(t, pk.px, pk.pr, pk.out);
            else mfn_field::pack_elem<_Float16, 128>(t, pk.px, pk.pr, pk.out);
        }
    }
    // step count / skip count / loss scale, and level_l1 zeroed for the next step's field_bw, by the
    // last workgroup (every workgroup has read level_l1, step_dev and the flag by now)
    if (amp) mfn::amp_step_end_last_block(step_dev, amp, level_l1, n_levels);
}

}  // namespace
