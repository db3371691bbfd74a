// wave_ops.hpp -- lane reads, scans and sums over one 64-lane wave, for the wave-per-ray kernels of
// vren_march.hip and vren_composite.hip.
#pragma once
#include "common.hpp"

namespace mfn {

__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int ffs64(uint64_t m) { return __ffsll((unsigned long long)m) - 1; }

// Wave scans and sums on the DPP network: row_shr 1/2/4/8 inside each 16-lane row, then
// row_bcast:15 / row_bcast:31 carry the row totals -- a few cycles per step, where each __shfl step
// is an LDS-routed ds_bpermute with ~100 cycles of latency (this path runs one wave per ray).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_src(float v) {
    // lanes outside ROW_MASK, or without a source lane, read 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float wave_incl_scan(float v) {
    v += dpp_src<0x111, 0xF>(v);  // row_shr:1
    v += dpp_src<0x112, 0xF>(v);  // row_shr:2
    v += dpp_src<0x114, 0xF>(v);  // row_shr:4
    v += dpp_src<0x118, 0xF>(v);  // row_shr:8
    v += dpp_src<0x142, 0xA>(v);  // row_bcast:15 -> rows 1 and 3
    v += dpp_src<0x143, 0xC>(v);  // row_bcast:31 -> rows 2 and 3
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return readlane_f(wave_incl_scan(v), 63); }

}  // namespace mfn
