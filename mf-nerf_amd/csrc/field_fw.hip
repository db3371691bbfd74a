// field_fw.hip -- NGP field head on gfx950 MFMA: the two tiny-cuda-nn FullyFusedMLPs of
// models/networks.py:36-79 (xyz: 32->64->16; rgb: [SH4(16) | h(16)] -> W -> W -> 3 with
// W = rgb_channels in {64, 128} (opt.py:87; the MF benchmark scripts use 128), ReLU, bias-free,
// fp16 operands / fp32 accumulation), TruncExp on h[0] and the SH4 direction encoding.  This unit:
// the weight repack, the forward and the SH4 encoding as a module of its own; the backward is
// field_bw.hip.
//
// Layout (one wave = one tile of 32 samples, v_mfma_f32_32x32x16_f16):
//   activations are kept TRANSPOSED -- channel on the MFMA row, sample on the lane (col = lane&31)
//   -- so layer k's fp32 accumulator, ReLU'd and packed to f16, IS layer k+1's B operand with no
//   LDS round trip (cdna_hip_programming.md section 3, "An accumulator tile as the next MFMA's
//   operand").  The weights are the A operands, pre-permuted once per optimizer step by
//   mfnerf_field_pack_weights into 1-KiB lane-linear fragments (ds_read_b128, conflict-free).
//   Backward: see the comment above field_bw_coop_kernel (field_bw.hip).
#include "common.hpp"
#include "mfma_pack.hpp"
#include "field_pack.hpp"
#include "field_fwd.hpp"
#include "field_width.hpp"
#include "../../include/mfnerf.h"

using namespace mfn;
using namespace mfn_field;

namespace {

// tcnn SphericalHarmonics degree 4 as a module of its own (the tinycudann route's dir_encoder,
// networks.py:60-67): in = (d/|d| + 1)/2 (n, 3) f32 -> (n, 16) f16, the IEEE operations and their
// order of mfnerf/tcnn.py sh4_torch (no contraction), rounded to f16 once.  The fused field head
// evaluates the same polynomial in-kernel (sh4 of field_fwd.hpp: both call sh4_poly).
__global__ __launch_bounds__(256) void sh4_fw_kernel(const float* __restrict__ in, int64_t n,
                                                     __half* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float o[16];
    sh4_poly(in[3 * i] * 2.0f - 1.0f, in[3 * i + 1] * 2.0f - 1.0f, in[3 * i + 2] * 2.0f - 1.0f, o);
    // each value rounded to f32 first, as torch does: an opaque use keeps the compiler from folding a
    // product and its f16 conversion into one v_fma_mix (a single rounding of the exact product,
    // which differs from torch's double rounding on ~1 value in 10^6)
#pragma unroll
    for (int k = 0; k < 16; ++k) asm volatile("" : "+v"(o[k]));
    __half2* dst = reinterpret_cast<__half2*>(out + 16 * i);
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = __floats2half2_rn(o[2 * k], o[2 * k + 1]);
}

template <typename TP, int W>
__global__ void pack_kernel(const TP* __restrict__ px, const TP* __restrict__ pr, _Float16* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < Geo<W>::N * FRAG_HALFS) pack_elem<TP, W>(t, px, pr, out);
}

// feat layouts (load_feat, field_fwd.hpp): plane_stride == 0 -> row-major; > 0 -> level-major planes.
__device__ __forceinline__ void load_tile_in(const _Float16* __restrict__ feat, int64_t plane_stride,
                                             const float* __restrict__ dirs, int64_t s, bool valid, int h,
                                             bool want_dirs, TileIn& I) {
    if (valid) {
        // load_feat's two bodies, by hand: called through it under this runtime choice, the four
        // non-density field_fw_kernel instantiations compile to other code
        if (plane_stride > 0) {
            const uint32_t* P = reinterpret_cast<const uint32_t*>(feat);
            uint32_t u[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u[k] = P[(int64_t)(4 * h + k) * plane_stride + s];
                u[4 + k] = P[(int64_t)(8 + 4 * h + k) * plane_stride + s];
            }
            I.x[0] = *reinterpret_cast<const half8*>(&u[0]);
            I.x[1] = *reinterpret_cast<const half8*>(&u[4]);
        } else {
            const half8* row = reinterpret_cast<const half8*>(feat + s * 32);
            I.x[0] = row[h];
            I.x[1] = row[2 + h];
        }
        if (want_dirs) { I.d[0] = dirs[3 * s]; I.d[1] = dirs[3 * s + 1]; I.d[2] = dirs[3 * s + 2]; }
    } else {
        I.x[0] = half8{}; I.x[1] = half8{};
        I.d[0] = I.d[1] = I.d[2] = 0.0f;
    }
}

// LOGRAD (mfnerf_field_fw_lograd): the rgb head without its sigmoid; `rgb` then points to an (n,3) f16
// buffer, the log-radiance as tcnn returns it (the tonemap kernels' input)
template <int W, bool DENSITY_ONLY, bool LOGRAD = false>
__global__ __launch_bounds__(FIELD_BLOCK) void field_fw_kernel(const _Float16* __restrict__ feat,
                                                                int64_t plane_stride,
                                                                const float* __restrict__ dirs, int64_t n,
                                                                const int32_t* __restrict__ n_dev,
                                                                const _Float16* __restrict__ packed,
                                                                float* __restrict__ sigma, float* __restrict__ rgb,
                                                                const int32_t* __restrict__ cell,
                                                                float* __restrict__ cell_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* lds = reinterpret_cast<_Float16*>(smem);
    load_frags(lds, packed, DENSITY_ONLY ? 8 : Geo<W>::N_FW);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int64_t tiles = div_up<int64_t>(nn, 32);
    // P tiles per trip (tile, tile + stride, ...), stage by stage (forward_tiles).  P = 2 measured no
    // faster at W = 64 (28.7 vs 28 us: 204 registers, one wave per SIMD instead of two) and spills
    // at W = 128
    constexpr int P = 1;
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wid; tile < tiles; tile += P * stride) {
        TileIn I[P];
        bool valid[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const int64_t s = (tile + q * stride) * 32 + r;
            valid[q] = s < nn;
            load_tile_in(feat, plane_stride, dirs, s, valid[q], h, !DENSITY_ONLY, I[q]);
        }
        FwdTile<W> T[P];
        forward_tiles<W, DENSITY_ONLY, P, true, LOGRAD>(lds, lane, I, valid, T);
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const int64_t s = (tile + q * stride) * 32 + r;
            if (valid[q] && h == 0) {
                const float sg = __expf(T[q].h0);  // TruncExp forward (custom_functions.py:166)
                sigma[s] = sg;
                if (DENSITY_ONLY && cell_out) {  // the occupancy refresh's density_grid_tmp[cell] = sigma
                    const int32_t k = cell[s];
                    if (k >= 0) cell_out[k] = sg;
                }
                if constexpr (LOGRAD) {
                    _Float16* lograd = reinterpret_cast<_Float16*>(rgb);
                    lograd[3 * s] = (_Float16)T[q].rgb[0];
                    lograd[3 * s + 1] = (_Float16)T[q].rgb[1];
                    lograd[3 * s + 2] = (_Float16)T[q].rgb[2];
                } else if (!DENSITY_ONLY) {
                    // tcnn returns fp16 rgb; the reference casts it to fp32 for compositing
                    rgb[3 * s] = (float)(_Float16)T[q].rgb[0];
                    rgb[3 * s + 1] = (float)(_Float16)T[q].rgb[1];
                    rgb[3 * s + 2] = (float)(_Float16)T[q].rgb[2];
                }
            }
        }
    }
}

template <typename TP, int W>
void launch_pack(const TP* px, const TP* pr, void* packed, mfnerf_stream_t stream) {
    const int total = Geo<W>::N * FRAG_HALFS;
    hipLaunchKernelGGL((pack_kernel<TP, W>), dim3((total + 255) / 256), dim3(256), 0, stream, px, pr,
                       (_Float16*)packed);
}

template <int W, bool LOGRAD>
void launch_fw(const void* feat, int64_t ps, const float* dirs, int64_t n, const int32_t* n_dev, const void* packed,
               int density_only, float* sigma, float* rgb, mfnerf_stream_t stream, const int32_t* cell,
               float* cell_out) {
    const int64_t tiles = div_up<int64_t>(n, 32);
    const int64_t want = div_up<int64_t>(tiles, 4);
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    if (density_only)
        hipLaunchKernelGGL((field_fw_kernel<W, true>), dim3(blocks), dim3(FIELD_BLOCK), 8 * FRAG_HALFS * 2, stream,
                           (const _Float16*)feat, ps, dirs, n, n_dev, (const _Float16*)packed, sigma, rgb, cell,
                           cell_out);
    else
        hipLaunchKernelGGL((field_fw_kernel<W, false, LOGRAD>), dim3(blocks), dim3(FIELD_BLOCK),
                           (size_t)Geo<W>::N_FW * FRAG_HALFS * 2, stream, (const _Float16*)feat, ps, dirs, n, n_dev,
                           (const _Float16*)packed, sigma, rgb, nullptr, nullptr);
}

// mfnerf_field_fw, mfnerf_field_fw_lograd (LOGRAD) and mfnerf_field_fw_density_scatter (scatter:
// density only, cell and cell_out required): the same checks and launch, reported under `what`
template <bool LOGRAD>
int field_fw_impl(const char* what, const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                  const int32_t* n_dev, const void* packed, int rgb_width, int density_only, float* sigma, float* rgb,
                  bool scatter, const int32_t* cell, float* cell_out, mfnerf_stream_t stream) {
    if (!width_ok(rgb_width)) return bad_width(rgb_width);
    if (n < 0 || (feat_plane_stride != 0 && feat_plane_stride < n)) {
        mfn_set_error("%s: bad size", what); return MFN_ERR_INVALID;
    }
    if (n == 0) return MFN_OK;
    if (!feat_f16 || !packed || !sigma || (!density_only && (!dirs || !rgb)) || (scatter && (!cell || !cell_out))) {
        mfn_set_error("%s: null pointer", what); return MFN_ERR_INVALID;
    }
    width_dispatch(rgb_width, [&](auto w) {
        launch_fw<decltype(w)::value, LOGRAD>(feat_f16, feat_plane_stride, dirs, n, n_dev, packed, density_only, sigma,
                                              rgb, stream, cell, cell_out);
    });
    return mfn_check_launch(what);
}

}  // namespace

extern "C" {

int64_t mfnerf_field_packed_bytes(int rgb_width) {
    if (!width_ok(rgb_width)) return -1;
    return width_dispatch(rgb_width, [](auto w) { return (int64_t)Geo<decltype(w)::value>::N * FRAG_HALFS * 2; });
}

int mfnerf_field_pack_weights(const float* params_xyz, const float* params_rgb, int rgb_width, void* packed,
                              mfnerf_stream_t stream) {
    if (!width_ok(rgb_width)) return bad_width(rgb_width);
    if (!params_xyz || !params_rgb || !packed) { mfn_set_error("field_pack_weights: null pointer"); return MFN_ERR_INVALID; }
    width_dispatch(rgb_width, [&](auto w) { launch_pack<float, decltype(w)::value>(params_xyz, params_rgb, packed, stream); });
    return mfn_check_launch("field_pack_weights");
}

int mfnerf_sh4_fw(const float* dirs01, int64_t n, void* out_f16, mfnerf_stream_t stream) {
    if (n < 0 || (n > 0 && (!dirs01 || !out_f16))) { mfn_set_error("sh4_fw: bad arguments"); return MFN_ERR_INVALID; }
    if (n == 0) return MFN_OK;
    hipLaunchKernelGGL(sh4_fw_kernel, dim3((unsigned)div_up<int64_t>(n, 256)), dim3(256), 0, stream, dirs01, n,
                       (__half*)out_f16);
    return mfn_check_launch("sh4_fw");
}

int mfnerf_field_pack_weights_f16(const void* params_xyz_f16, const void* params_rgb_f16, int rgb_width, void* packed,
                                  mfnerf_stream_t stream) {
    if (!width_ok(rgb_width)) return bad_width(rgb_width);
    if (!params_xyz_f16 || !params_rgb_f16 || !packed) { mfn_set_error("field_pack_weights_f16: null pointer"); return MFN_ERR_INVALID; }
    const _Float16* px = (const _Float16*)params_xyz_f16;
    const _Float16* pr = (const _Float16*)params_rgb_f16;
    width_dispatch(rgb_width, [&](auto w) { launch_pack<_Float16, decltype(w)::value>(px, pr, packed, stream); });
    return mfn_check_launch("field_pack_weights_f16");
}

int mfnerf_field_fw(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                    const int32_t* n_dev, const void* packed,
                    int rgb_width, int density_only, float* sigma, float* rgb, mfnerf_stream_t stream) {
    return field_fw_impl<false>("field_fw", feat_f16, feat_plane_stride, dirs, n, n_dev, packed, rgb_width,
                                density_only, sigma, rgb, false, nullptr, nullptr, stream);
}

int mfnerf_field_fw_lograd(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                           const int32_t* n_dev, const void* packed, int rgb_width, float* sigma, void* lograd_f16,
                           mfnerf_stream_t stream) {
    return field_fw_impl<true>("field_fw_lograd", feat_f16, feat_plane_stride, dirs, n, n_dev, packed, rgb_width, 0,
                               sigma, reinterpret_cast<float*>(lograd_f16), false, nullptr, nullptr, stream);
}

int mfnerf_field_fw_density_scatter(const void* feat_f16, int64_t feat_plane_stride, int64_t n, const int32_t* n_dev,
                                    const void* packed, int rgb_width, float* sigma, const int32_t* cell_idx,
                                    float* tmp, mfnerf_stream_t stream) {
    return field_fw_impl<false>("field_fw_density_scatter", feat_f16, feat_plane_stride, nullptr, n, n_dev, packed,
                                rgb_width, 1, sigma, nullptr, true, cell_idx, tmp, stream);
}

}  // extern "C"
