// field_fwd.hpp -- the wave-level forward of the NGP field head (one wave = one tile of 32 samples,
// v_mfma_f32_32x32x16_f16; layout: field_fw.hip, fragment order: field_pack.hpp), shared by
// field_fw.hip, field_bw.hip (its recomputation) and render.hip.
#pragma once
#include "common.hpp"
#include "mfma_pack.hpp"
#include "field_pack.hpp"

namespace mfn_field {

using mfn::lds_frag;
using mfn::load_frags;
using mfn::mfma;
using mfn::pack8;

constexpr int FIELD_BLOCK = 256;    // forward: 4 waves

// The degree-4 spherical-harmonics polynomial of tcnn on the unit direction (x, y, z): the IEEE
// operations and their order of mfnerf/tcnn.py sh4_torch.  (Its Jacobian: sh4_bw_dir, field_bw.hip.)
__device__ __forceinline__ void sh4_poly(float x, float y, float z, float* o) {
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    o[0] = 0.28209479177387814f;
    o[1] = -0.48860251190291987f * y;
    o[2] = 0.48860251190291987f * z;
    o[3] = -0.48860251190291987f * x;
    o[4] = 1.0925484305920792f * xy;
    o[5] = -1.0925484305920792f * yz;
    o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    o[7] = -1.0925484305920792f * xz;
    o[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    o[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
    o[10] = 2.8906114426405538f * xy * z;
    o[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    o[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
    o[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
    o[14] = 1.4453057213202769f * z * (x2 - y2);
    o[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
}

// tcnn SphericalHarmonics degree 4 on in = (d/|d| + 1)/2, mapped back x = in*2-1 (networks.py:145-146)
__device__ __forceinline__ void sh4(float dx, float dy, float dz, float* o) {
    const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
    float x = dx / nrm, y = dy / nrm, z = dz / nrm;
    x = ((x + 1.0f) / 2.0f) * 2.0f - 1.0f;
    y = ((y + 1.0f) / 2.0f) * 2.0f - 1.0f;
    z = ((z + 1.0f) / 2.0f) * 2.0f - 1.0f;
    sh4_poly(x, y, z, o);
}

// Forward state of one tile that the backward needs again.
template <int W>
struct FwdTile {
    half8 x[2];             // B operands of layer 1 (natural order, features 16q+8h+j)
    half8 y1[2][2];         // relu(Y1) as B operands [t][q]
    half8 hb;               // h (16 features, perm order) = rgb-input k-step 1
    half8 sh;               // SH (natural order 8h+j)    = rgb-input k-step 0
    half8 r1[W / 32][2];
    half8 r2[W / 32][2];
    float h0;               // h[0] (f16-rounded) on lanes h==0
    float rgb[3];           // sigmoid outputs on lanes h==0 (fp32); LOGRAD: the layer's raw outputs
};

// Loads of one tile's inputs (feature row halves for this lane, direction), used directly or as
// the next tile's prefetch.
struct TileIn {
    half8 x[2];
    float d[3];
};

// TileIn::x of sample s on lane half h.  feat layouts: row-major (n, 32) f16 (tcnn's encoding
// output), or PLANAR: level-major planes (16, plane_stride) half2 (mfnerf_grid_encode_fw_planar).
template <bool PLANAR>
__device__ __forceinline__ void load_feat(const _Float16* __restrict__ feat, int64_t plane_stride, int64_t s, int h,
                                          half8* x) {
    if constexpr (PLANAR) {
        // x[0] element j = feature 8h+j = level 4h + j/2; x[1]: level 8 + 4h + j/2
        const uint32_t* P = reinterpret_cast<const uint32_t*>(feat);
        uint32_t u[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u[k] = P[(int64_t)(4 * h + k) * plane_stride + s];
            u[4 + k] = P[(int64_t)(8 + 4 * h + k) * plane_stride + s];
        }
        x[0] = *reinterpret_cast<const half8*>(&u[0]);
        x[1] = *reinterpret_cast<const half8*>(&u[4]);
    } else {
        const half8* row = reinterpret_cast<const half8*>(feat + s * 32);
        x[0] = row[h];
        x[1] = row[2 + h];
    }
}

// The forward of P independent tiles, stage by stage: each layer's MFMAs for every tile, then the
// next layer.  The scheduler keeps this source order at one wave per SIMD, so a tile's packing
// (VALU) overlaps the next tile's MFMAs, and one fragment read from LDS serves all P tiles.
// LOGRAD: the rgb head has no output activation (NGP(rgb_act='None'), networks.py:134-155): T.rgb is
// the last layer's fp32 accumulator, the log-radiance before tcnn's fp16 rounding.
template <int W, bool DENSITY_ONLY, int P, bool ONE_TILE_FRAGS = false, bool LOGRAD = false>
__device__ __forceinline__ void forward_tiles(const _Float16* lds, int lane, const TileIn* I, const bool* valid,
                                              FwdTile<W>* T) {
    using G = Geo<W>;
    constexpr int MT = G::MT;
    const int h = lane >> 5;
    const f32x16 z = {};
    // xyz layer 1: Y1^T = W1 X^T
    {
        const half8 f0 = lds_frag(lds, G::F1 + 0, lane), f1 = lds_frag(lds, G::F1 + 1, lane);
        const half8 f2 = lds_frag(lds, G::F1 + 2, lane), f3 = lds_frag(lds, G::F1 + 3, lane);
        f32x16 y1a[P], y1b[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            T[q].x[0] = I[q].x[0];
            T[q].x[1] = I[q].x[1];
            y1a[q] = mfma(f0, T[q].x[0], z);
            y1a[q] = mfma(f1, T[q].x[1], y1a[q]);
            y1b[q] = mfma(f2, T[q].x[0], z);
            y1b[q] = mfma(f3, T[q].x[1], y1b[q]);
        }
#pragma unroll
        for (int q = 0; q < P; ++q) {
            T[q].y1[0][0] = pack8<0, true>(y1a[q]); T[q].y1[0][1] = pack8<8, true>(y1a[q]);
            T[q].y1[1][0] = pack8<0, true>(y1b[q]); T[q].y1[1][1] = pack8<8, true>(y1b[q]);
        }
    }
    // xyz layer 2: H^T = W2 relu(Y1)^T (rows 0..15 valid)
    {
        half8 f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = lds_frag(lds, G::F2 + i, lane);
        f32x16 ha[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            ha[q] = mfma(f[0], T[q].y1[0][0], z);
            ha[q] = mfma(f[1], T[q].y1[0][1], ha[q]);
            ha[q] = mfma(f[2], T[q].y1[1][0], ha[q]);
            ha[q] = mfma(f[3], T[q].y1[1][1], ha[q]);
        }
#pragma unroll
        for (int q = 0; q < P; ++q) {
            T[q].hb = pack8<0, false>(ha[q]);   // the fp16 network output of tcnn
            T[q].h0 = (float)T[q].hb[0];        // row 0 on lanes h==0
        }
    }
    if (DENSITY_ONLY) return;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        float shv[16];
        sh4(I[q].d[0], I[q].d[1], I[q].d[2], shv);  // (0/0 on invalid lanes, selected away: no branch)
#pragma unroll
        for (int i = 0; i < 16; ++i) shv[i] = valid[q] ? shv[i] : 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // select the loaded VALUES (a conditional of the two array lvalues is an lvalue: a load
            // through a selected pointer, which kept shv in scratch memory)
            const float lo = shv[j], hi = shv[8 + j];
            T[q].sh[j] = (_Float16)(h ? hi : lo);
        }
    }
    // rgb layer 1
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const half8 f0 = lds_frag(lds, G::F3 + 2 * mt, lane), f1 = lds_frag(lds, G::F3 + 2 * mt + 1, lane);
        f32x16 a[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            a[q] = mfma(f0, T[q].sh, z);
            a[q] = mfma(f1, T[q].hb, a[q]);
        }
#pragma unroll
        for (int q = 0; q < P; ++q) { T[q].r1[mt][0] = pack8<0, true>(a[q]); T[q].r1[mt][1] = pack8<8, true>(a[q]); }
    }
    // rgb layer 2
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        // the forward kernel: one output tile's fragments at a time -- the scheduler otherwise hoists
        // all of layer 2's fragment reads (W = 128: 32 of them, 332 registers, one wave per SIMD;
        // with the barrier 128 registers, four).  Not in the backward's recomputation, whose
        // workgroups hold a whole CU's LDS (one wave per SIMD either way) and which ran 44 us slower
        // with it at W = 128 (r6f)
        if constexpr (ONE_TILE_FRAGS) __builtin_amdgcn_sched_barrier(0);
        f32x16 a[P];
#pragma unroll
        for (int q = 0; q < P; ++q) a[q] = z;
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const half8 f = lds_frag(lds, G::F4 + mt * G::KC + t * 2 + k, lane);
#pragma unroll
                for (int q = 0; q < P; ++q) a[q] = mfma(f, T[q].r1[t][k], a[q]);
            }
#pragma unroll
        for (int q = 0; q < P; ++q) { T[q].r2[mt][0] = pack8<0, true>(a[q]); T[q].r2[mt][1] = pack8<8, true>(a[q]); }
    }
    // rgb layer 3 (rows 0..2 = rgb logits on lanes h==0)
    f32x16 o[P];
#pragma unroll
    for (int q = 0; q < P; ++q) o[q] = z;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const half8 f = lds_frag(lds, G::F5 + t * 2 + k, lane);
#pragma unroll
            for (int q = 0; q < P; ++q) o[q] = mfma(f, T[q].r2[t][k], o[q]);
        }
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (LOGRAD) T[q].rgb[c] = o[q][c];
            else T[q].rgb[c] = 1.0f / (1.0f + __expf(-o[q][c]));
        }
}

}  // namespace mfn_field
