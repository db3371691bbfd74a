// field_bw.hip -- the backward of the NGP field head (the networks, the forward and the MFMA layout:
// field_fw.hip; the recomputed forward: field_fwd.hpp; the weight fragments: field_pack.hpp).
//
// Data gradients chain through accumulators exactly like the forward ("T" orientation: channel on
// the MFMA row, sample on the lane).  Weight gradients dW = dY^T X reduce over SAMPLES, which must
// therefore sit in the MFMA K dimension, i.e. inside each lane's registers -- the transpose of the
// T operands, the "S" orientation (channel on the lane, samples in the registers): each T chunk is
// written to a per-wave LDS tile image and read back with the transposing ds_read_b64_tr_b16
// (t_put / s_get below; exact, no wave-level synchronisation).
//   dW[out][in] (32x32 tile) += S(dY)[out-tile] x S(X)[in-tile], K = the tile's 32 samples (2 MFMAs)
// The dW tiles accumulate across all sample tiles a workgroup processes (persistent grid) in
// registers, split over its waves (field_bw_coop_kernel), then one slab row per workgroup, summed
// in a fixed order by slab_reduce_kernel.
#include "common.hpp"
#include "mfma_pack.hpp"
#include "field_pack.hpp"
#include "field_fwd.hpp"
#include "field_width.hpp"
#include "../../include/mfnerf.h"

using namespace mfn;
using namespace mfn_field;

namespace {

// 4 waves per workgroup, each the forward + data-gradient chain of its own 32-sample tile,
// the weight-gradient tiles split over the waves (field_bw_coop_kernel).
// Rounds 1-4 held every tile in each wave (one wave per SIMD; at W = 128 a second pass recomputed the
// forward for dWr2's 16 tiles: 0.46 vs 0.23 ms on the mf128 step, profiles/r05_v8_*).
// Measured and not kept (rounds 1-2): every tile in an LDS image with two waves per SIMD (ds_add_f32
// per sample tile; W = 128: 836 vs 171 us), dWr2 by LDS atomics beside the register tiles (3.4 ms
// per 983k samples), Wr2^T read from global memory, two sample tiles per loop trip (~560 registers:
// 80-147 spilled, 177 vs 122 us inside the step).
// The transpose image of a tile: [sample][channel] in 64-B rows of eight 8-B chunks (4 channels), the
// chunk index XOR-swizzled with (row >> 1) & 7 (2-way bank conflicts on the writes, none on the reads);
// ds_read_b64_tr_b16 hands each 16-lane group a 4-sample x 16-channel block column by column
// (cdna_hip_programming.md T10).  The S operand's k order is the one the accumulator-as-operand
// packing has (element j of lane half h = sample 8(j>>2) + 4h + (j&3) of the k-step), so both operands
// of every dW product agree.  (Rounds 1-2 transposed on the matrix core instead: D = T x I,
// 2 MFMAs + 8 packing instructions per tile, ~30 of the 98 MFMAs of a sample tile.)
constexpr int TILE_HALFS = 32 * 32;
constexpr size_t TILE_BYTES = TILE_HALFS * 2;
typedef short short4v __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int tix(int row, int chunk) { return row * 32 + 4 * (chunk ^ ((row >> 1) & 7)); }

// this lane's 8 channels of a T chunk (sample = lane & 31) into the tile image; cbase = first channel / 4;
// perm: element j is channel 4 cbase + 8(j>>2) + 4h + (j&3) (a packed accumulator), else 4 cbase + 8h + j
__device__ __forceinline__ void t_put(_Float16* slot, int lane, const half8& v, int cbase, bool perm) {
    const int r = lane & 31, h = lane >> 5;
    const int c0 = cbase + (perm ? h : 2 * h), c1 = cbase + (perm ? 2 + h : 2 * h + 1);
    H8 u;
    u.h = v;
    *reinterpret_cast<u32x2*>(slot + tix(r, c0)) = u32x2{u.w[0], u.w[1]};
    *reinterpret_cast<u32x2*>(slot + tix(r, c1)) = u32x2{u.w[2], u.w[3]};
}

__device__ __forceinline__ u32x2 tr_read(const _Float16* p) {
    typedef __attribute__((address_space(3))) short4v* lds_s4;
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p)));
}

// S operands (K = samples 0..15 / 16..31 of the tile) of one 32-channel tile given as two T chunks
struct SOp { half8 k[2]; };

// the S operand of a tile image (t_put): lane 4q+p of 16-lane group g supplies row (sample)
// 16s + 4h + q (+8) at channels 16(g&1) + 4p; lane i of the group gets channel 16(g&1) + i
__device__ __forceinline__ SOp s_get(const _Float16* slot, int lane) {
    const int h = lane >> 5, q = (lane >> 2) & 3, c = 4 * ((lane >> 4) & 1) + (lane & 3);
    SOp o;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int r0 = 16 * s + 4 * h + q;
        const u32x2 a = tr_read(slot + tix(r0, c)), b = tr_read(slot + tix(r0 + 8, c));
        H8 u;
        u.w[0] = a[0]; u.w[1] = a[1]; u.w[2] = b[0]; u.w[3] = b[1];
        o.k[s] = u.h;
    }
    return o;
}

// one dW tile += dY x X (K = the tile's 32 samples: 2 MFMAs) into a PERSISTENT accumulator pinned to
// AGPRs: with MFMA results in VGPRs (-amdgpu-mfma-vgpr-form, which the data-gradient chain needs) the
// compiler otherwise moves each accumulator tile AGPR <-> VGPR around every update (~500 v_accvgpr
// moves per sample tile with 12 of them).
// The leading s_nop covers the VALU-write -> MFMA-read hazard on the packed operands (the compiler's
// hazard recognizer does not look into inline asm); back-to-back accumulation into the same
// registers needs none.  Readers of the accumulators wait with xdl_drain().
__device__ __forceinline__ void dw_acc_agpr(f32x16& acc, const SOp& dy, const SOp& x) {
    asm("s_nop 2\n\t"
        "v_mfma_f32_32x32x16_f16 %0, %1, %2, %0\n\t"
        "v_mfma_f32_32x32x16_f16 %0, %3, %4, %0"
        : "+a"(acc)
        : "v"(dy.k[0]), "v"(x.k[0]), "v"(dy.k[1]), "v"(x.k[1]));
}
__device__ __forceinline__ void xdl_drain() { asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory"); }

// A workgroup's slab row holds non-finite values: raise the step's flag now.  Every row finite
// bounds every slab sum: |row value| <= (samples of one workgroup) x 65504^2 (fp16 operands,
// f32 accumulation) ~ 1e13, 512 rows ~ 5e15, far below the f32 range -- so with the rows checked
// here the flag is final when field_bw returns, even with the fold deferred past the table's Adam
// (mfnerf_grid_encode_bw_binned_adam_all's slab tail).
__device__ __forceinline__ void slab_row_flag(int32_t* nonfinite, bool bad) {
    if (nonfinite && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(nonfinite, 1);
}

// store one 32x32 dW tile (row = out 32*ot + (i&3)+8(i>>2)+4h, col = in 32*it + lane&31) into a
// row-major fp32 LDS image of a (rows x cols) matrix (every entry belongs to one tile, so the waves'
// stores are disjoint); rows/cols are compile-time at every call, so the register rows that can
// never be in range are dropped statically
__device__ __forceinline__ void dw_store32(float* img, const f32x16& a, int ot, int it, int rows, int cols, int lane) {
    const int col = 32 * it + (lane & 31), h = lane >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = 32 * ot + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (row < rows && col < cols) img[row * cols + col] = a[i];
    }
}

// dL/dd of one sample from dL/dSH (mfnerf_field_bw_inputs).  dsh is the 32-row accumulator of
// d[SH;h] = Wr1^T dR1, still scaled by the loss scale: register i < 8 of lane half h is SH row
// (i&3) + 8(i>>2) + 4h, so h = 0 holds rows {0..3, 8..11} and h = 1 rows {4..7, 12..15} of the
// sample lane&31.  Each half applies its own eight rows of the SH4 Jacobian (J^T g, in dn = d/|d|;
// the encoding's (dn+1)/2 and the SH's 2u-1 cancel, the fp16 rounding of SH counts as identity):
// per register the Jacobian row is selected by h and folded into the running 3-vector at once, so
// nothing but the 3-vector and the direction's products stays live.  ONE exchange with lane^32 adds
// the two halves' partial 3-vectors (a + b on one side, b + a on the other: the same bits).  Then
// the normalisation: dL/dd = (g - dn (dn . g)) / |d|.  All fp32.
__device__ __forceinline__ void sh4_bw_dir(const f32x16& dsh, int h, float invS, const float* d, float* out) {
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float x = d[0] / nrm, y = d[1] / nrm, z = d[2] / nrm;
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    // (sh4_poly's coefficients, field_fwd.hpp: this is its Jacobian)
    constexpr float c1 = 0.48860251190291987f, c2 = 1.0925484305920792f, c3 = 0.94617469575755997f,
                    c4 = 0.54627421529603959f, c5 = 0.59004358992664352f, c6 = 2.8906114426405538f,
                    c7 = 0.45704579946446572f, c8 = 0.3731763325901154f, c9 = 1.4453057213202769f;
    const float a = c7 * (1.0f - 5.0f * z2), b = 3.0f * c5 * (y2 - x2);
    const bool hi = h != 0;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    // register i: the Jacobian row (d/dx, d/dy, d/dz) of SH row lo (h == 0) or lo + 4 (h == 1)
    auto row = [&](int i, float lx, float ly, float lz, float hx, float hy, float hz) {
        const float v = dsh[i] * invS;
        gx += v * (hi ? hx : lx);
        gy += v * (hi ? hy : ly);
        gz += v * (hi ? hz : lz);
    };
    row(0, 0.0f, 0.0f, 0.0f, c2 * y, c2 * x, 0.0f);                                        // rows 0 | 4
    row(1, 0.0f, -c1, 0.0f, 0.0f, -c2 * z, -c2 * y);                                       //      1 | 5
    row(2, 0.0f, 0.0f, c1, 0.0f, 0.0f, 2.0f * c3 * z);                                     //      2 | 6
    row(3, -c1, 0.0f, 0.0f, -c2 * z, 0.0f, -c2 * x);                                       //      3 | 7
    row(4, 2.0f * c4 * x, -2.0f * c4 * y, 0.0f, 0.0f, 0.0f, c8 * (15.0f * z2 - 3.0f));     //      8 | 12
    row(5, -6.0f * c5 * xy, b, 0.0f, a, 0.0f, -10.0f * c7 * xz);                           //      9 | 13
    row(6, c6 * yz, c6 * xz, c6 * xy, 2.0f * c9 * xz, -2.0f * c9 * yz, c9 * (x2 - y2));    //     10 | 14
    row(7, 0.0f, a, -10.0f * c7 * yz, b, 6.0f * c5 * xy, 0.0f);                            //     11 | 15
    gx += __shfl_xor(gx, 32, 64);
    gy += __shfl_xor(gy, 32, 64);
    gz += __shfl_xor(gz, 32, 64);
    const float t = x * gx + y * gy + z * gz;
    out[0] = (gx - x * t) / nrm;
    out[1] = (gy - y * t) / nrm;
    out[2] = (gz - z * t) / nrm;
}

// ---------------------------------------------------------------- cooperative backward
// field_bw_coop_kernel<W, PLANAR, DDIRS>, both widths.  Each of the workgroup's 4 waves runs the
// forward and the data-gradient chain of its own 32-sample tile; the weight-gradient tiles are split
// over the waves.  The weight-gradient operands (the transposed T chunks, t_put) are written stage by
// stage into the wave's transpose images, the workgroup synchronises, and each wave accumulates ITS
// tiles of that stage over all four waves' sample tiles (waves 0..3 in order: a fixed summation
// order, deterministic).  The chain's next MFMAs are issued between a stage's writes and its products.
//
// W = 64 (round 4): 12 tiles, 3 per wave -- 48 accumulator registers, so a wave fits 256 registers
// and TWO workgroups share a CU, two waves per SIMD.  LDS: the 44 fragments + 4 images per wave,
// 76 KB per workgroup.  Tiles per wave:
//   wave 0: dWr3[0], dWr2[0][0], dW2[0]      wave 2: dWr1[0], dWr2[1][0], dW1[0]
//   wave 1: dWr3[1], dWr2[0][1], dW2[1]      wave 3: dWr1[1], dWr2[1][1], dW1[1]
// Stages (images per wave): S1 dO, R2 x2 | S2 dR2 x2, R1 x2 | S3 dR1 x2, [SH;h] | S4 dh, Y1 x2 |
// S5 dY1 x2, X.
// Before (rounds 1-3) every wave held all 12 tiles (192 accumulator registers + ~170 for the
// chain): one wave per SIMD, nothing hid the chain's dependencies (PMC: waiting 56 % of its cycles).
//
// W = 128 (round 5; configs 3/4, MF-NeRF's benchmark field): 28 tiles, 7 per wave -- 112
// accumulator registers pinned to AGPRs, one wave per SIMD.  LDS: all 106 fragments (106 KB) beside
// 6 images per wave (48 KB), one workgroup per CU.  Tiles per wave w:
//   dWr3[w] (16 x 32 block w of the 16 x 128), dWr2[w][0..3] (row block w), dWr1[w],
//   and dW2[w] (waves 0, 1) or dW1[w - 2] (waves 2, 3).
// Stages (images per wave): S1 dO, R2 x4 | S2a dR2 x4, R1[0..1] | S2b R1[2..3] over R1[0..1] |
// S3 dR1 x4, [SH;h] | S4 dh, Y1 x2 | S5 dY1 x2, X.
// Before (rounds 1-4) every wave held all tiles but dWr2's 16 (448 accumulator registers do not
// fit), and a second pass recomputed the forward and dR2 for them: 0.46 ms of the 1.67 ms mf128
// step (profiles/r04_final_bench_mf128.json).
template <int W>
struct CoopGeo {
    static constexpr int SLOTS = W == 64 ? 4 : 6;          // transpose images per wave live at once
    static constexpr int BLOCKS = W == 64 ? 512 : 256;     // persistent workgroups = slab rows (two | one per CU)
    static constexpr int WAVES_PER_SIMD = W == 64 ? 2 : 1;
    static constexpr size_t LDS = (size_t)Geo<W>::N * FRAG_HALFS * 2 + (size_t)4 * SLOTS * TILE_BYTES;
    static_assert(W != 64 || LDS <= 80 * 1024, "two cooperative workgroups per CU");
    static_assert(W != 128 || LDS <= 160 * 1024, "one cooperative W = 128 workgroup per CU");
};

// LOGRAD (mfnerf_field_bw*_lograd): dL_drgb is dL/dlograd of the head without its sigmoid
template <int W, bool PLANAR, bool DDIRS, bool LOGRAD = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CoopGeo<W>::WAVES_PER_SIMD))) void field_bw_coop_kernel(
    const _Float16* __restrict__ feat, int64_t plane_stride, const float* __restrict__ dirs, int64_t n,
    const int32_t* __restrict__ n_dev, const _Float16* __restrict__ packed, const float* __restrict__ dL_dsigma,
    const float* __restrict__ dL_drgb, float grad_scale, const float* __restrict__ scale_dev,
    float* __restrict__ dL_dfeat, float* __restrict__ slab, int32_t* __restrict__ nonfinite, float* __restrict__ level_l1,
    float* __restrict__ dL_ddirs) {
    using G = Geo<W>;
    constexpr int MT = G::MT, SLOTS = CoopGeo<W>::SLOTS;
    constexpr int oR1 = N_XYZ_PARAMS, oR2 = oR1 + W * 32, oR3 = oR2 + W * W;
    constexpr size_t IMG_OFF = (size_t)G::N * FRAG_HALFS * 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* lds_base = reinterpret_cast<_Float16*>(smem);
    load_frags(lds_base, packed, G::N);
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform)
    const int r = lane & 31, h = lane >> 5;
    const float S = scale_dev ? *scale_dev : grad_scale, invS = 1.0f / S;
    const f32x16 z = {};
    // this wave's weight-gradient tiles (tables above): plain variables, the other width's unused
    // and free (as members of a per-width struct they compile to other code)
    f32x16 a_r13 = z, a_r2 = z;          // W = 64: dWr3 (waves 0, 1) | dWr1 (waves 2, 3); dWr2[w >> 1][w & 1]
    f32x16 a_r3 = z, a_r1 = z;           // W = 128: dWr3[w], dWr1[w]
    f32x16 a_x = z;                      // both: dW2[w] (waves 0, 1) | dW1[w - 2] (waves 2, 3)
    f32x16 a_r2w[MT];                    // W = 128: dWr2[w][0..3]
#pragma unroll
    for (int i = 0; i < MT; ++i) a_r2w[i] = z;
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int64_t tiles = div_up<int64_t>(nn, 32);
    const int64_t groups = div_up<int64_t>(tiles, 4);  // group g = tiles 4g .. 4g+3, one per wave
    struct BwIn { TileIn I; float gs, g0, g1, g2; bool live; };
    BwIn nx;
    // branch-free: every lane loads (index clamped), the incoming gradients are zeroed where
    // the sample is out of range or on lanes h == 1 -- an idle wave's tile contributes exact zeros
    auto fetch = [&](int64_t tile, BwIn& o) {
        const int64_t s = tile * 32 + r;
        const bool v = s < nn && h == 0;
        const int64_t sc = max<int64_t>(0, min<int64_t>(s, nn - 1));
        load_feat<PLANAR>(feat, plane_stride, sc, h, o.I.x);
        o.I.d[0] = dirs[3 * sc]; o.I.d[1] = dirs[3 * sc + 1]; o.I.d[2] = dirs[3 * sc + 2];
        o.gs = dL_dsigma[sc]; o.g0 = dL_drgb[3 * sc]; o.g1 = dL_drgb[3 * sc + 1]; o.g2 = dL_drgb[3 * sc + 2];
        o.live = v;
    };
    auto zero_grads = [&](BwIn& o) {
        o.gs = o.live ? o.gs : 0.0f;
        o.g0 = o.live ? o.g0 : 0.0f;
        o.g1 = o.live ? o.g1 : 0.0f;
        o.g2 = o.live ? o.g2 : 0.0f;
    };
    if ((int64_t)blockIdx.x < groups) fetch(4 * (int64_t)blockIdx.x + wid, nx);
    bool bad = false;
    float l1a[4] = {0.f, 0.f, 0.f, 0.f}, l1b[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        int opaque = 0;
        asm volatile("" : "+s"(opaque));
        const _Float16* lds = lds_base + opaque;
        _Float16* area = lds_base + opaque + IMG_OFF / 2;
        auto slot = [&](int u, int k) { return area + (u * SLOTS + k) * TILE_HALFS; };
        auto put2 = [&](_Float16* sl, const half8* v) {  // a 32-channel tile as two perm chunks
            t_put(sl, lane, v[0], 0, true);
            t_put(sl, lane, v[1], 4, true);
        };
        // this wave's tile of the group; the next group's inputs are loaded while it computes
        const int64_t tile = 4 * g + wid;
        BwIn in = nx;
        zero_grads(in);
        fetch(4 * (g + (int64_t)gridDim.x) + wid, nx);  // (clamped past the end)
        const bool valid = tile * 32 + r < nn;
        FwdTile<W> T;
        forward_tiles<W, false, 1, false, LOGRAD>(lds, lane, &in.I, &valid, &T);
        half8 dOb;
        {
            f32x16 dO = z;
            if constexpr (LOGRAD) {
                dO[0] = in.g0 * S;
                dO[1] = in.g1 * S;
                dO[2] = in.g2 * S;
            } else {
                dO[0] = in.g0 * S * T.rgb[0] * (1.0f - T.rgb[0]);
                dO[1] = in.g1 * S * T.rgb[1] * (1.0f - T.rgb[1]);
                dO[2] = in.g2 * S * T.rgb[2] * (1.0f - T.rgb[2]);
            }
            dOb = pack8<0, false>(dO);
        }
        //    dR2 = Wr3^T dO, masked by R2 > 0
        half8 dr2p[MT][2];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x16 a = mfma(lds_frag(lds, G::B5 + mt, lane), dOb, z);
            dr2p[mt][0] = relu_mask8(pack8<0, false>(a), T.r2[mt][0]);
            dr2p[mt][1] = relu_mask8(pack8<8, false>(a), T.r2[mt][1]);
        }
        // ---- S1: dO, R2 -> dWr3 (W = 64: waves 0, 1; W = 128: dWr3[w])
        // (S1-S3's puts stay per width: W = 64's two as a loop over MT compile to other code)
        t_put(slot(wid, 0), lane, dOb, 0, true);  // (channels 16..31 stale: rows 16..31 of dWr3, dropped)
        if constexpr (W == 64) {
            put2(slot(wid, 1), T.r2[0]);
            put2(slot(wid, 2), T.r2[1]);
            __syncthreads();
            if (wid < 2) {
#pragma unroll
                for (int u = 0; u < 4; ++u) dw_acc_agpr(a_r13, s_get(slot(u, 0), lane), s_get(slot(u, 1 + wid), lane));
            }
        } else {
#pragma unroll
            for (int i = 0; i < MT; ++i) put2(slot(wid, 1 + i), T.r2[i]);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) dw_acc_agpr(a_r3, s_get(slot(u, 0), lane), s_get(slot(u, 1 + wid), lane));
        }
        //    dR1 = Wr2^T dR2, masked by R1 > 0
        half8 dr1p[MT][2];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            f32x16 a = z;
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int k = 0; k < 2; ++k) a = mfma(lds_frag(lds, G::B4 + mt * G::KC + t * 2 + k, lane), dr2p[t][k], a);
            dr1p[mt][0] = relu_mask8(pack8<0, false>(a), T.r1[mt][0]);
            dr1p[mt][1] = relu_mask8(pack8<8, false>(a), T.r1[mt][1]);
        }
        __syncthreads();
        // ---- S2 (W = 128: S2a): dR2, R1[0..1] -> dWr2 (W = 64: one tile per wave; W = 128: dWr2[w][0..1])
        if constexpr (W == 64) {
            put2(slot(wid, 0), dr2p[0]);
            put2(slot(wid, 1), dr2p[1]);
            put2(slot(wid, 2), T.r1[0]);
            put2(slot(wid, 3), T.r1[1]);
        } else {
#pragma unroll
            for (int o = 0; o < MT; ++o) put2(slot(wid, o), dr2p[o]);
            put2(slot(wid, 4), T.r1[0]);
            put2(slot(wid, 5), T.r1[1]);
        }
        //    d[SH;h] = Wr1^T dR1 (rows 16..31 = dh) + TruncExp backward into h[0]
        half8 dhb;
        {
            f32x16 dsh = z;
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int k = 0; k < 2; ++k) dsh = mfma(lds_frag(lds, G::B3 + t * 2 + k, lane), dr1p[t][k], dsh);
            const float dh0 = in.gs * S * __expf(fminf(fmaxf(T.h0, -15.0f), 15.0f));
            dsh[8] = h == 0 ? dsh[8] + dh0 : dsh[8];
            dhb = pack8<8, false>(dsh);
            if constexpr (DDIRS) {  // rows 0..15 = dL/dSH: the chain rule to the sample's direction
                // (the direction is read again: keeping the forward's copy live costs registers)
                __builtin_amdgcn_sched_barrier(0);
                const int64_t s = tile * 32 + r, sc = max<int64_t>(0, min<int64_t>(s, nn - 1));
                const float dv[3] = {dirs[3 * sc], dirs[3 * sc + 1], dirs[3 * sc + 2]};
                float gd[3];
                sh4_bw_dir(dsh, h, invS, dv, gd);
                if (h == 0 && s < nn) {
                    bad |= !(isfinite(gd[0]) && isfinite(gd[1]) && isfinite(gd[2]));
                    dL_ddirs[3 * s] = gd[0]; dL_ddirs[3 * s + 1] = gd[1]; dL_ddirs[3 * s + 2] = gd[2];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        if constexpr (W == 64) {
            const int o = wid >> 1, i = wid & 1;
#pragma unroll
            for (int u = 0; u < 4; ++u) dw_acc_agpr(a_r2, s_get(slot(u, o), lane), s_get(slot(u, 2 + i), lane));
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const SOp d = s_get(slot(u, wid), lane);
                dw_acc_agpr(a_r2w[0], d, s_get(slot(u, 4), lane));
                dw_acc_agpr(a_r2w[1], d, s_get(slot(u, 5), lane));
            }
        }
        //    dY1 = W2^T dh, masked by Y1 > 0; dX = W1^T dY1
        half8 dy1p[2][2];
        f32x16 dx = z;
        {
            const f32x16 a0 = mfma(lds_frag(lds, G::B2 + 0, lane), dhb, z);
            const f32x16 a1 = mfma(lds_frag(lds, G::B2 + 1, lane), dhb, z);
            dy1p[0][0] = relu_mask8(pack8<0, false>(a0), T.y1[0][0]);
            dy1p[0][1] = relu_mask8(pack8<8, false>(a0), T.y1[0][1]);
            dy1p[1][0] = relu_mask8(pack8<0, false>(a1), T.y1[1][0]);
            dy1p[1][1] = relu_mask8(pack8<8, false>(a1), T.y1[1][1]);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int k = 0; k < 2; ++k) dx = mfma(lds_frag(lds, G::B1 + t * 2 + k, lane), dy1p[t][k], dx);
        }
        __syncthreads();
        // dX -> global fp32 (features (i&3)+8(i>>2)+4h), this wave's own tile.  The store sits where
        // each width's schedule has it, so its body is here twice: called as a lambda or a function
        // from the two places it compiles to other code
        if constexpr (W == 64) {
            // ---- S3: dR1, [SH;h] -> dWr1 (waves 2, 3)
            put2(slot(wid, 0), dr1p[0]);
            put2(slot(wid, 1), dr1p[1]);
            t_put(slot(wid, 2), lane, T.sh, 0, false);
            t_put(slot(wid, 2), lane, T.hb, 4, true);
            __syncthreads();
            if (wid >= 2) {
#pragma unroll
                for (int u = 0; u < 4; ++u) dw_acc_agpr(a_r13, s_get(slot(u, wid - 2), lane), s_get(slot(u, 2), lane));
            }
            const int64_t s = tile * 32 + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 o = make_float4(dx[4 * q] * invS, dx[4 * q + 1] * invS, dx[4 * q + 2] * invS, dx[4 * q + 3] * invS);
                bad |= !(isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(o.w));
                if (s < nn) reinterpret_cast<float4*>(dL_dfeat + s * 32)[2 * q + h] = o;
                l1a[q] += fabsf(o.x) + fabsf(o.y);
                l1b[q] += fabsf(o.z) + fabsf(o.w);
            }
        } else {
            // ---- S2b: R1[2..3] over R1[0..1] -> dWr2[w][2..3] (dR2 still in slots 0..3)
            put2(slot(wid, 4), T.r1[2]);
            put2(slot(wid, 5), T.r1[3]);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const SOp d = s_get(slot(u, wid), lane);
                dw_acc_agpr(a_r2w[2], d, s_get(slot(u, 4), lane));
                dw_acc_agpr(a_r2w[3], d, s_get(slot(u, 5), lane));
            }
            const int64_t s = tile * 32 + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 o = make_float4(dx[4 * q] * invS, dx[4 * q + 1] * invS, dx[4 * q + 2] * invS, dx[4 * q + 3] * invS);
                bad |= !(isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(o.w));
                if (s < nn) reinterpret_cast<float4*>(dL_dfeat + s * 32)[2 * q + h] = o;
                l1a[q] += fabsf(o.x) + fabsf(o.y);
                l1b[q] += fabsf(o.z) + fabsf(o.w);
            }
            __syncthreads();
            // ---- S3: dR1, [SH;h] -> dWr1[w]
#pragma unroll
            for (int o = 0; o < MT; ++o) put2(slot(wid, o), dr1p[o]);
            t_put(slot(wid, 4), lane, T.sh, 0, false);
            t_put(slot(wid, 4), lane, T.hb, 4, true);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) dw_acc_agpr(a_r1, s_get(slot(u, wid), lane), s_get(slot(u, 4), lane));
        }
        __syncthreads();
        // ---- S4: dh, Y1 -> dW2 (waves 0, 1)
        t_put(slot(wid, 0), lane, dhb, 0, true);  // (channels 16..31 stale: rows of dW2 dropped)
        put2(slot(wid, 1), T.y1[0]);
        put2(slot(wid, 2), T.y1[1]);
        __syncthreads();
        if (wid < 2) {
#pragma unroll
            for (int u = 0; u < 4; ++u) dw_acc_agpr(a_x, s_get(slot(u, 0), lane), s_get(slot(u, 1 + wid), lane));
        }
        __syncthreads();
        // ---- S5: dY1, X -> dW1 (waves 2, 3)
        put2(slot(wid, 0), dy1p[0]);
        put2(slot(wid, 1), dy1p[1]);
        t_put(slot(wid, 2), lane, T.x[0], 0, false);
        t_put(slot(wid, 2), lane, T.x[1], 4, false);
        __syncthreads();
        if (wid >= 2) {
#pragma unroll
            for (int u = 0; u < 4; ++u) dw_acc_agpr(a_x, s_get(slot(u, wid - 2), lane), s_get(slot(u, 2), lane));
        }
        __syncthreads();  // the images are rewritten by the next group's S1
    }
    if (nonfinite && __any(bad) && lane == 0) atomicOr(nonfinite, 1);

    // ---- epilogue: each tile stored by its owner wave (disjoint) -> one slab row per workgroup
    float* row = slab + (int64_t)blockIdx.x * G::N_DW;
    {
        constexpr int N_IMG = G::N_DW;
        static_assert((size_t)N_IMG * 4 + 64 <= IMG_OFF, "reduction image must fit the fragment area");
        xdl_drain();
        __syncthreads();
        float* img = reinterpret_cast<float*>(smem);
        float* l1_part = img + N_IMG;
        if (threadIdx.x < 16) l1_part[threadIdx.x] = 0.0f;
        __syncthreads();
        if (level_l1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float a = l1a[q], b = l1b[q];
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
                if (r == 0) { atomicAdd(l1_part + 4 * q + 2 * h, a); atomicAdd(l1_part + 4 * q + 2 * h + 1, b); }
            }
        }
        if constexpr (W == 64) {
            if (wid == 0) {
                dw_store32(img + oR3, a_r13, 0, 0, 16, W, lane);
                dw_store32(img + oR2, a_r2, 0, 0, W, W, lane);
                dw_store32(img + 64 * 32, a_x, 0, 0, 16, 64, lane);
            } else if (wid == 1) {
                dw_store32(img + oR3, a_r13, 0, 1, 16, W, lane);
                dw_store32(img + oR2, a_r2, 0, 1, W, W, lane);
                dw_store32(img + 64 * 32, a_x, 0, 1, 16, 64, lane);
            } else if (wid == 2) {
                dw_store32(img + oR1, a_r13, 0, 0, W, 32, lane);
                dw_store32(img + oR2, a_r2, 1, 0, W, W, lane);
                dw_store32(img, a_x, 0, 0, 64, 32, lane);
            } else {
                dw_store32(img + oR1, a_r13, 1, 0, W, 32, lane);
                dw_store32(img + oR2, a_r2, 1, 1, W, W, lane);
                dw_store32(img, a_x, 1, 0, 64, 32, lane);
            }
        } else {
            dw_store32(img + oR3, a_r3, 0, wid, 16, W, lane);
            dw_store32(img + oR1, a_r1, wid, 0, W, 32, lane);
#pragma unroll
            for (int i = 0; i < MT; ++i) dw_store32(img + oR2, a_r2w[i], wid, i, W, W, lane);
            if (wid < 2) dw_store32(img + 64 * 32, a_x, 0, wid, 16, 64, lane);
            else dw_store32(img, a_x, wid - 2, 0, 64, 32, lane);
        }
        __syncthreads();
        bool rbad = false;  // a non-finite weight-gradient partial (see slab_row_flag)
        for (int i = threadIdx.x; i < G::N_DW; i += blockDim.x) {
            const float val = img[i] * invS;
            row[i] = val;
            rbad |= !isfinite(val);
        }
        slab_row_flag(nonfinite, rbad);
        if (level_l1 && threadIdx.x < 16) atomicAdd(level_l1 + threadIdx.x, l1_part[threadIdx.x]);
    }
}

// grad[p] += sum over slab rows (fixed order: deterministic).  64 columns x 4 row groups per block.
template <int W>
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slab, int rows,
                                                          float* __restrict__ gx, float* __restrict__ gr,
                                                          int32_t* __restrict__ nonfinite, int store = 0) {
    // 64 parameters per block as 16 float4 columns x 16 row groups; each thread sums its rows
    // (rows/16, all loads in flight) and the 16 partials are added in a fixed tree order
    constexpr int N_DW = Geo<W>::N_DW;
    static_assert(N_DW % 4 == 0 && N_XYZ_PARAMS % 4 == 0, "float4 columns");
    __shared__ float4 part[16][16];
    const int c = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int p = blockIdx.x * 64 + 4 * c;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p < N_DW) {
        const float4* src = reinterpret_cast<const float4*>(slab + p);
        constexpr int RS = N_DW / 4;  // row stride in float4
        // 8 rows' loads issued before their adds (same order of adds): 512 slab rows (the coop
        // backward) are 4 round trips per thread instead of 32 -- measured 42 us beside the side
        // stream's march (r4e timeline), whose waves make every dependent round trip longer
        constexpr int U = 8;
        for (int b0 = rg; b0 < rows; b0 += 16 * U) {
            float4 v[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int b = b0 + 16 * k;
                v[k] = b < rows ? src[(int64_t)b * RS] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int k = 0; k < U; ++k)
                if (b0 + 16 * k < rows) { acc.x += v[k].x; acc.y += v[k].y; acc.z += v[k].z; acc.w += v[k].w; }
        }
    }
    part[rg][c] = acc;
    __syncthreads();
    if (rg == 0 && p < N_DW) {
        float4 t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = part[k][c];
#pragma unroll
        for (int w = 8; w > 0; w >>= 1)
#pragma unroll
            for (int k = 0; k < w; ++k) {
                t[k].x += t[k + w].x; t[k].y += t[k + w].y; t[k].z += t[k + w].z; t[k].w += t[k + w].w;
            }
        const float v[4] = {t[0].x, t[0].y, t[0].z, t[0].w};
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = p + k;
            float* dst = q < N_XYZ_PARAMS ? gx + q : gr + (q - N_XYZ_PARAMS);
            *dst = store ? v[k] : *dst + v[k];
            bad |= !isfinite(v[k]);
        }
        if (nonfinite && bad) atomicOr(nonfinite, 1);
    }
}

// the fold of the backward's slab (CoopGeo<W>::BLOCKS rows) into the gradients: added, or stored
template <int W>
void launch_slab_reduce(const void* workspace, float* grad_xyz, float* grad_rgb, int32_t* nonfinite, int store,
                        mfnerf_stream_t stream) {
    hipLaunchKernelGGL(slab_reduce_kernel<W>, dim3((Geo<W>::N_DW + 63) / 64), dim3(256), 0, stream,
                       (const float*)workspace, CoopGeo<W>::BLOCKS, grad_xyz, grad_rgb, nonfinite, store);
}

// the cooperative backward of width W (row-major and planar kernels; workgroups = slab rows and LDS
// from CoopGeo), then the slab fold (unless deferred: grad_xyz null, mfnerf_field_bw_reduce folds
// the slab later)
// DDIRS (mfnerf_field_bw_inputs): the kernels' direction-gradient instantiation, writing dL_ddirs
template <int W, bool DDIRS, bool LOGRAD>
int launch_bw(const void* feat, int64_t ps, const float* dirs, int64_t n, const int32_t* n_dev, const void* packed,
              const float* dL_dsigma, const float* dL_drgb, float grad_scale, const float* scale_dev, float* dL_dfeat,
              float* grad_xyz, float* grad_rgb, void* workspace, int32_t* nonfinite, float* level_l1,
              mfnerf_stream_t stream, float* dL_ddirs) {
    constexpr auto k0 = field_bw_coop_kernel<W, false, DDIRS, LOGRAD>, k1 = field_bw_coop_kernel<W, true, DDIRS, LOGRAD>;
    constexpr size_t lds = CoopGeo<W>::LDS;
    static const hipError_t attr = [] {
        const hipError_t a0 = hipFuncSetAttribute(reinterpret_cast<const void*>(k0),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        const hipError_t a1 = hipFuncSetAttribute(reinterpret_cast<const void*>(k1),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        return a0 != hipSuccess ? a0 : a1;
    }();
    if (attr != hipSuccess) {
        mfn_set_error("field_bw: cannot raise the LDS limit to %d bytes", (int)lds);
        return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(ps > 0 ? k1 : k0, dim3(CoopGeo<W>::BLOCKS), dim3(256), lds, stream, (const _Float16*)feat, ps,
                       dirs, n, n_dev, (const _Float16*)packed, dL_dsigma, dL_drgb, grad_scale, scale_dev, dL_dfeat,
                       (float*)workspace, nonfinite, level_l1, dL_ddirs);
    if (grad_xyz) launch_slab_reduce<W>(workspace, grad_xyz, grad_rgb, nonfinite, 0, stream);
    return MFN_OK;
}

// mfnerf_field_bw (DDIRS off) and mfnerf_field_bw_inputs (on), and their _lograd forms: the same
// checks and launches
template <bool DDIRS, bool LOGRAD = false>
int field_bw_impl(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n, const int32_t* n_dev,
                  const void* packed, int rgb_width, const float* dL_dsigma, const float* dL_drgb, float grad_scale,
                  float* dL_dfeat, float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp,
                  float* level_l1, mfnerf_stream_t stream, float* dL_ddirs) {
    if (!width_ok(rgb_width)) return bad_width(rgb_width);
    if (n < 0 || !(grad_scale >= 0.0f) || (grad_scale == 0.0f && !amp) ||
        (feat_plane_stride != 0 && feat_plane_stride < n)) {
        mfn_set_error("field_bw: bad size, plane stride or grad_scale (0 = dynamic needs amp)"); return MFN_ERR_INVALID;
    }
    if (n == 0) return MFN_OK;
    if (!feat_f16 || !dirs || !packed || !dL_dsigma || !dL_drgb || !dL_dfeat || !workspace || (!grad_xyz != !grad_rgb) ||
        (DDIRS && !dL_ddirs)) {
        mfn_set_error("field_bw: null pointer"); return MFN_ERR_INVALID;
    }
    int32_t* nonfinite = amp ? &amp->nonfinite : nullptr;
    const float* scale_dev = grad_scale == 0.0f ? &amp->scale : nullptr;
    const int st = width_dispatch(rgb_width, [&](auto w) {
        return launch_bw<decltype(w)::value, DDIRS, LOGRAD>(feat_f16, feat_plane_stride, dirs, n, n_dev, packed, dL_dsigma,
                                                    dL_drgb, grad_scale, scale_dev, dL_dfeat, grad_xyz, grad_rgb,
                                                    workspace, nonfinite, level_l1, stream, dL_ddirs);
    });
    if (st != MFN_OK) return st;
    return mfn_check_launch(DDIRS ? "field_bw_inputs" : "field_bw");
}

}  // namespace

extern "C" {

int mfnerf_field_bw_slab_rows(int rgb_width) {
    if (!width_ok(rgb_width)) return -1;
    return width_dispatch(rgb_width, [](auto w) { return CoopGeo<decltype(w)::value>::BLOCKS; });
}

int64_t mfnerf_field_bw_workspace(int64_t n, int rgb_width) {
    (void)n;
    if (!width_ok(rgb_width)) return -1;
    return width_dispatch(rgb_width, [](auto w) {
        constexpr int W = decltype(w)::value;
        return (int64_t)CoopGeo<W>::BLOCKS * Geo<W>::N_DW * 4;
    });
}

int mfnerf_field_bw(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                    const int32_t* n_dev, const void* packed,
                    int rgb_width, const float* dL_dsigma, const float* dL_drgb, float grad_scale, float* dL_dfeat,
                    float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp, float* level_l1,
                    mfnerf_stream_t stream) {
    return field_bw_impl<false>(feat_f16, feat_plane_stride, dirs, n, n_dev, packed, rgb_width, dL_dsigma, dL_drgb,
                                grad_scale, dL_dfeat, grad_xyz, grad_rgb, workspace, amp, level_l1, stream, nullptr);
}

int mfnerf_field_bw_inputs(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                           const int32_t* n_dev, const void* packed,
                           int rgb_width, const float* dL_dsigma, const float* dL_drgb, float grad_scale, float* dL_dfeat,
                           float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp, float* level_l1,
                           float* dL_ddirs, mfnerf_stream_t stream) {
    return field_bw_impl<true>(feat_f16, feat_plane_stride, dirs, n, n_dev, packed, rgb_width, dL_dsigma, dL_drgb,
                               grad_scale, dL_dfeat, grad_xyz, grad_rgb, workspace, amp, level_l1, stream, dL_ddirs);
}

int mfnerf_field_bw_lograd(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                           const int32_t* n_dev, const void* packed,
                           int rgb_width, const float* dL_dsigma, const float* dL_dlograd, float grad_scale, float* dL_dfeat,
                           float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp, float* level_l1,
                           mfnerf_stream_t stream) {
    return field_bw_impl<false, true>(feat_f16, feat_plane_stride, dirs, n, n_dev, packed, rgb_width, dL_dsigma,
                                      dL_dlograd, grad_scale, dL_dfeat, grad_xyz, grad_rgb, workspace, amp, level_l1,
                                      stream, nullptr);
}

int mfnerf_field_bw_inputs_lograd(const void* feat_f16, int64_t feat_plane_stride, const float* dirs, int64_t n,
                                  const int32_t* n_dev, const void* packed,
                                  int rgb_width, const float* dL_dsigma, const float* dL_dlograd, float grad_scale,
                                  float* dL_dfeat, float* grad_xyz, float* grad_rgb, void* workspace, mfnerf_amp_state* amp,
                                  float* level_l1, float* dL_ddirs, mfnerf_stream_t stream) {
    return field_bw_impl<true, true>(feat_f16, feat_plane_stride, dirs, n, n_dev, packed, rgb_width, dL_dsigma,
                                     dL_dlograd, grad_scale, dL_dfeat, grad_xyz, grad_rgb, workspace, amp, level_l1,
                                     stream, dL_ddirs);
}

static int field_bw_fold(int rgb_width, const void* workspace, float* grad_xyz, float* grad_rgb, int32_t* nonfinite,
                         int store, mfnerf_stream_t stream) {
    if (!width_ok(rgb_width)) return bad_width(rgb_width);
    if (!workspace || !grad_xyz || !grad_rgb) { mfn_set_error("field_bw_reduce: null pointer"); return MFN_ERR_INVALID; }
    width_dispatch(rgb_width, [&](auto w) {
        launch_slab_reduce<decltype(w)::value>(workspace, grad_xyz, grad_rgb, nonfinite, store, stream);
    });
    return mfn_check_launch("field_bw_reduce");
}

int mfnerf_field_bw_reduce(int rgb_width, const void* workspace, float* grad_xyz, float* grad_rgb,
                           int32_t* nonfinite, mfnerf_stream_t stream) {
    return field_bw_fold(rgb_width, workspace, grad_xyz, grad_rgb, nonfinite, 0, stream);
}

int mfnerf_field_bw_reduce_store(int rgb_width, const void* workspace, float* grad_xyz, float* grad_rgb,
                                 int32_t* nonfinite, mfnerf_stream_t stream) {
    return field_bw_fold(rgb_width, workspace, grad_xyz, grad_rgb, nonfinite, 1, stream);
}

}  // extern "C"
