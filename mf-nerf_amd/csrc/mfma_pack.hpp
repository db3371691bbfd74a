// mfma_pack.hpp -- what every v_mfma_f32_32x32x16_f16 unit shares (field_fw.hip, field_bw.hip,
// render.hip, mlp.hip): the operand types, the MFMA itself, the 1-KiB lane-linear weight fragments
// in LDS (their k order, the copy into LDS, one lane's read), and fp32 accumulator halves -> f16 B
// operands with the ReLU and the ReLU backward mask done on the packed halves.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace mfn {

__device__ __forceinline__ f32x16 mfma(const half8& a, const half8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// k index carried by element j of lane half h (natural B order, or accumulator-as-operand order)
__device__ __forceinline__ int k_of(int j, int h, int perm) { return perm ? 8 * (j >> 2) + 4 * h + (j & 3) : 8 * h + j; }

// the workgroup copies n_frags packed fragments (64 lanes x 8 f16 each) into LDS, then synchronises
__device__ __forceinline__ void load_frags(_Float16* lds, const _Float16* __restrict__ packed, int n_frags) {
    const uint4* src = reinterpret_cast<const uint4*>(packed);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    for (int i = threadIdx.x; i < n_frags * 64; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// this lane's 8 halves of fragment f (ds_read_b128, conflict-free)
__device__ __forceinline__ half8 lds_frag(const _Float16* lds, int f, int lane) {
    return *reinterpret_cast<const half8*>(lds + (f * 64 + lane) * 8);
}

typedef short short2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
union H8 { half8 h; half2v p[4]; short2v s[4]; uint32_t w[4]; };

// ReLU applied AFTER the round to f16, on the packed halves as int16 (v_pk_max_i16): an f16 and its
// bits order the same way for non-negative values and every negative f16 (-0 included) is a
// negative int16, so max(bits, 0) == f16(max(v, 0)) for every finite v -- 4 packed ops per 8 values
// instead of a canonicalising v_max_f32 pair per value (IEEE mode).  A NaN stays NaN here.
template <int BASE, bool RELU>
__device__ __forceinline__ half8 pack8(const f32x16& a) {
    H8 r;
#pragma unroll
    for (int w = 0; w < 4; ++w) {  // v_cvt_pk_f16_f32 (round to nearest even) per pair
        const float2v p = {a[BASE + 2 * w], a[BASE + 2 * w + 1]};
        r.p[w] = __builtin_convertvector(p, half2v);
    }
    if (RELU) {
        const short2v zero = {0, 0};
#pragma unroll
        for (int w = 0; w < 4; ++w) r.s[w] = __builtin_elementwise_max(r.s[w], zero);
    }
    return r.h;
}

// zero the packed dY halves where the forward activation y (f16, post-ReLU: +0 or positive, never
// negative) is not positive: dY * min(bits(y), 1) on the packed halves (v_pk_min_u16 +
// v_pk_mul_lo_u16), bit-identical to selecting on (float)y > 0 before the round to f16
__device__ __forceinline__ half8 relu_mask8(const half8& d, const half8& y) {
    H8 D, Y;
    D.h = d;
    Y.h = y;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t m;
        // the 1s come from a register: an inline constant of a packed op feeds only the low half
        asm("v_pk_min_u16 %0, %1, %3\n\tv_pk_mul_lo_u16 %0, %2, %0"
            : "=&v"(m)
            : "v"(Y.w[w]), "v"(D.w[w]), "v"(0x00010001u));
        D.w[w] = m;
    }
    return D.h;
}

}  // namespace mfn
