// tonemap.hip -- the HDR-NeRF tonemappers of the reference's exposure path (networks.py:81-94,
// 111-132): log-radiance plus log-exposure through one tcnn.Network(1, 1, FullyFusedMLP ReLU/Sigmoid,
// 64 neurons, 1 hidden layer) per colour channel.
//
// tcnn pads the scalar input to a 16-wide half row whose padding its identity encoding fills with
// ones, so the bias-free 16 -> 64 -> 16 MLP is, per channel and sample,
//     x16 = half(float(lograd) + log e)                      (log e rounded to fp32; 0 without exposure)
//     h_j = half(relu(W1h[j,0] * x16 + b_j)),  b_j = sum_{k=1..15} W1h[j,k]
//     y   = half(sigmoid(sum_j W2h[0,j] * h_j))
// with the fp32 weights rounded to half (W1h, W2h) and fp32 accumulation.  A channel's 2048 fp32
// parameters are W1 (64,16) row-major, then W2 (16,64) row-major (tcnn's layout); rows 1..15 of W2
// feed the padded outputs nobody reads.
//
// Nothing padded is ever in memory.  Every workgroup folds the C x 64 triples (W1h[j,0], b_j,
// W2h[0,j]) into LDS once (2.3 KiB for C = 3) and then strides over the samples:
//   forward   a sample per lane; the triples are read at one address by all lanes (LDS broadcast);
//             6 B in, 6 B out and 4 B of exposure per sample at C = 3.
//   backward  fp32 from the same fp16 points, no loss scale: dz = dy * y * (1 - y) from the saved y,
//             h_j recomputed, dh_j = dz * W2h[0,j] where h_j > 0.  A wave takes 64 samples at a time:
//             first a sample per lane for dL/dlograd = sum_j dh_j * W1h[j,0]; then a hidden unit per
//             lane (64 units = the wave width), the wave's 64 (x16, dz) pairs broadcast one after the
//             other (v_readlane), each lane adding its unit's three sums in registers:
//                 sum dh_j * x16 (dW1[j,0]),  sum dh_j (dW1[j,1..15], all equal),  sum dz * h_j (dW2[0,j]).
//             The waves of a workgroup are added in wave order, the workgroup's C x 192 sums stored
//             to its workspace row, and a second launch adds the rows in a fixed order and writes
//             the whole (C,2048) gradient (rows 1..15 of dW2 zero).  No atomics: two runs give the
//             same bits, and the workspace may hold anything on entry.
#include <math.h>

#include "common.hpp"
#include "../../include/mfnerf.h"

namespace {

constexpr int TM_BLOCK = 256, TM_WAVES = TM_BLOCK / 64;
constexpr int TM_H = 64;            // hidden units = lanes of a wave
constexpr int TM_IN = 16;           // padded input width (W1's row length) and padded output rows of W2
constexpr int TM_PARAMS = TM_H * TM_IN + TM_IN * TM_H;  // 2048 per channel
constexpr int TM_SUMS = 3 * TM_H;   // per channel: dW1[:,0], the bias column, dW2[0,:]
constexpr int TM_FW_MAX_BLOCKS = 2048;
constexpr int TM_BW_MAX_BLOCKS = 512;  // workspace rows; 2 waves per SIMD on 256 CUs

static_assert(TM_H == 64, "the backward's weight-gradient pass puts one hidden unit on each lane");
static_assert(TM_PARAMS == 2048, "tcnn's parameter count of Network(1, 1, 64 neurons, 1 hidden layer)");

__device__ __forceinline__ float half_round(float v) { return __half2float(__float2half(v)); }

// (W1h[j,0], b_j, W2h[0,j]) of every channel and hidden unit -> w[c][j]; ends in a barrier
template <int C>
__device__ __forceinline__ void fold_weights(const float* __restrict__ params, float4 (*w)[TM_H]) {
    for (int e = threadIdx.x; e < C * TM_H; e += TM_BLOCK) {
        const int c = e / TM_H, j = e % TM_H;
        const float* row = params + (int64_t)c * TM_PARAMS + j * TM_IN;
        float b = 0.0f;
#pragma unroll
        for (int k = 1; k < TM_IN; ++k) b += half_round(row[k]);
        w[c][j] = make_float4(half_round(row[0]), b, half_round(params[(int64_t)c * TM_PARAMS + TM_H * TM_IN + j]),
                              0.0f);
    }
    __syncthreads();
}

// log of sample i's exposure rounded to fp32 (the double log keeps it the correctly rounded value,
// the same on every implementation); stride 0 = one value for all samples
__device__ __forceinline__ float log_exposure(const float* __restrict__ exposure, int64_t stride, int64_t i) {
    if (!exposure) return 0.0f;
    return (float)log((double)exposure[i * stride]);
}

__device__ __forceinline__ float hidden(float4 q, float x) { return half_round(fmaxf(fmaf(q.x, x, q.y), 0.0f)); }

template <int C>
__global__ __launch_bounds__(TM_BLOCK) void tonemap_fw_kernel(const __half* __restrict__ lograd,
                                                              const float* __restrict__ exposure, int64_t e_stride,
                                                              int64_t n, const float* __restrict__ params,
                                                              __half* __restrict__ rgb) {
    __shared__ float4 w[C][TM_H];
    fold_weights<C>(params, w);
    for (int64_t i = (int64_t)blockIdx.x * TM_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TM_BLOCK) {
        const float le = log_exposure(exposure, e_stride, i);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float x = half_round(__half2float(lograd[i * C + c]) + le);
            float z = 0.0f;
#pragma unroll 16
            for (int j = 0; j < TM_H; ++j) {
                const float4 q = w[c][j];
                z = fmaf(q.z, hidden(q, x), z);
            }
            rgb[i * C + c] = __float2half(1.0f / (1.0f + expf(-z)));
        }
    }
}

__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// partials: (gridDim.x, C, 3, 64) f32, row blockIdx.x written whole by this workgroup
template <int C>
__global__ __launch_bounds__(TM_BLOCK) void tonemap_bw_kernel(const __half* __restrict__ lograd,
                                                              const float* __restrict__ exposure, int64_t e_stride,
                                                              int64_t n, const float* __restrict__ params,
                                                              const __half* __restrict__ rgb,
                                                              const float* __restrict__ dL_drgb,
                                                              float* __restrict__ dL_dlograd,
                                                              float* __restrict__ partials) {
    __shared__ float4 w[C][TM_H];
    __shared__ float fold[TM_WAVES][C * TM_SUMS];
    fold_weights<C>(params, w);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4 mine[C];  // this lane's hidden unit
    float acc[C][3];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        mine[c] = w[c][lane];
        acc[c][0] = acc[c][1] = acc[c][2] = 0.0f;
    }
    const int64_t chunks = (n + 63) / 64;
    for (int64_t ch = (int64_t)blockIdx.x * TM_WAVES + wave; ch < chunks; ch += (int64_t)gridDim.x * TM_WAVES) {
        const int64_t i = ch * 64 + lane;
        const bool valid = i < n;
        const float le = valid ? log_exposure(exposure, e_stride, i) : 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            // a lane past the end carries dz = 0: it adds nothing to any sum
            float x = 0.0f, dz = 0.0f;
            if (valid) {
                x = half_round(__half2float(lograd[i * C + c]) + le);
                const float y = __half2float(rgb[i * C + c]);
                dz = dL_drgb[i * C + c] * y * (1.0f - y);
            }
            // a sample per lane: the input gradient
            float dx = 0.0f;
#pragma unroll 16
            for (int j = 0; j < TM_H; ++j) {
                const float4 q = w[c][j];
                const float dh = hidden(q, x) > 0.0f ? dz * q.z : 0.0f;
                dx = fmaf(dh, q.x, dx);
            }
            if (valid) dL_dlograd[i * C + c] = dx;
            // a hidden unit per lane: the wave's samples in order
            const float4 q = mine[c];
#pragma unroll 8
            for (int s = 0; s < 64; ++s) {
                const float xs = lane_value(x, s), dzs = lane_value(dz, s);
                const float h = hidden(q, xs);
                const float dh = h > 0.0f ? dzs * q.z : 0.0f;
                acc[c][0] = fmaf(dh, xs, acc[c][0]);
                acc[c][1] += dh;
                acc[c][2] = fmaf(dzs, h, acc[c][2]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) fold[wave][c * TM_SUMS + k * TM_H + lane] = acc[c][k];
    __syncthreads();
    for (int e = threadIdx.x; e < C * TM_SUMS; e += TM_BLOCK) {
        float s = fold[0][e];
#pragma unroll
        for (int v = 1; v < TM_WAVES; ++v) s += fold[v][e];
        partials[(int64_t)blockIdx.x * (C * TM_SUMS) + e] = s;
    }
}

// One workgroup per channel: wave q adds rows q, q + 4, ... in order, the four waves are added in
// order, and the channel's 2048 gradient values are written (n_rows = 0 writes zeros).
__global__ __launch_bounds__(TM_BLOCK) void tonemap_bw_finish_kernel(const float* __restrict__ partials, int n_rows,
                                                                     int C, float* __restrict__ grad_params) {
    __shared__ float part[3][TM_WAVES][TM_H];
    const int c = blockIdx.x, j = threadIdx.x & 63, q = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float s = 0.0f;
        for (int b = q; b < n_rows; b += TM_WAVES) s += partials[((int64_t)b * C + c) * TM_SUMS + k * TM_H + j];
        part[k][q][j] = s;
    }
    __syncthreads();
    float* g = grad_params + (int64_t)c * TM_PARAMS;
    for (int e = threadIdx.x; e < TM_H * TM_IN; e += TM_BLOCK) {  // dW1 (64,16): column 0, then the bias columns
        const int u = e / TM_IN, k = e % TM_IN ? 1 : 0;
        g[e] = ((part[k][0][u] + part[k][1][u]) + part[k][2][u]) + part[k][3][u];
    }
    for (int e = threadIdx.x; e < TM_IN * TM_H; e += TM_BLOCK) {  // dW2 (16,64): row 0, zeros below
        const int u = e % TM_H;
        g[TM_H * TM_IN + e] = e < TM_H ? ((part[2][0][u] + part[2][1][u]) + part[2][2][u]) + part[2][3][u] : 0.0f;
    }
}

static_assert(TM_WAVES == 4, "tonemap_bw_finish_kernel adds four waves' sums");

int64_t blocks_for(int64_t n, int64_t cap) {
    const int64_t b = (n + TM_BLOCK - 1) / TM_BLOCK;
    return b < cap ? b : cap;
}

int64_t bw_rows(int64_t n) { return n <= 0 ? 0 : blocks_for(n, TM_BW_MAX_BLOCKS); }

bool check_args(const char* what, const void* lograd, const float* exposure, int64_t e_stride, int64_t n, int C,
                const float* params) {
    if (C != 1 && C != 3) {
        mfn_set_error("%s: C must be 1 or 3, got %d", what, C);
        return false;
    }
    if (n < 0 || n > ((int64_t)1 << 40)) {
        mfn_set_error("%s: bad sample count %lld", what, (long long)n);
        return false;
    }
    if (exposure && e_stride != 0 && e_stride != 1) {
        mfn_set_error("%s: exposure_stride must be 0 (one value) or 1 (per sample), got %lld", what,
                      (long long)e_stride);
        return false;
    }
    if (!params || (n > 0 && !lograd)) {
        mfn_set_error("%s: null pointer", what);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int mfnerf_tonemap_fw(const void* lograd_f16, const float* exposure, int64_t exposure_stride, int64_t n,
                                 int C, const float* params, void* rgb_f16, mfnerf_stream_t stream) {
    if (!check_args("tonemap_fw", lograd_f16, exposure, exposure_stride, n, C, params)) return MFN_ERR_INVALID;
    if (n == 0) return MFN_OK;
    if (!rgb_f16) {
        mfn_set_error("tonemap_fw: null pointer");
        return MFN_ERR_INVALID;
    }
    const unsigned blocks = (unsigned)blocks_for(n, TM_FW_MAX_BLOCKS);
    if (C == 1)
        hipLaunchKernelGGL(tonemap_fw_kernel<1>, dim3(blocks), dim3(TM_BLOCK), 0, stream, (const __half*)lograd_f16,
                           exposure, exposure_stride, n, params, (__half*)rgb_f16);
    else
        hipLaunchKernelGGL(tonemap_fw_kernel<3>, dim3(blocks), dim3(TM_BLOCK), 0, stream, (const __half*)lograd_f16,
                           exposure, exposure_stride, n, params, (__half*)rgb_f16);
    return mfn_check_launch("tonemap_fw");
}

extern "C" int64_t mfnerf_tonemap_bw_workspace(int64_t n, int C) {
    if (C != 1 && C != 3) return 0;
    return bw_rows(n) * C * TM_SUMS * (int64_t)sizeof(float);
}

extern "C" int mfnerf_tonemap_bw(const void* lograd_f16, const float* exposure, int64_t exposure_stride, int64_t n,
                                 int C, const float* params, const void* rgb_f16, const float* dL_drgb,
                                 float* dL_dlograd, float* grad_params, void* workspace, mfnerf_stream_t stream) {
    if (!check_args("tonemap_bw", lograd_f16, exposure, exposure_stride, n, C, params)) return MFN_ERR_INVALID;
    if (!grad_params || (n > 0 && (!rgb_f16 || !dL_drgb || !dL_dlograd || !workspace))) {
        mfn_set_error("tonemap_bw: null pointer");
        return MFN_ERR_INVALID;
    }
    const int rows = (int)bw_rows(n);
    if (rows > 0) {
        if (C == 1)
            hipLaunchKernelGGL(tonemap_bw_kernel<1>, dim3(rows), dim3(TM_BLOCK), 0, stream,
                               (const __half*)lograd_f16, exposure, exposure_stride, n, params,
                               (const __half*)rgb_f16, dL_drgb, dL_dlograd, (float*)workspace);
        else
            hipLaunchKernelGGL(tonemap_bw_kernel<3>, dim3(rows), dim3(TM_BLOCK), 0, stream,
                               (const __half*)lograd_f16, exposure, exposure_stride, n, params,
                               (const __half*)rgb_f16, dL_drgb, dL_dlograd, (float*)workspace);
        const int st = mfn_check_launch("tonemap_bw");
        if (st != MFN_OK) return st;
    }
    hipLaunchKernelGGL(tonemap_bw_finish_kernel, dim3(C), dim3(TM_BLOCK), 0, stream, (const float*)workspace, rows, C,
                       grad_params);
    return mfn_check_launch("tonemap_bw (finish)");
}
