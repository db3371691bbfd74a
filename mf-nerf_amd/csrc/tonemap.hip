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
//
// The training step's forms (mfnerf_tonemap_*_live, C = 3) are the same kernels with the sample count
// read on the device (n is a capacity that only sizes the grid; nothing past *n_dev is touched) and
// rgb kept as fp32 holding the half value, which is what the compositing kernels read.  Beside them:
// the per-ray exposure repeated per sample (mfnerf_expand_exposure), the unit-exposure loss term of
// train.py:172-177 with its gradient added to the tonemappers' (mfnerf_tonemap_unit_loss), and Adam
// for a small parameter group of its own (mfnerf_side_adam_step).
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

// rgb as the kernels keep it: f16 (the module's), or fp32 holding the half value (the step's)
__device__ __forceinline__ float rgb_load(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float rgb_load(const float* p) { return *p; }
__device__ __forceinline__ void rgb_store(__half* p, float y) { *p = __float2half(y); }
__device__ __forceinline__ void rgb_store(float* p, float y) { *p = half_round(y); }

// the live sample count: n, or (n_dev given) min(n, max(*n_dev, 0))
__device__ __forceinline__ int64_t live_count(int64_t n, const int32_t* __restrict__ n_dev) {
    if (!n_dev) return n;
    const int64_t k = *n_dev;
    return k < 0 ? 0 : (k < n ? k : n);
}

template <int C, typename RGB>
__global__ __launch_bounds__(TM_BLOCK) void tonemap_fw_kernel(const __half* __restrict__ lograd,
                                                              const float* __restrict__ exposure, int64_t e_stride,
                                                              int64_t n, const int32_t* __restrict__ n_dev,
                                                              const float* __restrict__ params,
                                                              RGB* __restrict__ rgb) {
    __shared__ float4 w[C][TM_H];
    fold_weights<C>(params, w);
    n = live_count(n, n_dev);
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
            rgb_store(rgb + i * C + c, 1.0f / (1.0f + expf(-z)));
        }
    }
}

__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// partials: (gridDim.x, C, 3, 64) f32, row blockIdx.x written whole by this workgroup
template <int C, typename RGB>
__global__ __launch_bounds__(TM_BLOCK) void tonemap_bw_kernel(const __half* __restrict__ lograd,
                                                              const float* __restrict__ exposure, int64_t e_stride,
                                                              int64_t n, const int32_t* __restrict__ n_dev,
                                                              const float* __restrict__ params,
                                                              const RGB* __restrict__ rgb,
                                                              const float* __restrict__ dL_drgb,
                                                              float* __restrict__ dL_dlograd,
                                                              float* __restrict__ partials) {
    __shared__ float4 w[C][TM_H];
    __shared__ float fold[TM_WAVES][C * TM_SUMS];
    fold_weights<C>(params, w);
    n = live_count(n, n_dev);
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
                const float y = rgb_load(rgb + i * C + c);
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

// rendering.py:142-145: a wave per ray; sample s of [start, start + count) gets the exposure of the
// ray's batch index.  Rows are clipped to [0, min(cap, *n_dev)); a ray index outside the batch writes nothing.
__global__ __launch_bounds__(TM_BLOCK) void expand_exposure_kernel(const float* __restrict__ exposure_ray,
                                                                   const int64_t* __restrict__ rays_a, int64_t n_rays,
                                                                   int64_t cap, const int32_t* __restrict__ n_dev,
                                                                   float* __restrict__ exposure_s) {
    const int lane = threadIdx.x & 63;
    const int64_t live = live_count(cap, n_dev);
    for (int64_t r = (int64_t)blockIdx.x * TM_WAVES + (threadIdx.x >> 6); r < n_rays;
         r += (int64_t)gridDim.x * TM_WAVES) {
        const int64_t ray = rays_a[3 * r], start = rays_a[3 * r + 1], cnt = rays_a[3 * r + 2];
        if (ray < 0 || ray >= n_rays || start < 0 || cnt <= 0 || start >= live) continue;
        const int64_t end = cnt < live - start ? start + cnt : live;
        const float e = exposure_ray[ray];
        for (int64_t s = start + lane; s < end; s += 64) exposure_s[s] = e;
    }
}

// train.py:172-177, one workgroup of 64 lanes per channel: y_c at log-radiance 0 and unit exposure
// (x16 = 0: h_j = half(relu(b_j)), the forward's summation order), the loss term 0.5 (y_c - u)^2 / C
// and its gradient dL/dy_c = (y_c - u) / C through the backward's fp16 points, ADDED to grad_params
// (the x16 column, dW1[:,0], gets dh_j * 0).  Channel c's term is stored to loss_out[c].  Every
// value of the channel's gradient that can be non-zero passes through here: a non-finite one raises
// amp->nonfinite.
__global__ __launch_bounds__(TM_H) void tonemap_unit_kernel(const float* __restrict__ params, int C, float target,
                                                            float* __restrict__ grad_params,
                                                            float* __restrict__ loss_out,
                                                            mfnerf_amp_state* __restrict__ amp) {
    __shared__ float4 w[TM_H];
    const int c = blockIdx.x, j = threadIdx.x;
    {
        const float* row = params + (int64_t)c * TM_PARAMS + j * TM_IN;
        float b = 0.0f;
#pragma unroll
        for (int k = 1; k < TM_IN; ++k) b += half_round(row[k]);
        w[j] = make_float4(half_round(row[0]), b, half_round(params[(int64_t)c * TM_PARAMS + TM_H * TM_IN + j]), 0.0f);
    }
    __syncthreads();
    float z = 0.0f;
#pragma unroll 16
    for (int k = 0; k < TM_H; ++k) {
        const float4 q = w[k];
        z = fmaf(q.z, hidden(q, 0.0f), z);
    }
    const float y = half_round(1.0f / (1.0f + expf(-z)));
    const float d = y - target;
    const float dz = (d / (float)C) * y * (1.0f - y);
    const float4 q = w[j];
    const float h = hidden(q, 0.0f);
    const float dh = h > 0.0f ? dz * q.z : 0.0f;
    float* g = grad_params + (int64_t)c * TM_PARAMS;
    bool bad = !isfinite(g[j * TM_IN]);  // (+ dh * x16 = 0)
    for (int k = 1; k < TM_IN; ++k) {
        const float v = g[j * TM_IN + k] + dh;
        g[j * TM_IN + k] = v;
        bad |= !isfinite(v);
    }
    const float v2 = g[TM_H * TM_IN + j] + dz * h;
    g[TM_H * TM_IN + j] = v2;
    bad |= !isfinite(v2);
    if (j == 0) loss_out[c] = 0.5f * d * d / (float)C;
    if (amp && __any(bad) && j == 0) atomicOr(&amp->nonfinite, 1);
}

// Adam on a small parameter group, one workgroup (mfnerf_pose_step's scheme): skipped when the
// step's non-finite flag is up, which the main optimizer call clears later
constexpr int SA_BLOCK = 1024;
__global__ __launch_bounds__(SA_BLOCK) void side_adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                            float lr, float b1, float b2, float eps,
                                                            int32_t* __restrict__ step_dev,
                                                            const float* __restrict__ lr_dev,
                                                            const mfnerf_amp_state* __restrict__ amp) {
    if (amp && amp->nonfinite != 0) return;  // (uniform)
    const int st = *step_dev + 1;
    if (lr_dev) lr = *lr_dev;
    // 1 - beta^t in double: in fp32 the difference keeps ~1e-5 relative at small t for beta2 = 0.999
    const float bc1 = (float)(1.0 - pow((double)b1, (double)st));
    const float bc2 = (float)(1.0 - pow((double)b2, (double)st));
    for (int64_t i = threadIdx.x; i < n; i += SA_BLOCK) {
        float pp = p[i], mm = m[i], vv = v[i];
        mfn::adam_elem(pp, mm, vv, g[i], b1, b2, eps, lr, bc1, bc2);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
    // every thread has read *step_dev above
    __syncthreads();
    if (threadIdx.x == 0) *step_dev = st;
}

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
        hipLaunchKernelGGL((tonemap_fw_kernel<1, __half>), dim3(blocks), dim3(TM_BLOCK), 0, stream,
                           (const __half*)lograd_f16, exposure, exposure_stride, n, (const int32_t*)nullptr, params,
                           (__half*)rgb_f16);
    else
        hipLaunchKernelGGL((tonemap_fw_kernel<3, __half>), dim3(blocks), dim3(TM_BLOCK), 0, stream,
                           (const __half*)lograd_f16, exposure, exposure_stride, n, (const int32_t*)nullptr, params,
                           (__half*)rgb_f16);
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
            hipLaunchKernelGGL((tonemap_bw_kernel<1, __half>), dim3(rows), dim3(TM_BLOCK), 0, stream,
                               (const __half*)lograd_f16, exposure, exposure_stride, n, (const int32_t*)nullptr, params,
                               (const __half*)rgb_f16, dL_drgb, dL_dlograd, (float*)workspace);
        else
            hipLaunchKernelGGL((tonemap_bw_kernel<3, __half>), dim3(rows), dim3(TM_BLOCK), 0, stream,
                               (const __half*)lograd_f16, exposure, exposure_stride, n, (const int32_t*)nullptr, params,
                               (const __half*)rgb_f16, dL_drgb, dL_dlograd, (float*)workspace);
        const int st = mfn_check_launch("tonemap_bw");
        if (st != MFN_OK) return st;
    }
    hipLaunchKernelGGL(tonemap_bw_finish_kernel, dim3(C), dim3(TM_BLOCK), 0, stream, (const float*)workspace, rows, C,
                       grad_params);
    return mfn_check_launch("tonemap_bw (finish)");
}

// ---------------------------------------------------------------- the training step's forms
namespace {

bool check_live(const char* what, int64_t cap, const void* lograd, const float* exposure, int64_t e_stride,
                const int32_t* n_dev, const float* params) {
    if (!check_args(what, lograd, exposure, e_stride, cap, 3, params)) return false;
    if (cap > 0x7fffffff || !n_dev) {
        mfn_set_error("%s: the capacity must fit the int32 device count, which must be given", what);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int mfnerf_tonemap_fw_live(const void* lograd_f16, const float* exposure, int64_t exposure_stride,
                                      int64_t cap, const int32_t* n_dev, const float* params, float* rgb,
                                      mfnerf_stream_t stream) {
    if (!check_live("tonemap_fw_live", cap, lograd_f16, exposure, exposure_stride, n_dev, params)) return MFN_ERR_INVALID;
    if (cap == 0) return MFN_OK;
    if (!rgb) {
        mfn_set_error("tonemap_fw_live: null pointer");
        return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL((tonemap_fw_kernel<3, float>), dim3((unsigned)blocks_for(cap, TM_FW_MAX_BLOCKS)), dim3(TM_BLOCK),
                       0, stream, (const __half*)lograd_f16, exposure, exposure_stride, cap, n_dev, params, rgb);
    return mfn_check_launch("tonemap_fw_live");
}

extern "C" int mfnerf_tonemap_bw_live(const void* lograd_f16, const float* exposure, int64_t exposure_stride,
                                      int64_t cap, const int32_t* n_dev, const float* params, const float* rgb,
                                      const float* dL_drgb, float* dL_dlograd, float* grad_params, void* workspace,
                                      mfnerf_stream_t stream) {
    if (!check_live("tonemap_bw_live", cap, lograd_f16, exposure, exposure_stride, n_dev, params)) return MFN_ERR_INVALID;
    if (!grad_params || (cap > 0 && (!rgb || !dL_drgb || !dL_dlograd || !workspace))) {
        mfn_set_error("tonemap_bw_live: null pointer");
        return MFN_ERR_INVALID;
    }
    const int rows = (int)bw_rows(cap);
    if (rows > 0) {
        hipLaunchKernelGGL((tonemap_bw_kernel<3, float>), dim3(rows), dim3(TM_BLOCK), 0, stream,
                           (const __half*)lograd_f16, exposure, exposure_stride, cap, n_dev, params, rgb, dL_drgb,
                           dL_dlograd, (float*)workspace);
        const int st = mfn_check_launch("tonemap_bw_live");
        if (st != MFN_OK) return st;
    }
    hipLaunchKernelGGL(tonemap_bw_finish_kernel, dim3(3), dim3(TM_BLOCK), 0, stream, (const float*)workspace, rows, 3,
                       grad_params);
    return mfn_check_launch("tonemap_bw_live (finish)");
}

extern "C" int mfnerf_expand_exposure(const float* exposure_ray, const int64_t* rays_a, int64_t n_rays, int64_t cap,
                                      const int32_t* n_dev, float* exposure_s, mfnerf_stream_t stream) {
    if (n_rays < 0 || cap < 0 || cap > 0x7fffffff) {
        mfn_set_error("expand_exposure: bad sizes");
        return MFN_ERR_INVALID;
    }
    if (n_rays == 0 || cap == 0) return MFN_OK;
    if (!exposure_ray || !rays_a || !n_dev || !exposure_s) {
        mfn_set_error("expand_exposure: null pointer");
        return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(expand_exposure_kernel, dim3((unsigned)blocks_for(n_rays * 64, TM_FW_MAX_BLOCKS)),
                       dim3(TM_BLOCK), 0, stream, exposure_ray, rays_a, n_rays, cap, n_dev, exposure_s);
    return mfn_check_launch("expand_exposure");
}

extern "C" int mfnerf_tonemap_unit_loss(const float* params, int C, float unit_exposure_rgb, float* grad_params,
                                        float* loss_out, mfnerf_amp_state* amp, mfnerf_stream_t stream) {
    if (C != 1 && C != 3) {
        mfn_set_error("tonemap_unit_loss: C must be 1 or 3, got %d", C);
        return MFN_ERR_INVALID;
    }
    if (!params || !grad_params || !loss_out) {
        mfn_set_error("tonemap_unit_loss: null pointer");
        return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(tonemap_unit_kernel, dim3(C), dim3(TM_H), 0, stream, params, C, unit_exposure_rgb, grad_params,
                       loss_out, amp);
    return mfn_check_launch("tonemap_unit_loss");
}

extern "C" int mfnerf_side_adam_step(float* params, const float* grads, float* m, float* v, int64_t n, float lr,
                                     float beta1, float beta2, float eps, int32_t* step_dev, const float* lr_dev,
                                     const mfnerf_amp_state* amp, mfnerf_stream_t stream) {
    if (n < 0 || n > ((int64_t)1 << 20)) {
        mfn_set_error("side_adam_step: bad size %lld (one workgroup: at most 2^20 values)", (long long)n);
        return MFN_ERR_INVALID;
    }
    if (n == 0) return MFN_OK;
    if (!params || !grads || !m || !v || !step_dev) {
        mfn_set_error("side_adam_step: null pointer");
        return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(side_adam_kernel, dim3(1), dim3(SA_BLOCK), 0, stream, params, grads, m, v, n, lr, beta1, beta2,
                       eps, step_dev, lr_dev, amp);
    return mfn_check_launch("side_adam_step");
}
