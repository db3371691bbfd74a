// pose.hip -- camera-pose refinement inside the fused step (train.py:91-94, 122-139, --optimize_ext;
// datasets/ray_utils.py axisangle_to_R): the loss gradient with respect to the batch's rays reduced
// to every image's rotation / translation offsets, their Adam step and the refined poses the next
// draw reads.
//
// mfnerf_pose_grad: one 256-thread workgroup per image.  It scans the batch's image indices (a few
// tens of KB, shared by every workgroup through L2); thread t takes rays t, t + 256, ... in order and
// adds J^T dL_drays_d / dL_drays_o of the rays of its image to its own running sums; the 64 lanes fold
// by a fixed xor tree, the four waves' sums are added in wave order.  No float atomics and no
// dependence on which rays other images own: the same bits on every run, and every row is written.
//
// mfnerf_pose_step: one workgroup, a thread per image (strided): Adam on the image's six offsets, then
// its refined pose.  One workgroup, so the step counter needs no cross-workgroup ticket.
#include "common.hpp"
#include "pose_math.hpp"
#include "../../include/mfnerf.h"

using namespace mfn;
using namespace mfn_pose;

namespace {

constexpr int PG_BLOCK = 256, PG_WAVES = PG_BLOCK / 64;
constexpr int PG_UNROLL = 4;  // image indices in flight per thread before any is used

__global__ __launch_bounds__(PG_BLOCK) void pose_grad_kernel(const float* __restrict__ dL_drays_o,
                                                             const float* __restrict__ dL_drays_d,
                                                             const int32_t* __restrict__ img_idx,
                                                             const int32_t* __restrict__ pix_idx,
                                                             const float* __restrict__ poses,
                                                             const float* __restrict__ directions,
                                                             const float* __restrict__ dR, int64_t n_rays,
                                                             int64_t hw, float* __restrict__ grad_dR,
                                                             float* __restrict__ grad_dT,
                                                             mfnerf_amp_state* __restrict__ amp) {
    __shared__ float part[PG_WAVES][6];
    const int64_t img = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* c2w = poses + 12 * img;
    const Axis A = axis_of(dR + 3 * img);
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // dR | dT
    for (int64_t r0 = tid; r0 < n_rays; r0 += (int64_t)PG_BLOCK * PG_UNROLL) {
        int32_t im[PG_UNROLL];
#pragma unroll
        for (int k = 0; k < PG_UNROLL; ++k) {
            const int64_t r = r0 + (int64_t)k * PG_BLOCK;
            im[k] = r < n_rays ? img_idx[r] : -1;
        }
#pragma unroll
        for (int k = 0; k < PG_UNROLL; ++k) {
            if ((int64_t)im[k] != img) continue;
            const int64_t r = r0 + (int64_t)k * PG_BLOCK;
            const int64_t px = pix_idx[r];
            if (px < 0 || px >= hw) continue;  // a malformed pixel index reads nothing
            const float* d = directions + 3 * px;
            const float dx = d[0], dy = d[1], dz = d[2];
            float u[3], g[3], j[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                // the base pose's ray direction, as the draw forms it (data.hip)
                u[a] = fmaf(dz, c2w[4 * a + 2], fmaf(dy, c2w[4 * a + 1], dx * c2w[4 * a]));
                g[a] = dL_drays_d[3 * r + a];
            }
            jt_g(A, u, g, j);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                acc[a] += j[a];
                acc[3 + a] += dL_drays_o[3 * r + a];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) part[wave][k] = acc[k];
    __syncthreads();
    if (tid < 6) {
        float s = part[0][tid];
#pragma unroll
        for (int w = 1; w < PG_WAVES; ++w) s += part[w][tid];
        float* dst = tid < 3 ? grad_dR + 3 * img + tid : grad_dT + 3 * img + (tid - 3);
        *dst = s;
        if (amp && !isfinite(s)) atomicOr(&amp->nonfinite, 1);
    }
}

constexpr int PS_BLOCK = 256;

__global__ __launch_bounds__(PS_BLOCK) void pose_step_kernel(float* __restrict__ dR, float* __restrict__ dT,
                                                             float* __restrict__ m, float* __restrict__ v,
                                                             const float* __restrict__ grad_dR,
                                                             const float* __restrict__ grad_dT,
                                                             const float* __restrict__ poses, int64_t n_img, float lr,
                                                             float b1, float b2, float eps,
                                                             int32_t* __restrict__ step_dev,
                                                             const float* __restrict__ lr_dev,
                                                             const mfnerf_amp_state* __restrict__ amp,
                                                             float* __restrict__ poses_out) {
    // GradScaler: no update on a non-finite gradient (the field's optimizer pass does the bookkeeping)
    const bool update = grad_dR && !(amp && amp->nonfinite != 0);
    const int st = update ? *step_dev + 1 : 0;
    if (lr_dev) lr = *lr_dev;
    // 1 - beta^t in double: in fp32 the difference keeps ~1e-5 relative at small t for beta2 = 0.999
    const float bc1 = update ? (float)(1.0 - pow((double)b1, (double)st)) : 1.0f;
    const float bc2 = update ? (float)(1.0 - pow((double)b2, (double)st)) : 1.0f;
    for (int64_t i = threadIdx.x; i < n_img; i += PS_BLOCK) {
        float w[3], t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { w[k] = dR[3 * i + k]; t[k] = dT[3 * i + k]; }
        if (update) {
            float* mR = m + 3 * i; float* vR = v + 3 * i;
            float* mT = m + 3 * (n_img + i); float* vT = v + 3 * (n_img + i);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float mm = mR[k], vv = vR[k];
                adam_elem(w[k], mm, vv, grad_dR[3 * i + k], b1, b2, eps, lr, bc1, bc2);
                mR[k] = mm; vR[k] = vv; dR[3 * i + k] = w[k];
                mm = mT[k]; vv = vT[k];
                adam_elem(t[k], mm, vv, grad_dT[3 * i + k], b1, b2, eps, lr, bc1, bc2);
                mT[k] = mm; vT[k] = vv; dT[3 * i + k] = t[k];
            }
        }
        // [R(dR) @ R0 | t0 + dT]
        float R[9];
        rotation(axis_of(w), R);
        const float* c2w = poses + 12 * i;
        float* out = poses_out + 12 * i;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                out[4 * a + c] = fmaf(R[3 * a + 2], c2w[8 + c], fmaf(R[3 * a + 1], c2w[4 + c], R[3 * a] * c2w[c]));
            out[4 * a + 3] = c2w[4 * a + 3] + t[a];
        }
    }
    if (update) {
        // every thread has read *step_dev above
        __syncthreads();
        if (threadIdx.x == 0) *step_dev = st;
    }
}

}  // namespace

extern "C" int mfnerf_pose_grad(const float* dL_drays_o, const float* dL_drays_d, const int32_t* img_idx,
                                const int32_t* pix_idx, const float* poses, const float* directions,
                                const float* dR, int64_t n_rays, int64_t n_img, int64_t hw, float* grad_dR,
                                float* grad_dT, mfnerf_amp_state* amp, mfnerf_stream_t stream) {
    if (n_rays < 0 || n_img < 0 || hw <= 0 || n_img > 0x7fffffff || hw > 0x7fffffff) {
        mfn_set_error("pose_grad: bad sizes");
        return MFN_ERR_INVALID;
    }
    if (n_img == 0) return MFN_OK;
    if (!poses || !directions || !dR || !grad_dR || !grad_dT ||
        (n_rays > 0 && (!dL_drays_o || !dL_drays_d || !img_idx || !pix_idx))) {
        mfn_set_error("pose_grad: null pointer");
        return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(pose_grad_kernel, dim3((unsigned)n_img), dim3(PG_BLOCK), 0, stream, dL_drays_o, dL_drays_d,
                       img_idx, pix_idx, poses, directions, dR, n_rays, hw, grad_dR, grad_dT, amp);
    return mfn_check_launch("pose_grad");
}

extern "C" int mfnerf_pose_step(float* dR, float* dT, float* m, float* v, const float* grad_dR, const float* grad_dT,
                                const float* poses, int64_t n_img, float lr, float beta1, float beta2, float eps,
                                int32_t* step_dev, const float* lr_dev, const mfnerf_amp_state* amp, float* poses_out,
                                mfnerf_stream_t stream) {
    if (n_img < 0) { mfn_set_error("pose_step: bad size"); return MFN_ERR_INVALID; }
    if (n_img == 0) return MFN_OK;
    if (!dR || !dT || !poses || !poses_out) { mfn_set_error("pose_step: null pointer"); return MFN_ERR_INVALID; }
    if ((grad_dR == nullptr) != (grad_dT == nullptr)) {
        mfn_set_error("pose_step: grad_dR and grad_dT go together"); return MFN_ERR_INVALID;
    }
    if (grad_dR && (!m || !v || !step_dev)) { mfn_set_error("pose_step: null optimizer state"); return MFN_ERR_INVALID; }
    if (poses_out == poses) { mfn_set_error("pose_step: poses_out must not be the base poses"); return MFN_ERR_INVALID; }
    hipLaunchKernelGGL(pose_step_kernel, dim3(1), dim3(PS_BLOCK), 0, stream, dR, dT, m, v, grad_dR, grad_dT, poses, n_img,
                       lr, beta1, beta2, eps, step_dev, lr_dev, amp, poses_out);
    return mfn_check_launch("pose_step");
}
