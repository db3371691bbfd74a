// metrics.hip -- the reference's validation metrics of one test view on the device (train.py:65-67,
// 198-237: torchmetrics PeakSignalNoiseRatio(data_range=1) and StructuralSimilarityIndexMeasure(
// data_range=1), logged as test/psnr and test/ssim): the mean squared error and the SSIM of two
// (H*W, 3) fp32 images, accumulated in fp64.
//
// SSIM is the mean over the pixels whose 11x11 Gaussian window (sigma 1.5) lies inside the image --
// what torchmetrics keeps after it pads by reflection and crops the padded border again -- of
//     s = ((2 mp mt + c1)(2 spt + c2)) / ((mp^2 + mt^2 + c1)(sp2 + st2 + c2)),
// mp, mt the filtered means, sp2 = E[p^2] - mp^2, st2, spt = E[pt] - mp mt.  Those differences cancel
// in fp32 on near-flat bright windows (white backgrounds), so every product, filter sum, the
// expression and both reductions are fp64 here; the inputs stay fp32 in LDS and are widened as read.
//
// The three interleaved channels make the image a (H, 3W) plane whose horizontal taps are 3 apart,
// so one workgroup filters all channels of its tile at once:
//   1. the MT_TH x MT_TW output tile's (MT_TH+10) x (MT_TW+10) pixel halo of both images -> LDS
//      (a halo row is (MT_TW+10)*3 contiguous floats; rows or columns past the image read 0 and feed
//      only outputs that are masked);
//   2. the squared error of the image pixels this tile owns (the image is cut along the tile seams,
//      the border going to the outer tiles: every pixel belongs to exactly one tile);
//   3. horizontal pass: the five moments of every halo row at the tile's MT_TW*3 columns -> LDS (fp64);
//   4. vertical pass + the SSIM expression, masked to the image's valid outputs;
//   5. a fixed-order fold (lanes by xor tree, waves in order) -> one {sse, ssim_sum} pair per tile,
//      plain stores; a second one-workgroup launch sums the pairs in a fixed order and divides.
// No atomics, no ticket, nothing to zero: two runs give the same bits and the workspace may hold
// anything on entry.
//
// LDS banking sets the tile.  The moments are read and written 8 bytes a lane (ds_read_b64: 32-lane
// groups over 64 four-byte banks; ds_write_b64: 16-lane groups over 32), work items run along a row
// and on into the next, and a row of MT_TW*3 = 48 doubles is 16 mod 32: a 32-lane group that ends
// one row at columns 32..47 and starts the next at 0..15 lands on the two halves of the bank row, so
// every group is conflict-free without padding.  The fp32 input rows are padded from 78 to 80 floats
// (16 mod 32 again) for the same straddle under ds_read_b32.  16 x 16 keeps the workgroup at 65 KiB
// of LDS, two workgroups a CU.
#include <math.h>

#include "common.hpp"
#include "../../include/mfnerf.h"

namespace {

constexpr int MT_TH = 16, MT_TW = 16;      // output tile, pixels
constexpr int MT_R = 5, MT_TAPS = 2 * MT_R + 1;
constexpr int MT_HH = MT_TH + 2 * MT_R;    // halo rows
constexpr int MT_HC = (MT_TW + 2 * MT_R) * 3;  // halo row, floats
constexpr int MT_IN_STRIDE = 80;           // halo row in LDS, floats
constexpr int MT_XC = MT_TW * 3;           // output columns of the (H, 3W) plane
constexpr int MT_BLOCK = 256, MT_WAVES = MT_BLOCK / 64;
constexpr int MT_MOMENTS = 5;              // mp, mt, E[p^2], E[t^2], E[pt]

// mfnerf/metrics.py publishes the tile (TILE_H, TILE_W): the tests place their shapes around it
static_assert(MT_TH == 16 && MT_TW == 16, "keep mfnerf/metrics.py TILE_H / TILE_W equal to MT_TH / MT_TW");
static_assert(MT_IN_STRIDE >= MT_HC && MT_IN_STRIDE % 32 == 16, "input rows: 16 mod 32 floats");
static_assert(MT_XC % 32 == 16, "moment rows: 16 mod 32 doubles");
static_assert((MT_TH * MT_XC) % MT_BLOCK == 0, "the vertical pass gives every thread the same item count");

struct Weights { double g[MT_R + 1]; };  // g[d] = the tap at distance d from the centre

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(MT_BLOCK) void image_metrics_tile_kernel(const float* __restrict__ pred,
                                                                      const float* __restrict__ target, int H, int W,
                                                                      int tiles_x, Weights wt,
                                                                      double* __restrict__ partials) {
    __shared__ float in_p[MT_HH * MT_IN_STRIDE];
    __shared__ float in_t[MT_HH * MT_IN_STRIDE];
    __shared__ double mid[MT_MOMENTS][MT_HH * MT_XC];
    __shared__ double fold[MT_WAVES][2];
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x % tiles_x;
    const int y0 = ty * MT_TH, x0 = tx * MT_TW;  // the halo's first image row / column
    const int tiles_y = (int)gridDim.x / tiles_x;

    // 1. halo -> LDS
    const int cols_in = min(MT_HC, (W - x0) * 3);  // floats of a halo row inside the image
    for (int e = tid; e < MT_HH * MT_HC; e += MT_BLOCK) {
        const int r = e / MT_HC, c = e % MT_HC;
        float p = 0.0f, t = 0.0f;
        if (y0 + r < H && c < cols_in) {
            const int64_t at = ((int64_t)(y0 + r) * W + x0) * 3 + c;
            p = pred[at];
            t = target[at];
        }
        in_p[r * MT_IN_STRIDE + c] = p;
        in_t[r * MT_IN_STRIDE + c] = t;
    }
    __syncthreads();

    // 2. squared error of the pixels this tile owns, halo-local rows [ya, yb) x floats [ca, cb)
    const int ya = ty == 0 ? 0 : MT_R, yb = ty == tiles_y - 1 ? H - y0 : MT_R + MT_TH;
    const int ca = tx == 0 ? 0 : MT_R * 3, cb = tx == tiles_x - 1 ? (W - x0) * 3 : (MT_R + MT_TW) * 3;
    double sse = 0.0;
    for (int e = tid; e < MT_HH * MT_HC; e += MT_BLOCK) {
        const int r = e / MT_HC, c = e % MT_HC;
        if (r >= ya && r < yb && c >= ca && c < cb) {
            const double d = (double)in_p[r * MT_IN_STRIDE + c] - (double)in_t[r * MT_IN_STRIDE + c];
            sse += d * d;
        }
    }

    // 3. horizontal pass: the same operation order for E[p^2], E[t^2] and E[pt]
    for (int e = tid; e < MT_HH * MT_XC; e += MT_BLOCK) {
        const int r = e / MT_XC, j = e % MT_XC;
        const float* rp = in_p + r * MT_IN_STRIDE + j;
        const float* rt = in_t + r * MT_IN_STRIDE + j;
        double mp = 0.0, mt = 0.0, pp = 0.0, tt = 0.0, pt = 0.0;
#pragma unroll
        for (int k = 0; k < MT_TAPS; ++k) {
            const double g = wt.g[k < MT_R ? MT_R - k : k - MT_R];
            const double p = (double)rp[3 * k], t = (double)rt[3 * k];
            mp = fma(g, p, mp);
            mt = fma(g, t, mt);
            pp = fma(g, p * p, pp);
            tt = fma(g, t * t, tt);
            pt = fma(g, p * t, pt);
        }
        mid[0][e] = mp;
        mid[1][e] = mt;
        mid[2][e] = pp;
        mid[3][e] = tt;
        mid[4][e] = pt;
    }
    __syncthreads();

    // 4. vertical pass and the SSIM expression
    const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
    const int out_h = H - 2 * MT_R, out_w = W - 2 * MT_R;
    double ssim = 0.0;
#pragma unroll
    for (int it = 0; it < MT_TH * MT_XC / MT_BLOCK; ++it) {
        const int e = tid + it * MT_BLOCK;
        const int y = e / MT_XC, j = e % MT_XC;
        double m[MT_MOMENTS];
#pragma unroll
        for (int q = 0; q < MT_MOMENTS; ++q) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < MT_TAPS; ++k)
                a = fma(wt.g[k < MT_R ? MT_R - k : k - MT_R], mid[q][(y + k) * MT_XC + j], a);
            m[q] = a;
        }
        const double mp = m[0], mt = m[1];
        const double sp2 = m[2] - mp * mp, st2 = m[3] - mt * mt, spt = m[4] - mp * mt;
        const double num = (2.0 * (mp * mt) + c1) * (2.0 * spt + c2);
        const double den = ((mp * mp + mt * mt) + c1) * ((sp2 + st2) + c2);
        if (y0 + y < out_h && x0 + j / 3 < out_w) ssim += num / den;
    }

    // 5. fixed-order fold -> this tile's pair
    sse = wave_sum(sse);
    ssim = wave_sum(ssim);
    if ((tid & 63) == 0) {
        fold[tid >> 6][0] = sse;
        fold[tid >> 6][1] = ssim;
    }
    __syncthreads();
    if (tid < 2) {
        double s = fold[0][tid];
#pragma unroll
        for (int w = 1; w < MT_WAVES; ++w) s += fold[w][tid];
        partials[2 * (int64_t)blockIdx.x + tid] = s;
    }
}

// The tiles' pairs summed in a fixed order: thread t adds tiles t, t + 256, ... in order, then the
// same fold as above.  out = {sse / (3 H W), ssim_sum / (3 (H-10) (W-10))}.
__global__ __launch_bounds__(MT_BLOCK) void image_metrics_finish_kernel(const double* __restrict__ partials,
                                                                        int64_t n_tiles, double n_mse, double n_ssim,
                                                                        double* __restrict__ out) {
    __shared__ double fold[MT_WAVES][2];
    const int tid = threadIdx.x;
    double sse = 0.0, ssim = 0.0;
    for (int64_t i = tid; i < n_tiles; i += MT_BLOCK) {
        sse += partials[2 * i];
        ssim += partials[2 * i + 1];
    }
    sse = wave_sum(sse);
    ssim = wave_sum(ssim);
    if ((tid & 63) == 0) {
        fold[tid >> 6][0] = sse;
        fold[tid >> 6][1] = ssim;
    }
    __syncthreads();
    if (tid < 2) {
        double s = fold[0][tid];
#pragma unroll
        for (int w = 1; w < MT_WAVES; ++w) s += fold[w][tid];
        out[tid] = s / (tid == 0 ? n_mse : n_ssim);
    }
}

constexpr int64_t MT_MAX_SIDE = 1 << 20;  // 3*H*W and the tile count stay far inside int64 / a 1-D grid

bool tiles_of(int64_t H, int64_t W, int64_t* tiles_y, int64_t* tiles_x) {
    if (H < MT_TAPS || W < MT_TAPS || H > MT_MAX_SIDE || W > MT_MAX_SIDE) return false;
    *tiles_y = (H - 2 * MT_R + MT_TH - 1) / MT_TH;
    *tiles_x = (W - 2 * MT_R + MT_TW - 1) / MT_TW;
    return *tiles_y * *tiles_x <= 0x7fffffff;
}

// g[k] ~ exp(-(k-5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1; by distance from the centre
Weights gaussian_weights() {
    double e[MT_TAPS], sum = 0.0;
    for (int k = 0; k < MT_TAPS; ++k) {
        const double d = (double)(k - MT_R);
        e[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += e[k];
    }
    Weights w;
    for (int d = 0; d <= MT_R; ++d) w.g[d] = e[MT_R + d] / sum;
    return w;
}

}  // namespace

extern "C" int64_t mfnerf_image_metrics_workspace(int64_t H, int64_t W) {
    int64_t tiles_y, tiles_x;
    if (!tiles_of(H, W, &tiles_y, &tiles_x)) return 0;
    return tiles_y * tiles_x * 2 * (int64_t)sizeof(double);
}

extern "C" int mfnerf_image_metrics(const float* pred, const float* target, int64_t H, int64_t W, double* out,
                                    void* workspace, mfnerf_stream_t stream) {
    if (H < MT_TAPS || W < MT_TAPS) {
        mfn_set_error("image_metrics: H and W must be at least %d (the SSIM window), got %lld x %lld", MT_TAPS,
                      (long long)H, (long long)W);
        return MFN_ERR_INVALID;
    }
    int64_t tiles_y, tiles_x;
    if (!tiles_of(H, W, &tiles_y, &tiles_x)) {
        mfn_set_error("image_metrics: image too large (%lld x %lld)", (long long)H, (long long)W);
        return MFN_ERR_INVALID;
    }
    if (!pred || !target || !out || !workspace) {
        mfn_set_error("image_metrics: null pointer");
        return MFN_ERR_INVALID;
    }
    static const Weights wt = gaussian_weights();
    const int64_t n_tiles = tiles_y * tiles_x;
    hipLaunchKernelGGL(image_metrics_tile_kernel, dim3((unsigned)n_tiles), dim3(MT_BLOCK), 0, stream, pred, target,
                       (int)H, (int)W, (int)tiles_x, wt, (double*)workspace);
    const int st = mfn_check_launch("image_metrics (tiles)");
    if (st != MFN_OK) return st;
    hipLaunchKernelGGL(image_metrics_finish_kernel, dim3(1), dim3(MT_BLOCK), 0, stream, (const double*)workspace,
                       n_tiles, 3.0 * (double)H * (double)W, 3.0 * (double)(H - 2 * MT_R) * (double)(W - 2 * MT_R), out);
    return mfn_check_launch("image_metrics (finish)");
}
