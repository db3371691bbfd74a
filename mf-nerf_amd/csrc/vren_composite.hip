// vren_composite.hip -- compositing (volumerendering.cu) and the losses computed from its outputs
// (losses.cu, losses.py), with their C-ABI entry points.  Training compositing writes every sample of
// every ray exactly once (zeros after termination), so no n_samples-sized memsets are needed; the
// backward's per-ray scan runs in registers.
#include "composite_sample.hpp"
#include "wave_ops.hpp"
#include "vren_launch.hpp"

using namespace mfn;
using namespace mfn_vren;

namespace {

// ---- wave-per-ray compositing (volumerendering.cu:6-45 / :87-151).  One wave per ray, lanes =
// samples (coalesced loads/stores, 64 samples per chunk).  The transmittance chain T *= 1-a is
// evaluated in the reference's sequential order by a uniform loop over the lanes (bit-identical
// T, hence identical termination and total_samples); the rgb/depth/opacity sums and the backward's
// prefix sums are wave reductions/scans (wave_ops.hpp; fp32 reassociation only, ~1e-7 relative).

// Sequential T over the chunk: returns this lane's T before its sample; T_run is advanced; *stop is
// the first lane whose post-update T <= thr (64 if none).  The reference's order is kept exactly:
// T_j = fl(T_{j-1} * fl(1 - a_{j-1})), so T, termination and total_samples are bit-identical to its
// sequential loop.  The chain is propagated one lane per step with a whole-wave DPP shift
// (wave_shr:1): after k steps lanes 0..k hold their final T, so n_valid-1 steps of one shifted
// multiply replace n_valid serial readlane/multiply/compare/branch rounds -- the long rays' chains
// (hundreds of samples) were this kernel's critical path.
__device__ __forceinline__ float t_chain(float a, float& T_run, float thr, int lane, int n_valid, int* stop) {
    constexpr int WAVE_SHR1 = 0x138;
    const float b = 1.0f - a;  // lanes past n_valid: a = 0, b = 1
    // bs[j] = b[j-1], bs[0] = 1 (T_0 = T_run * 1 exactly)
    const float bs = __int_as_float(
        __builtin_amdgcn_update_dpp(__float_as_int(1.0f), __float_as_int(b), WAVE_SHR1, 0xF, 0xF, false));
    const int t0 = __float_as_int(T_run);
    float X = T_run;
    const int nv = __builtin_amdgcn_readfirstlane(n_valid);  // wave-uniform: a scalar loop
    for (int k = 1; k < nv; ++k)
        X = __int_as_float(__builtin_amdgcn_update_dpp(t0, __float_as_int(X), WAVE_SHR1, 0xF, 0xF, false)) * bs;
    const float Ta = X * b;  // T after this lane's sample
    const uint64_t hit = __ballot(lane < n_valid && Ta <= thr);
    const int st = hit ? (int)__builtin_ctzll(hit) : 64;
    T_run = readlane_f(Ta, st < 64 ? st : n_valid - 1);
    *stop = st;
    return X;
}

__global__ __launch_bounds__(256) void composite_fw_wave_kernel(
    const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
    const float* __restrict__ ts, const int64_t* __restrict__ rays_a, int64_t n_rays, float T_thr,
    int64_t* __restrict__ total_samples, float* __restrict__ opacity, float* __restrict__ depth,
    float* __restrict__ rgb, float* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (n >= n_rays) return;
    const int64_t ray = rays_a[3 * n], start = rays_a[3 * n + 1];
    const int N = (int)rays_a[3 * n + 2];
    float T = 1.0f, R = 0.f, G = 0.f, B = 0.f, D = 0.f, O = 0.f;
    int total = N;
    bool ended = false;
    for (int k0 = 0; k0 < N; k0 += 64) {
        const int nv = min(64, N - k0);
        const int64_t s = start + k0 + lane;
        const bool valid = lane < nv;
        float w = 0.0f;
        if (!ended) {
            const float a = valid ? 1.0f - fast_exp(-sigmas[s] * deltas[s]) : 0.0f;
            int stop;
            const float myT = t_chain(a, T, T_thr, lane, nv, &stop);
            if (valid && lane <= stop) {
                w = a * myT;
                R = fmaf(w, rgbs[3 * s], R); G = fmaf(w, rgbs[3 * s + 1], G); B = fmaf(w, rgbs[3 * s + 2], B);
                D = fmaf(w, ts[s], D);
                O += w;
            }
            if (stop < 64) { ended = true; total = k0 + stop; }
        }
        if (valid) ws[s] = w;
    }
    R = wave_sum(R); G = wave_sum(G); B = wave_sum(B); D = wave_sum(D); O = wave_sum(O);
    if (lane == 0) {
        opacity[ray] = O; depth[ray] = D;
        rgb[3 * ray] = R; rgb[3 * ray + 1] = G; rgb[3 * ray + 2] = B;
        total_samples[ray] = total;
    }
}

__global__ __launch_bounds__(256) void composite_bw_wave_kernel(
    const float* __restrict__ dL_dopacity, const float* __restrict__ dL_ddepth, const float* __restrict__ dL_drgb,
    const float* __restrict__ dL_dws, const float* __restrict__ sigmas, const float* __restrict__ rgbs,
    const float* __restrict__ ws, const float* __restrict__ deltas, const float* __restrict__ ts,
    const int64_t* __restrict__ rays_a, const float* __restrict__ opacity, const float* __restrict__ depth,
    const float* __restrict__ rgb, int64_t n_rays, float T_thr, float* __restrict__ dL_dsigmas,
    float* __restrict__ dL_drgbs) {
    const int lane = threadIdx.x & 63;
    const int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (n >= n_rays) return;
    const int64_t ray = rays_a[3 * n], start = rays_a[3 * n + 1];
    const int N = (int)rays_a[3 * n + 2];
    if (N <= 0) return;
    // total of dL_dws*ws over the whole ray (the inclusive scan's last element)
    float wsum = 0.0f;
    for (int k0 = 0; k0 < N; k0 += 64) {
        const int64_t s = start + k0 + lane;
        if (k0 + lane < N) wsum += dL_dws[s] * ws[s];
    }
    wsum = wave_sum(wsum);
    const float Rt = rgb[3 * ray], Gt = rgb[3 * ray + 1], Bt = rgb[3 * ray + 2];
    const float O = opacity[ray], Dt = depth[ray];
    const float gr = dL_drgb[3 * ray], gg = dL_drgb[3 * ray + 1], gb = dL_drgb[3 * ray + 2];
    const float go = dL_dopacity[ray], gd = dL_ddepth[ray];
    float T = 1.0f, cr = 0.f, cg = 0.f, cb = 0.f, cd = 0.f, cs = 0.f;  // carries of the prefix sums
    bool ended = false;
    for (int k0 = 0; k0 < N; k0 += 64) {
        const int nv = min(64, N - k0);
        const int64_t s = start + k0 + lane;
        const bool valid = lane < nv;
        float dsig = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
        if (!ended) {
            float sg = 0.f, dl = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, tv = 0.f, dw = 0.f, wv = 0.f;
            if (valid) {
                sg = sigmas[s]; dl = deltas[s]; tv = ts[s]; dw = dL_dws[s]; wv = ws[s];
                c0 = rgbs[3 * s]; c1 = rgbs[3 * s + 1]; c2 = rgbs[3 * s + 2];
            }
            const float a = valid ? 1.0f - fast_exp(-sg * dl) : 0.0f;
            int stop;
            const float myT = t_chain(a, T, T_thr, lane, nv, &stop);
            const bool act = valid && lane <= stop;
            const float w = act ? a * myT : 0.0f;
            const float Tn = myT * (1.0f - a);  // T after this sample (the reference's updated T)
            const float pr = wave_incl_scan(w * c0) + cr, pg = wave_incl_scan(w * c1) + cg;
            const float pb = wave_incl_scan(w * c2) + cb, pd = wave_incl_scan(w * tv) + cd;
            const float ps = wave_incl_scan(act ? dw * wv : 0.0f) + cs;
            cr = readlane_f(pr, 63); cg = readlane_f(pg, 63); cb = readlane_f(pb, 63); cd = readlane_f(pd, 63);
            cs = readlane_f(ps, 63);
            if (act) {
                d0 = gr * w; d1 = gg * w; d2 = gb * w;
                float acc = gr * fmaf(c0, Tn, -(Rt - pr));
                acc = fmaf(gg, fmaf(c1, Tn, -(Gt - pg)), acc);
                acc = fmaf(gb, fmaf(c2, Tn, -(Bt - pb)), acc);
                acc = fmaf(go, 1 - O, acc);
                acc = fmaf(gd, fmaf(tv, Tn, -(Dt - pd)), acc);
                acc = fmaf(Tn, dw, acc);
                acc = acc - (wsum - ps);
                dsig = dl * acc;
            }
            if (stop < 64) ended = true;
        }
        if (valid) {
            dL_dsigmas[s] = dsig;
            dL_drgbs[3 * s] = d0; dL_drgbs[3 * s + 1] = d1; dL_drgbs[3 * s + 2] = d2;
        }
    }
}

// The loss's background colour (rendering.py:153-161) as the loss-carrying kernels take it: three
// kernel arguments (a fixed colour: white on synthetic scenes, black on real ones), or three floats in
// device memory (--random_bg: the colour is drawn on the device for each batch, and a captured graph
// freezes its scalar arguments).  A template parameter of the kernels chooses at compile time:
// DEV_BG = false keeps the parameter list (float, float, float) and so, instruction for instruction, the
// code the kernels had before the option existed (a struct of three floats, or the body behind a thin
// kernel, each reordered it); DEV_BG = true takes (const float*, -, -) and reads the three values once,
// before any sample.  Both feed the same arithmetic in the same order.
struct BgUnused {};
template <bool DEV_BG> struct BgParam { using first = float; using rest = float; };
template <> struct BgParam<true> { using first = const float*; using rest = BgUnused; };
template <bool DEV_BG>
__device__ __forceinline__ void bg_fetch(typename BgParam<DEV_BG>::first a0, typename BgParam<DEV_BG>::rest a1,
                                         typename BgParam<DEV_BG>::rest a2, float& b0, float& b1, float& b2) {
    if constexpr (DEV_BG) { b0 = a0[0]; b1 = a0[1]; b2 = a0[2]; }
    else { b0 = a0; b1 = a1; b2 = a2; }
}

// Fused training compositing for the default loss (no distortion term): composite_train_fw ->
// background blend + NeRFLoss and its gradient -> composite_train_bw with dL/ddepth = 0 and
// dL/dws = 0, one wave per ray, one launch.  Pass 1 is composite_fw_wave_kernel's loop and also
// stores each sample's post-sample transmittance into dL_dsigmas (as scratch); pass 2 reads w and
// T back (same lane, same address) instead of re-walking the transmittance chain, so the result is
// bit-identical to the three separate kernels (the dropped terms are exact zeros).  The loss value
// is written as one partial sum per workgroup of 4 rays (plain stores: no zeroing, no atomics).
// DEV_BG: the background colour is three floats in device memory, read once per ray before pass 1.
template <bool DEV_BG>
__global__ __launch_bounds__(256) void composite_fused_wave_kernel(
    const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ deltas,
    const float* __restrict__ ts, const int64_t* __restrict__ rays_a, int64_t n_rays, float T_thr,
    const float* __restrict__ target, int64_t n_mean, float lambda_o, typename BgParam<DEV_BG>::first bg0,
    typename BgParam<DEV_BG>::rest bg1, typename BgParam<DEV_BG>::rest bg2,
    int64_t* __restrict__ total_samples, float* __restrict__ opacity, float* __restrict__ depth,
    float* __restrict__ rgb, float* __restrict__ ws, float* __restrict__ dL_drgb, float* __restrict__ dL_dop,
    float* __restrict__ dL_dsigmas, float* __restrict__ dL_drgbs, float* __restrict__ loss_part) {
    __shared__ float lsum[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    float l = 0.0f;
    if (n < n_rays) {
        const int64_t ray = rays_a[3 * n], start = rays_a[3 * n + 1];
        const int N = (int)rays_a[3 * n + 2];
        const float tg[3] = {target[3 * ray], target[3 * ray + 1], target[3 * ray + 2]};
        float b0, b1, b2;
        bg_fetch<DEV_BG>(bg0, bg1, bg2, b0, b1, b2);
        // ---- pass 1: forward (composite_fw_wave_kernel)
        float T = 1.0f, R = 0.f, G = 0.f, B = 0.f, D = 0.f, O = 0.f;
        int total = N;
        bool ended = false;
        for (int k0 = 0; k0 < N; k0 += 64) {
            const int nv = min(64, N - k0);
            const int64_t s = start + k0 + lane;
            const bool valid = lane < nv;
            float w = 0.0f, tn = 0.0f;
            if (!ended) {
                // the chunk's loads are all issued before the serial chain, which hides them
                float sg = 0.f, dl = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, tv = 0.f;
                if (valid) {
                    sg = sigmas[s]; dl = deltas[s]; tv = ts[s];
                    c0 = rgbs[3 * s]; c1 = rgbs[3 * s + 1]; c2 = rgbs[3 * s + 2];
                }
                const float a = valid ? 1.0f - fast_exp(-sg * dl) : 0.0f;
                int stop;
                const float myT = t_chain(a, T, T_thr, lane, nv, &stop);
                if (valid && lane <= stop) {
                    w = a * myT;
                    tn = myT * (1.0f - a);
                    R = fmaf(w, c0, R); G = fmaf(w, c1, G); B = fmaf(w, c2, B);
                    D = fmaf(w, tv, D);
                    O += w;
                }
                if (stop < 64) { ended = true; total = k0 + stop; }
            }
            if (valid) { ws[s] = w; dL_dsigmas[s] = tn; }
        }
        R = wave_sum(R); G = wave_sum(G); B = wave_sum(B); D = wave_sum(D); O = wave_sum(O);
        // ---- loss (nerf_loss_kernel, same expression order), wave-uniform
        const float inv3n = 1.0f / (3.0f * (float)n_mean), invn = 1.0f / (float)n_mean;
        const float bg[3] = {b0, b1, b2}, col[3] = {R, G, B};
        float gcol[3], dop = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float e = col[c] + bg[c] * (1.0f - O) - tg[c];
            l += e * e * inv3n;
            gcol[c] = 2.0f * e * inv3n;
            dop -= bg[c] * gcol[c];
        }
        const float o = O + 1e-10f;
        l += lambda_o * (-o * logf(o)) * invn;
        const float go = dop + lambda_o * (-(logf(o) + 1.0f)) * invn;
        if (lane == 0) {
            opacity[ray] = O; depth[ray] = D;
            rgb[3 * ray] = R; rgb[3 * ray + 1] = G; rgb[3 * ray + 2] = B;
            total_samples[ray] = total;
            dL_drgb[3 * ray] = gcol[0]; dL_drgb[3 * ray + 1] = gcol[1]; dL_drgb[3 * ray + 2] = gcol[2];
            dL_dop[ray] = go;
        }
        // ---- pass 2: backward (composite_bw_wave_kernel with dL_ddepth = dL_dws = 0)
        const int last = ended ? total : N - 1;  // the last accumulated sample
        const float gr = gcol[0], gg = gcol[1], gb = gcol[2];
        float cr = 0.f, cg = 0.f, cb = 0.f;
        for (int k0 = 0; k0 < N; k0 += 64) {
            const int64_t s = start + k0 + lane;
            const bool valid = k0 + lane < N;
            const bool act = k0 + lane <= last;
            if (k0 > last) {  // after termination: zero gradients
                if (valid) {
                    dL_dsigmas[s] = 0.0f;
                    dL_drgbs[3 * s] = 0.0f; dL_drgbs[3 * s + 1] = 0.0f; dL_drgbs[3 * s + 2] = 0.0f;
                }
                continue;
            }
            float w = 0.f, tn = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dl = 0.f;
            if (act) {
                w = ws[s]; tn = dL_dsigmas[s]; dl = deltas[s];
                c0 = rgbs[3 * s]; c1 = rgbs[3 * s + 1]; c2 = rgbs[3 * s + 2];
            }
            const float pr = wave_incl_scan(w * c0) + cr, pg = wave_incl_scan(w * c1) + cg;
            const float pb = wave_incl_scan(w * c2) + cb;
            cr = readlane_f(pr, 63); cg = readlane_f(pg, 63); cb = readlane_f(pb, 63);
            float dsig = 0.0f, d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
            if (act) {
                d0 = gr * w; d1 = gg * w; d2 = gb * w;
                float acc = gr * fmaf(c0, tn, -(R - pr));
                acc = fmaf(gg, fmaf(c1, tn, -(G - pg)), acc);
                acc = fmaf(gb, fmaf(c2, tn, -(B - pb)), acc);
                acc = fmaf(go, 1 - O, acc);
                dsig = dl * acc;
            }
            if (valid) {
                dL_dsigmas[s] = dsig;
                dL_drgbs[3 * s] = d0; dL_drgbs[3 * s + 1] = d1; dL_drgbs[3 * s + 2] = d2;
            }
        }
    }
    if (lane == 0) lsum[wid] = l;
    __syncthreads();
    if (threadIdx.x == 0 && loss_part) loss_part[blockIdx.x] = (lsum[0] + lsum[1]) + (lsum[2] + lsum[3]);
}

__global__ void composite_test_kernel(const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                      const float* __restrict__ deltas, const float* __restrict__ ts,
                                      int64_t* __restrict__ alive, int64_t n_alive, int N_samples, float T_thr,
                                      const int32_t* __restrict__ n_eff, float* __restrict__ opacity,
                                      float* __restrict__ depth, float* __restrict__ rgb) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int ne = n_eff[n];
    if (ne == 0) { alive[n] = -1; return; }
    const int64_t r = alive[n];
    RaySums S;
    S.O = opacity[r]; S.D = depth[r]; S.R = rgb[3 * r]; S.G = rgb[3 * r + 1]; S.B = rgb[3 * r + 2];
    S.T = 1 - S.O;
    for (int s = 0; s < ne; ++s) {
        const int64_t k = n * N_samples + s;
        // (loaded in the order the reference's statements read them: the load order is part of the code)
        const float sg = sigmas[k], dl = deltas[k];
        const float c0 = rgbs[3 * k], c1 = rgbs[3 * k + 1], c2 = rgbs[3 * k + 2];
        const float tv = ts[k];
        if (composite_sample(S, sg, dl, tv, c0, c1, c2, T_thr)) { alive[n] = -1; break; }
    }
    opacity[r] = S.O; depth[r] = S.D; rgb[3 * r] = S.R; rgb[3 * r + 1] = S.G; rgb[3 * r + 2] = S.B;
}

// ------------------------------------------------------------------ distortion loss (losses.cu)
__global__ void distortion_fw_kernel(const float* __restrict__ ws, const float* __restrict__ deltas,
                                     const float* __restrict__ ts, const int64_t* __restrict__ rays_a,
                                     int64_t n_rays, float* __restrict__ loss, float* __restrict__ ws_incl,
                                     float* __restrict__ wts_incl) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rays) return;
    const int64_t ray = rays_a[3 * n], start = rays_a[3 * n + 1];
    const int N = (int)rays_a[3 * n + 2];
    const float third = 1.0f / 3;
    float a = 0.f, b = 0.f, sum = 0.f;
    for (int k = 0; k < N; ++k) {
        const int64_t s = start + k;
        const float wx = a, wtx = b;
        a += ws[s]; b += ws[s] * ts[s];
        ws_incl[s] = a; wts_incl[s] = b;
        sum += 2 * (b * wx - a * wtx) + third * ws[s] * ws[s] * deltas[s];
    }
    loss[ray] = sum;
}

__global__ void distortion_bw_kernel(const float* __restrict__ dL_dloss, const float* __restrict__ ws_incl,
                                     const float* __restrict__ wts_incl, const float* __restrict__ ws,
                                     const float* __restrict__ deltas, const float* __restrict__ ts,
                                     const int64_t* __restrict__ rays_a, int64_t n_rays, float* __restrict__ dL_dws) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rays) return;
    const int64_t ray = rays_a[3 * n], start = rays_a[3 * n + 1];
    const int N = (int)rays_a[3 * n + 2];
    if (N <= 0) return;
    const int64_t end = start + N - 1;
    const float ws_sum = ws_incl[end], wts_sum = wts_incl[end], g = dL_dloss[ray];
    for (int64_t s = start; s <= end; ++s) {
        const float first = (s == start) ? 0.0f : fmaf(ts[s], ws_incl[s - 1], -wts_incl[s - 1]);
        const float second = fmaf(-ts[s], ws_sum - ws_incl[s], wts_sum - wts_incl[s]);
        float v = g * 2 * (first + second);
        dL_dws[s] = fmaf(g * (float)2 / 3 * ws[s], deltas[s], v);
    }
}


// ------------------------------------------------------------------ NeRF loss (losses.py:47-60, train.py:178)
// pred = rgb + bg*(1-opacity) (rendering.py:153-161); loss = mean((pred-gt)^2) + lambda*mean(-o ln o),
// o = opacity + 1e-10.  Writes dL/drgb, dL/dopacity of that scalar and accumulates it into loss_sum.
template <bool DEV_BG>
__global__ void nerf_loss_kernel(const float* __restrict__ rgb, const float* __restrict__ opacity,
                                 const float* __restrict__ gt, int64_t n_rays, int64_t n_mean, float lambda_o,
                                 typename BgParam<DEV_BG>::first bg0, typename BgParam<DEV_BG>::rest bg1,
                                 typename BgParam<DEV_BG>::rest bg2, float* __restrict__ dL_drgb,
                                 float* __restrict__ dL_dop, float* __restrict__ loss_sum) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float l = 0.0f;
    if (r < n_rays) {
        const float op = opacity[r];
        const float inv3n = 1.0f / (3.0f * (float)n_mean), invn = 1.0f / (float)n_mean;
        float b0, b1, b2;
        bg_fetch<DEV_BG>(bg0, bg1, bg2, b0, b1, b2);
        const float bg[3] = {b0, b1, b2};
        float dop = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float e = rgb[3 * r + c] + bg[c] * (1.0f - op) - gt[3 * r + c];
            l += e * e * inv3n;
            const float g = 2.0f * e * inv3n;
            dL_drgb[3 * r + c] = g;
            dop -= bg[c] * g;
        }
        const float o = op + 1e-10f;
        l += lambda_o * (-o * logf(o)) * invn;
        dL_dop[r] = dop + lambda_o * (-(logf(o) + 1.0f)) * invn;
    }
    // wave reduction, one atomic per wave
    for (int off = 32; off > 0; off >>= 1) l += __shfl_down(l, off, 64);
    if ((threadIdx.x & 63) == 0 && loss_sum) atomicAdd(loss_sum, l);
}

// the two forms of mfnerf_composite_train_fused / mfnerf_nerf_loss: one validation, one launch
template <bool DEV_BG>
int composite_train_fused_launch(const char* what, const float* sigmas, const float* rgbs, const float* deltas,
                                 const float* ts, const int64_t* rays_a, int64_t n_rays, int64_t n_samples,
                                 float T_threshold, const float* target, int64_t n_mean, float lambda_opacity,
                                 typename BgParam<DEV_BG>::first bg0, typename BgParam<DEV_BG>::rest bg1,
                                 typename BgParam<DEV_BG>::rest bg2, int64_t* total_samples, float* opacity,
                                 float* depth, float* rgb, float* ws, float* dL_drgb, float* dL_dopacity,
                                 float* dL_dsigmas, float* dL_drgbs, float* loss_partials, mfnerf_stream_t stream) {
    if (n_rays < 0 || n_samples < 0 || n_mean < 0 || (n_mean > 0 && n_mean < n_rays)) {
        mfn_set_error("%s: bad sizes", what); return MFN_ERR_INVALID;
    }
    if (n_mean == 0) n_mean = n_rays;
    if (n_rays == 0) return MFN_OK;
    if (!rays_a || !target || !total_samples || !opacity || !depth || !rgb || !dL_drgb || !dL_dopacity ||
        (n_samples > 0 && (!sigmas || !rgbs || !deltas || !ts || !ws || !dL_dsigmas || !dL_drgbs))) {
        mfn_set_error("%s: null pointer", what); return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(composite_fused_wave_kernel<DEV_BG>, dim3(blocks_for(n_rays, 4)), dim3(256), 0, stream, sigmas,
                       rgbs, deltas, ts, rays_a, n_rays, T_threshold, target, n_mean, lambda_opacity, bg0, bg1, bg2,
                       total_samples, opacity, depth, rgb, ws, dL_drgb, dL_dopacity, dL_dsigmas, dL_drgbs,
                       loss_partials);
    return mfn_check_launch(what);
}

template <bool DEV_BG>
int nerf_loss_launch(const char* what, const float* rgb, const float* opacity, const float* target, int64_t n_rays,
                     int64_t n_mean, float lambda_opacity, typename BgParam<DEV_BG>::first bg0,
                     typename BgParam<DEV_BG>::rest bg1, typename BgParam<DEV_BG>::rest bg2, float* dL_drgb,
                     float* dL_dopacity, float* loss_sum, mfnerf_stream_t stream) {
    if (n_rays < 0 || n_mean < 0 || (n_mean > 0 && n_mean < n_rays)) {
        mfn_set_error("%s: bad size", what); return MFN_ERR_INVALID;
    }
    if (n_mean == 0) n_mean = n_rays;
    if (n_rays == 0) return MFN_OK;
    if (!rgb || !opacity || !target || !dL_drgb || !dL_dopacity) {
        mfn_set_error("%s: null pointer", what); return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(nerf_loss_kernel<DEV_BG>, dim3(blocks_for(n_rays, 256)), dim3(256), 0, stream, rgb, opacity,
                       target, n_rays, n_mean, lambda_opacity, bg0, bg1, bg2, dL_drgb, dL_dopacity, loss_sum);
    return mfn_check_launch(what);
}

}  // namespace

extern "C" {

int mfnerf_composite_train_fw(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                              const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float T_threshold,
                              int64_t* total_samples, float* opacity, float* depth, float* rgb, float* ws,
                              mfnerf_stream_t stream) {
    if (n_rays < 0 || n_samples < 0) { mfn_set_error("composite_train_fw: bad sizes"); return MFN_ERR_INVALID; }
    if (n_rays == 0) return MFN_OK;
    if (!rays_a || !total_samples || !opacity || !depth || !rgb ||
        (n_samples > 0 && (!sigmas || !rgbs || !deltas || !ts || !ws))) {
        mfn_set_error("composite_train_fw: null pointer"); return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(composite_fw_wave_kernel, dim3(blocks_for(n_rays, 4)), dim3(256), 0, stream, sigmas, rgbs, deltas,
                       ts, rays_a, n_rays, T_threshold, total_samples, opacity, depth, rgb, ws);
    return mfn_check_launch("composite_train_fw");
}

int mfnerf_composite_train_bw(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb,
                              const float* dL_dws, const float* sigmas, const float* rgbs, const float* ws,
                              const float* deltas, const float* ts, const int64_t* rays_a, const float* opacity,
                              const float* depth, const float* rgb, int64_t n_rays, int64_t n_samples,
                              float T_threshold, float* dL_dsigmas, float* dL_drgbs, mfnerf_stream_t stream) {
    if (n_rays < 0 || n_samples < 0) { mfn_set_error("composite_train_bw: bad sizes"); return MFN_ERR_INVALID; }
    if (n_rays == 0) return MFN_OK;
    if (!dL_dopacity || !dL_ddepth || !dL_drgb || !rays_a || !opacity || !depth || !rgb ||
        (n_samples > 0 && (!dL_dws || !sigmas || !rgbs || !ws || !deltas || !ts || !dL_dsigmas || !dL_drgbs))) {
        mfn_set_error("composite_train_bw: null pointer"); return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(composite_bw_wave_kernel, dim3(blocks_for(n_rays, 4)), dim3(256), 0, stream,
                       dL_dopacity, dL_ddepth, dL_drgb, dL_dws, sigmas, rgbs, ws, deltas, ts, rays_a, opacity,
                       depth, rgb, n_rays, T_threshold, dL_dsigmas, dL_drgbs);
    return mfn_check_launch("composite_train_bw");
}

int mfnerf_composite_train_fused(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                                 const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float T_threshold,
                                 const float* target, int64_t n_mean, float lambda_opacity, float bg_r, float bg_g,
                                 float bg_b, int64_t* total_samples, float* opacity, float* depth, float* rgb,
                                 float* ws, float* dL_drgb, float* dL_dopacity, float* dL_dsigmas, float* dL_drgbs,
                                 float* loss_partials, mfnerf_stream_t stream) {
    return composite_train_fused_launch<false>("composite_train_fused", sigmas, rgbs, deltas, ts, rays_a, n_rays,
                                               n_samples, T_threshold, target, n_mean, lambda_opacity, bg_r, bg_g, bg_b,
                                               total_samples, opacity, depth, rgb, ws, dL_drgb, dL_dopacity,
                                               dL_dsigmas, dL_drgbs, loss_partials, stream);
}

int mfnerf_composite_train_fused_bg(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                                    const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float T_threshold,
                                    const float* target, int64_t n_mean, float lambda_opacity, const float* bg,
                                    int64_t* total_samples, float* opacity, float* depth, float* rgb, float* ws,
                                    float* dL_drgb, float* dL_dopacity, float* dL_dsigmas, float* dL_drgbs,
                                    float* loss_partials, mfnerf_stream_t stream) {
    if (!bg) { mfn_set_error("composite_train_fused_bg: null bg"); return MFN_ERR_INVALID; }
    return composite_train_fused_launch<true>("composite_train_fused_bg", sigmas, rgbs, deltas, ts, rays_a, n_rays,
                                              n_samples, T_threshold, target, n_mean, lambda_opacity, bg, BgUnused{},
                                              BgUnused{}, total_samples, opacity, depth, rgb, ws, dL_drgb, dL_dopacity,
                                              dL_dsigmas, dL_drgbs, loss_partials, stream);
}

int mfnerf_composite_test_fw(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                             int64_t* alive_indices, int64_t n_alive, int N_samples, float T_threshold,
                             const int32_t* n_eff, float* opacity, float* depth, float* rgb,
                             mfnerf_stream_t stream) {
    if (n_alive < 0 || N_samples < 0) { mfn_set_error("composite_test_fw: bad sizes"); return MFN_ERR_INVALID; }
    if (n_alive == 0) return MFN_OK;
    if (!alive_indices || !n_eff || !opacity || !depth || !rgb ||
        (N_samples > 0 && (!sigmas || !rgbs || !deltas || !ts))) {
        mfn_set_error("composite_test_fw: null pointer"); return MFN_ERR_INVALID;
    }
    hipLaunchKernelGGL(composite_test_kernel, dim3(blocks_for(n_alive, RAY_BLOCK)), dim3(RAY_BLOCK), 0, stream,
                       sigmas, rgbs, deltas, ts, alive_indices, n_alive, N_samples, T_threshold, n_eff, opacity,
                       depth, rgb);
    return mfn_check_launch("composite_test_fw");
}

int mfnerf_distortion_loss_fw(const float* ws, const float* deltas, const float* ts, const int64_t* rays_a,
                              int64_t n_rays, int64_t n_samples, float* loss, float* ws_incl, float* wts_incl,
                              mfnerf_stream_t stream) {
    if (n_rays < 0 || n_samples < 0) { mfn_set_error("distortion_loss_fw: bad sizes"); return MFN_ERR_INVALID; }
    if (n_rays == 0) return MFN_OK;
    if (!rays_a || !loss || (n_samples > 0 && (!ws || !deltas || !ts || !ws_incl || !wts_incl))) {
        mfn_set_error("distortion_loss_fw: null pointer"); return MFN_ERR_INVALID;
    }
    mfn_zero_async(loss, n_rays * sizeof(float), stream);
    hipLaunchKernelGGL(distortion_fw_kernel, dim3(blocks_for(n_rays, RAY_BLOCK)), dim3(RAY_BLOCK), 0, stream, ws,
                       deltas, ts, rays_a, n_rays, loss, ws_incl, wts_incl);
    return mfn_check_launch("distortion_loss_fw");
}

int mfnerf_distortion_loss_bw(const float* dL_dloss, const float* ws_incl, const float* wts_incl,
                              const float* ws, const float* deltas, const float* ts, const int64_t* rays_a,
                              int64_t n_rays, int64_t n_samples, float* dL_dws, mfnerf_stream_t stream) {
    if (n_rays < 0 || n_samples < 0) { mfn_set_error("distortion_loss_bw: bad sizes"); return MFN_ERR_INVALID; }
    if (n_rays == 0) return MFN_OK;
    if (!dL_dloss || !rays_a || (n_samples > 0 && (!ws_incl || !wts_incl || !ws || !deltas || !ts || !dL_dws))) {
        mfn_set_error("distortion_loss_bw: null pointer"); return MFN_ERR_INVALID;
    }
    if (n_samples > 0) mfn_zero_async(dL_dws, n_samples * sizeof(float), stream);
    hipLaunchKernelGGL(distortion_bw_kernel, dim3(blocks_for(n_rays, RAY_BLOCK)), dim3(RAY_BLOCK), 0, stream,
                       dL_dloss, ws_incl, wts_incl, ws, deltas, ts, rays_a, n_rays, dL_dws);
    return mfn_check_launch("distortion_loss_bw");
}

int mfnerf_nerf_loss(const float* rgb, const float* opacity, const float* target, int64_t n_rays, int64_t n_mean,
                     float lambda_opacity, float bg_r, float bg_g, float bg_b, float* dL_drgb, float* dL_dopacity,
                     float* loss_sum, mfnerf_stream_t stream) {
    return nerf_loss_launch<false>("nerf_loss", rgb, opacity, target, n_rays, n_mean, lambda_opacity, bg_r, bg_g, bg_b,
                                   dL_drgb, dL_dopacity, loss_sum, stream);
}

int mfnerf_nerf_loss_bg(const float* rgb, const float* opacity, const float* target, int64_t n_rays, int64_t n_mean,
                        float lambda_opacity, const float* bg, float* dL_drgb, float* dL_dopacity, float* loss_sum,
                        mfnerf_stream_t stream) {
    if (!bg) { mfn_set_error("nerf_loss_bg: null bg"); return MFN_ERR_INVALID; }
    return nerf_loss_launch<true>("nerf_loss_bg", rgb, opacity, target, n_rays, n_mean, lambda_opacity, bg, BgUnused{},
                                  BgUnused{}, dL_drgb, dL_dopacity, loss_sum, stream);
}

}  // extern "C"
