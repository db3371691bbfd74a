// vren_march.hip -- ray marching through the occupancy grid (raymarching.cu:166-454) and its C-ABI
// entry points.  Every marcher walks the step of ray_march.hpp.  raymarching_train is
// count -> one-workgroup prefix scan -> write, with the sample count kept on the device (no host sync,
// graph-capturable) and rays_a in canonical ray order; constant-dt scenes take the wave-per-ray
// marcher in place of count and write.
#include "ray_march.hpp"
#include "wave_ops.hpp"
#include "vren_launch.hpp"

using namespace mfn;
using namespace mfn_vren;

namespace {

struct MarchParams {
    const float* o; const float* d; const float* hits_t; int64_t hits_stride;
    const uint8_t* bitfield; int cascades; float scale; float exp_step; const float* noise;
    int grid_size; int max_samples;
};

// Marches ray r (raymarching.cu:190-234 / :243-279).  WRITE=false counts (up to max_samples);
// WRITE=true re-marches and stores the first `limit` samples at `base`.
template <bool WRITE>
__device__ __forceinline__ int march_ray(const MarchParams& p, int64_t r, int limit, int64_t base,
                                         float* __restrict__ xyzs, float* __restrict__ dirs,
                                         float* __restrict__ deltas, float* __restrict__ ts) {
    const MarchGrid g = train_grid(p);
    const Ray ray = load_ray(p.o, p.d, r);
    float t1 = p.hits_t[r * p.hits_stride], t2 = p.hits_t[r * p.hits_stride + 1];
    if (t1 >= 0) t1 = fmaf(march_dt(g, t1), p.noise[r], t1);
    float t = t1; int n = 0;
    while (0 <= t && t < t2 && n < limit) {
        const MarchPoint m = march_point(g, ray, t);
        if (m.c.occ) {
            if (WRITE) {
                const int64_t s = base + n;
                xyzs[3 * s] = m.x; xyzs[3 * s + 1] = m.y; xyzs[3 * s + 2] = m.z;
                dirs[3 * s] = ray.dx; dirs[3 * s + 1] = ray.dy; dirs[3 * s + 2] = ray.dz;
                ts[s] = t; deltas[s] = m.dt;
            }
            t += m.dt; n++;
        } else {
            t = skip_empty(g, ray, m, t);
        }
    }
    return n;
}

__global__ void march_count_kernel(MarchParams p, int64_t n_rays, int32_t* __restrict__ counts) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    counts[r] = march_ray<false>(p, r, p.max_samples, 0, nullptr, nullptr, nullptr, nullptr);
}

// One-workgroup exclusive scan of the per-ray counts -> rays_a rows and counter (device resident).
// It runs on the side stream beside the table-gradient scatter, whose 1024-thread workgroups hold 4
// waves x 112 VGPRs of every SIMD: 64 VGPRs per SIMD lane stay free, room for ONE more wave of <= 64
// registers per SIMD.  So 256 threads (one wave per SIMD) at <= 64 VGPRs: the 512-thread form (two
// waves per SIMD) found no CU until the scatter ended -- 84 us in the step timeline
// (profiles/r05_v5_march_estimate_timeline.txt) for a few microseconds of work.
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_K = 16;  // counts per thread loaded together
__global__ __launch_bounds__(SCAN_THREADS) __attribute__((amdgpu_waves_per_eu(8))) void march_scan_kernel(
    const int32_t* __restrict__ counts, int64_t n_rays, int64_t capacity, int64_t* __restrict__ rays_a,
    int32_t* __restrict__ counter) {
    __shared__ int64_t wave_tot[SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = (int)n_rays;  // (<= 2^31: checked by the caller)
    const int chunk = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int b = tid * chunk, e = min(n, b + chunk);
    // SCAN_K counts per thread in flight together: one memory round trip per SCAN_K instead of chunk
    // dependent ones (beside the scatter every load waits behind its traffic)
    int64_t local = 0;
    for (int b0 = b; b0 < e; b0 += SCAN_K) {
        int32_t cr[SCAN_K];
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) cr[k] = counts[b0 + k < e ? b0 + k : 0];
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) local += b0 + k < e ? cr[k] : 0;
    }
    // inclusive wave scan
    int64_t v = local;
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    if (lane == 63) wave_tot[wid] = v;
    __syncthreads();
    if (wid == 0) {
        int64_t w = lane < SCAN_THREADS / 64 ? wave_tot[lane] : 0;
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t u = __shfl_up(w, off, 64);
            if (lane >= off) w += u;
        }
        if (lane < SCAN_THREADS / 64) wave_tot[lane] = w;  // inclusive per-wave totals
    }
    __syncthreads();
    int64_t run = (v - local) + (wid > 0 ? wave_tot[wid - 1] : 0);  // exclusive start of this chunk
    // the write pass re-reads the counts (cache hits now), SCAN_K at a time again, rather than keep
    // them live through the scan: the kernel must stay within 64 registers
    for (int b0 = b; b0 < e; b0 += SCAN_K) {
        int32_t cr[SCAN_K];
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) cr[k] = counts[b0 + k < e ? b0 + k : 0];
        for (int k = 0; k < SCAN_K && b0 + k < e; ++k) {
            const int64_t i = b0 + k, c = cr[k];
            rays_a[3 * i] = i;
            rays_a[3 * i + 1] = min(run, capacity);
            rays_a[3 * i + 2] = max<int64_t>(0, min(c, capacity - run));
            run += c;
        }
    }
    if (tid == SCAN_THREADS - 1) {
        counter[0] = (int32_t)min(run, capacity);
        counter[1] = (int32_t)n_rays;
    }
}

__global__ void march_write_kernel(MarchParams p, int64_t n_rays, const int64_t* __restrict__ rays_a,
                                   float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ deltas,
                                   float* __restrict__ ts) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const int limit = (int)rays_a[3 * r + 2];
    if (limit == 0) return;
    march_ray<true>(p, r, limit, rays_a[3 * r + 1], xyzs, dirs, deltas, ts);
}

// ---- wave-per-ray marching for constant dt (exp_step_factor == 0: every synthetic scene).
// One wave marches one ray 64 chain points at a time.  The chain t_{k+1} = fl(t_k + dt) that both
// reference branches walk (raymarching.cu:223,230-232) is laid on the lanes in closed form,
// t_j = fmaf(j, delta, t_base) with delta = fl(t_base+dt) - t_base, and every lane checks
// fl(t_j + dt) == t_{j+1}: the chunk is truncated at the first mismatch (binade crossing, tie), so
// the lane values ARE the sequential chain.  Each live lane looks up its cell; a scalar walk over
// the lanes then replays the reference's control flow exactly (occupied: emit and step; empty:
// jump to the first chain point >= the DDA target), and the emitted lanes are compacted with a
// ballot prefix count.  Bit-identical to march_ray<> (and the oracle), ~64x more parallel.
// The march runs ONCE: it counts the ray's samples and keeps their t values at tbuf[r * max_samples
// + j]; after the scan, march_expand_kernel writes the compacted samples from them (x = fmaf(t, d, o)
// as here, the ray's direction, t, the constant dt).  Until round 3 a second march re-walked every
// ray to write (count + re-march ~250 us on the side stream, beside the table-gradient scatter).

// One chunk of the chain on the lanes: its points, where the successor chain breaks, the next chunk's
// base, and each live lane's cell with its bitfield byte requested (chunk_occ reads it later).
struct MarchChunk {
    float t_base, tl, x, y, z, next_base;
    int chain_end;
    bool live;
    Cell c;
    uint32_t bit;      // bit of the cell in its byte
    uint32_t byte;     // the bitfield byte (in flight until chunk_occ)
};

__device__ __forceinline__ MarchChunk march_chunk(const MarchParams& p, float t_base, float dt, float t2,
                                                  const Ray& ray, int lane, float inv_scale) {
    MarchChunk k;
    k.t_base = t_base;
    const float delta = (t_base + dt) - t_base;
    k.tl = fmaf((float)lane, delta, t_base);
    const float succ = k.tl + dt;
    const float tl_next = __shfl_down(k.tl, 1, 64);
    const uint64_t bad = __ballot(lane < 63 && succ != tl_next);
    k.chain_end = bad ? ffs64(bad) + 1 : 64;
    k.next_base = readlane_f(succ, k.chain_end - 1);
    k.live = lane < k.chain_end && k.tl < t2;
    k.x = fmaf(k.tl, ray.dx, ray.ox); k.y = fmaf(k.tl, ray.dy, ray.oy); k.z = fmaf(k.tl, ray.dz, ray.oz);
    // lookup_cell's arithmetic on every lane (branch-free: a load under a lane condition makes the
    // compiler wait for every outstanding load where the paths join, i.e. for this prefetch), the
    // byte load issued here and used a chunk later; a lane past the chain reads byte 0
    const uint32_t g3 = (uint32_t)p.grid_size * p.grid_size * p.grid_size;
    const int mip = max(mip_from_pos(k.x, k.y, k.z, p.cascades), mip_from_dt(dt, p.grid_size, p.cascades));
    k.c.mip_bound = fminf(scalbnf(1.0f, mip - 1), p.scale);
    // lookup_cell's 1 / mip_bound without a per-lane IEEE division: 2^(1-mip) is exact, and 1/scale
    // is the same correctly rounded quotient computed once (inv_scale)
    const float inv = k.c.mip_bound == p.scale ? inv_scale : scalbnf(1.0f, 1 - mip);
    const float gs = (float)p.grid_size, gm1 = (float)p.grid_size - 1.0f;
    k.c.nx = (int)clampf(0.5f * fmaf(k.x, inv, 1.0f) * gs, 0.0f, gm1);
    k.c.ny = (int)clampf(0.5f * fmaf(k.y, inv, 1.0f) * gs, 0.0f, gm1);
    k.c.nz = (int)clampf(0.5f * fmaf(k.z, inv, 1.0f) * gs, 0.0f, gm1);
    const uint32_t idx = (uint32_t)mip * g3 + morton3((uint32_t)k.c.nx, (uint32_t)k.c.ny, (uint32_t)k.c.nz);
    k.bit = idx & 7;
    k.byte = p.bitfield[k.live ? idx >> 3 : 0u];
    return k;
}

__device__ __forceinline__ void march_wave_ray(const MarchParams& p, int64_t r, int32_t* __restrict__ counts,
                                               float* __restrict__ tbuf) {
    const int lane = threadIdx.x & 63;
    const int limit = p.max_samples;
    float* tr = tbuf + r * (int64_t)p.max_samples;
    const MarchGrid g = train_grid(p);
    const Ray ray = load_ray(p.o, p.d, r);
    float t1 = p.hits_t[r * p.hits_stride];
    const float t2 = p.hits_t[r * p.hits_stride + 1];
    int n = 0;
    if (t1 >= 0) {
        const float dt = march_dt(g, t1);  // constant
        t1 = fmaf(dt, p.noise[r], t1);
        float t_base = t1, pending = 0.0f;
        bool skip = false, done = false;
        // round 5: the next chunk's points are pure arithmetic (the chain does not depend on the
        // walk), so its bitfield bytes are requested before this chunk's walk -- one memory round trip
        // hidden per chunk (the march runs beside the table-gradient scatter, where every load waits
        // behind its traffic)
        const float inv_scale = 1 / p.scale;
        MarchChunk cur = march_chunk(p, t_base, dt, t2, ray, lane, inv_scale);
        while (!done) {
            if (!(t_base < t2) || n >= limit) break;  // every later visited point fails the loop test
            const MarchChunk nxt = march_chunk(p, cur.next_base, dt, t2, ray, lane, inv_scale);
            const float tl = cur.tl;
            const int chain_end = cur.chain_end;
            const bool live = cur.live;
            const bool occ = live && ((cur.byte >> cur.bit) & 1u);
            const float tt = live && !occ ? skip_target(tl, cur.c, cur.x, cur.y, cur.z, ray, g.gsi) : 0.0f;
            const uint64_t live_m = __ballot(live), occ_m = __ballot(occ);
            const uint64_t chain_m = chain_end == 64 ? ~0ull : ((1ull << chain_end) - 1);
            // Round 5: the empty cells' DDA jumps resolved on the lanes instead of one scalar walk step
            // per empty cell (PMC: 27.8 M SALU vs 12.6 M VALU instructions, issue-blocked 50 % -- the
            // march was bound by its scalar walk).  Empty live lane j jumps to J(j) = the first chain
            // lane k > j with tl_k >= tt_j (tl_k = fmaf(k, delta, t_base) is monotone in k: a binary
            // search over the closed form, no lookups), or OUT (64) past the chunk.  Pointer doubling
            // over those jumps (occupied and non-live lanes stop) gives every lane the lane the walk
            // lands on from it, and the lane whose jump leaves the chunk (its target becomes the next
            // chunk's pending skip).  The scalar walk then steps once per occupied run instead of once
            // per empty cell.  The visited set -- hence counts, samples, order -- is the walk's own.
            constexpr int OUT = 64;
            int P = lane, L = -1;
            if (live && !occ) {
                // first k in [0, chain_end) with tl_k >= tt (chain_end: none).  Inside the verified
                // chain tl_k = t_base + k delta exactly, so k = ceil((tt - t_base) / delta); the
                // estimate (approximate reciprocal: off by far less than a lane) is put right by one
                // exact comparison each way
                const float delta = (cur.t_base + dt) - cur.t_base;
                const float est = (tt - cur.t_base) * __builtin_amdgcn_rcpf(delta);
                int k = tt == tt ? (int)ceilf(fminf(fmaxf(est, 0.0f), (float)chain_end)) : chain_end;
                if (k > 0 && fmaf((float)(k - 1), delta, cur.t_base) >= tt) --k;
                if (k < chain_end && !(fmaf((float)k, delta, cur.t_base) >= tt)) ++k;
                const int J = max(k, lane + 1);
                P = J < chain_end ? J : OUT;
                L = J < chain_end ? -1 : lane;
            }
#pragma unroll
            for (int it = 0; it < 6; ++it) {
                const int q = min(P, 63);
                const int Pq = __shfl(P, q, 64), Lq = __shfl(L, q, 64);
                if (P < OUT) { P = Pq; L = Lq; }
            }
            uint64_t emit_m = 0;
            const int n0 = n;
            int c = 0;
            if (skip) {
                const uint64_t ge = __ballot(tl >= pending) & chain_m;
                if (ge) { c = ffs64(ge); skip = false; } else c = chain_end;
            }
            while (c < chain_end) {
                const int s = __builtin_amdgcn_readlane(P, c);  // (c itself when occupied or not live)
                if (s >= OUT) {
                    skip = true;
                    pending = readlane_f(tt, __builtin_amdgcn_readlane(L, c));
                    break;
                }
                c = s;
                if (!((live_m >> c) & 1) || n >= limit) { done = true; break; }
                const uint64_t rest = ~(occ_m >> c);  // (lane c is occupied)
                int len = rest ? ffs64(rest) : 64 - c;
                len = min(len, limit - n);
                emit_m |= (len >= 64 ? ~0ull : ((1ull << len) - 1)) << c;
                n += len; c += len;
            }
            if ((emit_m >> lane) & 1) tr[n0 + __popcll(emit_m & ((1ull << lane) - 1))] = tl;
            t_base = cur.next_base;
            cur = nxt;
        }
    }
    if (lane == 0) counts[r] = n;
}

// one ray per wave per trip; a wave takes rays w, w + W, ... (W = the grid's waves)
__global__ __launch_bounds__(256) void march_wave_kernel(MarchParams p, int64_t n_rays, int32_t* __restrict__ counts,
                                                         float* __restrict__ tbuf) {
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_rays; r += nw)  // wave-uniform
        march_wave_ray(p, r, counts, tbuf);
}


// The compacted samples of ray r (one wave): its first rays_a[r].count t values from march_wave.
// <= 64 VGPRs (waves_per_eu(8)): the kernel follows the scan beside the scatter, which leaves 64
// registers per SIMD lane free (see march_scan_kernel); at 68 it waited for the scatter to end and ran
// beside the accumulate instead.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void march_expand_kernel(MarchParams p, int64_t n_rays,
                                                           const int64_t* __restrict__ rays_a,
                                                           const float* __restrict__ tbuf, float* __restrict__ xyzs,
                                                           float* __restrict__ dirs, float* __restrict__ deltas,
                                                           float* __restrict__ ts) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= n_rays) return;  // wave-uniform
    const int cnt = (int)rays_a[3 * r + 2];
    if (cnt == 0) return;
    const int64_t base = rays_a[3 * r + 1];
    const float ox = p.o[3 * r], oy = p.o[3 * r + 1], oz = p.o[3 * r + 2];
    const float dx = p.d[3 * r], dy = p.d[3 * r + 1], dz = p.d[3 * r + 2];
    // march_wave's constant step, from the same un-perturbed entry point
    const float dt = calc_dt(p.hits_t[r * p.hits_stride], p.exp_step, p.max_samples, p.grid_size, p.scale);
    const float* tr = tbuf + r * (int64_t)p.max_samples;
    for (int j = lane; j < cnt; j += 64) {
        const float t = tr[j];
        const int64_t s = base + j;
        xyzs[3 * s] = fmaf(t, dx, ox); xyzs[3 * s + 1] = fmaf(t, dy, oy); xyzs[3 * s + 2] = fmaf(t, dz, oz);
        dirs[3 * s] = dx; dirs[3 * s + 1] = dy; dirs[3 * s + 2] = dz;
        ts[s] = t; deltas[s] = dt;
    }
}

// raymarching_test_kernel (raymarching.cu:335-404) with the calc_dt(..., cascades) quirk (test_grid).
__global__ void march_test_kernel(MarchParams p, float* __restrict__ hits_t, const int64_t* __restrict__ alive,
                                  int64_t n_alive, int N_samples, float* __restrict__ xyzs, float* __restrict__ dirs,
                                  float* __restrict__ deltas, float* __restrict__ ts, int32_t* __restrict__ n_eff) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int64_t r = alive[n];
    const MarchGrid g = test_grid(p);
    const Ray ray = load_ray(p.o, p.d, r);
    float t = hits_t[r * p.hits_stride], t2 = hits_t[r * p.hits_stride + 1];
    const int64_t row = n * N_samples;
    int s = 0;
    while (t < t2 && s < N_samples) {
        const MarchPoint m = march_point(g, ray, t);
        if (m.c.occ) {
            const int64_t k = row + s;
            xyzs[3 * k] = m.x; xyzs[3 * k + 1] = m.y; xyzs[3 * k + 2] = m.z;
            dirs[3 * k] = ray.dx; dirs[3 * k + 1] = ray.dy; dirs[3 * k + 2] = ray.dz;
            ts[k] = t; deltas[k] = m.dt;
            t += m.dt;
            hits_t[r * p.hits_stride] = t;
            s++;
        } else {
            t = skip_empty(g, ray, m, t);
        }
    }
    for (int k = s; k < N_samples; ++k) {  // zero the unused tail of this row (the reference zero-fills)
        const int64_t q = row + k;
        xyzs[3 * q] = 0.f; xyzs[3 * q + 1] = 0.f; xyzs[3 * q + 2] = 0.f;
        dirs[3 * q] = 0.f; dirs[3 * q + 1] = 0.f; dirs[3 * q + 2] = 0.f;
        ts[q] = 0.f; deltas[q] = 0.f;
    }
    n_eff[n] = s;
}

}  // namespace

extern "C" {

// the per-ray counts, then (constant-dt scenes) the per-ray sample t values of march_wave
int64_t mfnerf_raymarching_train_workspace(int64_t n_rays, int max_samples) {
    const int64_t counts = ((n_rays * 4 + 255) / 256) * 256;
    return counts + (max_samples > 0 ? n_rays * (int64_t)max_samples * 4 : 0);
}

int mfnerf_raymarching_train(const float* rays_o, const float* rays_d, const float* hits_t, int64_t hits_stride,
                             const uint8_t* bitfield, int cascades, float scale, float exp_step_factor,
                             const float* noise, int grid_size, int max_samples, int64_t n_rays, int64_t capacity,
                             int64_t* rays_a, float* xyzs, float* dirs, float* deltas, float* ts, int32_t* counter,
                             void* workspace, mfnerf_stream_t stream) {
    if (n_rays < 0 || n_rays > INT32_MAX - SCAN_THREADS || capacity < 0 || cascades < 1 || grid_size < 1 ||
        grid_size > 1024 || max_samples < 1 || hits_stride < 2) {
        mfn_set_error("raymarching_train: bad arguments"); return MFN_ERR_INVALID;
    }
    if (!counter) { mfn_set_error("raymarching_train: null counter"); return MFN_ERR_INVALID; }
    if (n_rays == 0) { mfn_zero_async(counter, 8, stream); return mfn_check_launch("raymarching_train"); }
    if (!rays_o || !rays_d || !hits_t || !bitfield || !noise || !rays_a || !workspace ||
        (capacity > 0 && (!xyzs || !dirs || !deltas || !ts))) {
        mfn_set_error("raymarching_train: null pointer"); return MFN_ERR_INVALID;
    }
    MarchParams p{rays_o, rays_d, hits_t, hits_stride, bitfield, cascades, scale, exp_step_factor, noise,
                  grid_size, max_samples};
    int32_t* counts = (int32_t*)workspace;
    float* tbuf = reinterpret_cast<float*>((char*)workspace + ((n_rays * 4 + 255) / 256) * 256);
    const unsigned nb = blocks_for(n_rays, RAY_BLOCK);
    const bool wave = exp_step_factor == 0.0f;  // constant dt: the wave-per-ray marcher applies
    const unsigned nbw = (unsigned)div_up<int64_t>(n_rays, 4);
    if (wave)
        hipLaunchKernelGGL(march_wave_kernel, dim3(nbw), dim3(256), 0, stream, p, n_rays, counts, tbuf);
    else
        hipLaunchKernelGGL(march_count_kernel, dim3(nb), dim3(RAY_BLOCK), 0, stream, p, n_rays, counts);
    hipLaunchKernelGGL(march_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, counts, n_rays, capacity, rays_a,
                       counter);
    if (wave)
        hipLaunchKernelGGL(march_expand_kernel, dim3(nbw), dim3(256), 0, stream, p, n_rays, rays_a, tbuf, xyzs,
                           dirs, deltas, ts);
    else
        hipLaunchKernelGGL(march_write_kernel, dim3(nb), dim3(RAY_BLOCK), 0, stream, p, n_rays, rays_a, xyzs, dirs,
                           deltas, ts);
    return mfn_check_launch("raymarching_train");
}

int mfnerf_raymarching_test(const float* rays_o, const float* rays_d, float* hits_t, int64_t hits_stride,
                            const int64_t* alive_indices, int64_t n_alive, const uint8_t* bitfield, int cascades,
                            float scale, float exp_step_factor, int grid_size, int max_samples, int N_samples,
                            float* xyzs, float* dirs, float* deltas, float* ts, int32_t* n_eff,
                            mfnerf_stream_t stream) {
    if (n_alive < 0 || N_samples < 0 || cascades < 1 || grid_size < 1 || grid_size > 1024 || max_samples < 1 ||
        hits_stride < 2) {
        mfn_set_error("raymarching_test: bad arguments"); return MFN_ERR_INVALID;
    }
    if (n_alive == 0) return MFN_OK;
    if (!rays_o || !rays_d || !hits_t || !alive_indices || !bitfield || !n_eff ||
        (N_samples > 0 && (!xyzs || !dirs || !deltas || !ts))) {
        mfn_set_error("raymarching_test: null pointer"); return MFN_ERR_INVALID;
    }
    MarchParams p{rays_o, rays_d, hits_t, hits_stride, bitfield, cascades, scale, exp_step_factor, nullptr,
                  grid_size, max_samples};
    hipLaunchKernelGGL(march_test_kernel, dim3(blocks_for(n_alive, RAY_BLOCK)), dim3(RAY_BLOCK), 0, stream, p,
                       hits_t, alive_indices, n_alive, N_samples, xyzs, dirs, deltas, ts, n_eff);
    return mfn_check_launch("raymarching_test");
}

}  // extern "C"

