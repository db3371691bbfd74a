// grid_bw_atomic.hip -- the hash-grid table gradient by memory-side atomics: the request-shaped
// scatter over all levels (grid_bw_kernel), the dense coarse levels one sample per lane
// (grid_bw_dense_kernel), the float path's fold of their private copies (the fixed-point path's
// convert pass: grid_adam_fixed.hpp), and the per-level L1 norm the fixed-point scales come from.
#include <algorithm>

#include "grid_common.hpp"
#include "grid_internal.hpp"

using namespace mfn;
using namespace mfn_grid;

namespace {

// Backward.  The table gradient is a scatter-add; on MI355X a float atomic executes at the memory
// side and costs one request per distinct 64-B line of a wave-instruction -- lanes of one line are
// free, lanes on the SAME address are not coalesced (tools/atomic_probe2.hip) -- so the kernel is
// shaped to minimise requests, not bytes:
//   * one wave = 16 consecutive samples, walking all levels; lane = (xb, f, s) with the sample s
//     fastest: per (y,z) corner pair the 4 lanes of a sample add to entries idx(x), idx(x+1) x
//     features f0,f1 -- one 16-B span, i.e. one line for dense levels and, for hashed levels,
//     whenever x->x+1 leaves the hash's low bits alone (7/8 of the time);
//   * consecutive samples lie along a ray, so coarse levels repeat a corner for many samples: a
//     4-step segmented suffix scan (DPP row shifts inside each 16-lane row = one (xb,f) stream)
//     merges such runs and only run heads issue the atomic;
//   * the dense coarse levels (a few hundred to a few thousand hot lines) add into GRAD_COPIES
//     private copies, picked per wave, folded back by fold_copies_kernel.
// MAXL: level-count bound (16 or 32) sizing the LDS tile and the prefetch registers.
// FIX: fixed-point accumulation -- per level l, each (run-merged) contribution v is added as the
// int32 rint(v * scale_l) with global_atomic_add (integer atomics run ~28% faster than float ones
// at the memory side, tools/atomic_probe3.hip), scale_l = fixed_scale(level_l1[l]); the buffers
// then hold int32 bit patterns until fold_convert_kernel turns them back into floats.
// the scatter as workgroup `bid` of `nblk` (a launch of its own, or a share of a fused launch)
template <int MAXL, bool FIX>
__device__ __forceinline__ void grid_bw_body(int bid, int nblk, const float* __restrict__ X, int64_t n,
                                             const int32_t* __restrict__ n_dev, float x_min, float x_range,
                                             const mfnerf_grid_desc& D, const float* __restrict__ dy,
                                             float* __restrict__ grad, float* __restrict__ priv,
                                             int64_t dense_entries, const float* __restrict__ level_l1, int l_end) {
    // dL/dy of the wave's chunk (16 samples x 2L floats) is staged in LDS (rows padded by one
    // float: conflict-free column reads) and the NEXT chunk is prefetched into registers before
    // this chunk's atomics are issued.  On gfx9 no-return atomics count in vmcnt, so a global load
    // between atomics would make the wave wait for every earlier atomic's round trip; with the
    // loads hoisted there is at most one such wait per chunk (64 atomics) instead of per level.
    __shared__ float sdy_all[ENC_BLOCK / 64][16 * (2 * MAXL + 1)];
    const int L_ = D.n_levels;
    const int lane = threadIdx.x & 63, s = lane & 15, f = (lane >> 4) & 1, xb = lane >> 5;
    const int row = 2 * L_, rs = 2 * L_ + 1, per_chunk = 16 * row;
    float* sdy = sdy_all[threadIdx.x >> 6];
    __shared__ float fs_s[MAXL];  // fixed-point scale per level (its table's)
    if (FIX) {
        if ((int)threadIdx.x < L_) fs_s[threadIdx.x] = table_fixed_scale(D, level_l1, threadIdx.x);
        __syncthreads();
    }
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int64_t chunks = div_up<int64_t>(nn, 16);
    const int64_t wave0 = ((int64_t)bid * ENC_BLOCK + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)nblk * ENC_BLOCK) >> 6;
    const int64_t n_vals = nn * row;

    float pf[MAXL / 2];  // this lane's share of a chunk's dL/dy
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    auto fetch = [&](int64_t ch) {
        const int64_t base = ch * per_chunk;
#pragma unroll
        for (int k = 0; k < MAXL / 2; ++k) {
            const int idx = lane + 64 * k;
            pf[k] = (idx < per_chunk && base + idx < n_vals) ? dy[base + idx] : 0.0f;
        }
        const int64_t i = ch * 16 + s;
        if (i < nn) { px = X[3 * i]; py = X[3 * i + 1]; pz = X[3 * i + 2]; }
    };
    if (wave0 < chunks) fetch(wave0);
    for (int64_t chunk = wave0; chunk < chunks; chunk += n_waves) {
        const int64_t i = chunk * 16 + s;
        const bool valid = i < nn;
#pragma unroll
        for (int k = 0; k < MAXL / 2; ++k) {
            const int idx = lane + 64 * k;
            if (idx < per_chunk) sdy[(idx / row) * rs + idx % row] = pf[k];
        }
        const float x = valid ? (px - x_min) / x_range : 0.0f;
        const float y = valid ? (py - x_min) / x_range : 0.0f;
        const float z = valid ? (pz - x_min) / x_range : 0.0f;
        if (chunk + n_waves < chunks) fetch(chunk + n_waves);  // in flight during this chunk's atomics
        const float* srow = sdy + s * rs + f;
        for (int l = l_end >> 8; l < (l_end & 255); ++l) {  // levels [l_end >> 8, l_end & 255)
            const float g = srow[2 * l];
            const float fs = FIX ? fs_s[l] : 0.0f;
            const LevelGeo Lg = level_geo(D.scale[l], x, y, z);
            const bool spread = priv && (int64_t)D.offset[l] + D.size[l] <= dense_entries;
            float* gt = spread ? priv + 2 * ((chunk & (GRAD_COPIES - 1)) * dense_entries + (int64_t)D.offset[l])
                               : grad + 2 * (int64_t)D.offset[l];
#pragma unroll
            for (int yz = 0; yz < 4; ++yz) {
                const int c = xb | (yz << 1);
                const uint32_t idx =
                    corner_index(D, l, Lg.g[0] + (c & 1), Lg.g[1] + ((c >> 1) & 1), Lg.g[2] + ((c >> 2) & 1));
                const int key = valid ? (int)idx : -1;
                float v = corner_weight(Lg, c) * g;
                const int kn = dpp_i<DPP_ROW_SHL(1)>(key), kp = dpp_i<DPP_ROW_SHR(1)>(key);
                const bool head = (s == 0) || kp != key;
                int stop = (s == 15) || kn != key;  // this lane ends its run
                // segmented suffix sum within the 16-lane row: run heads end up with the run total
                { const float vp = dpp_f<DPP_ROW_SHL(1)>(v); const int sp = dpp_i<DPP_ROW_SHL(1)>(stop); if (!stop) { v += vp; stop = sp; } }
                { const float vp = dpp_f<DPP_ROW_SHL(2)>(v); const int sp = dpp_i<DPP_ROW_SHL(2)>(stop); if (!stop) { v += vp; stop = sp; } }
                { const float vp = dpp_f<DPP_ROW_SHL(4)>(v); const int sp = dpp_i<DPP_ROW_SHL(4)>(stop); if (!stop) { v += vp; stop = sp; } }
                { const float vp = dpp_f<DPP_ROW_SHL(8)>(v); const int sp = dpp_i<DPP_ROW_SHL(8)>(stop); if (!stop) { v += vp; stop = sp; } }
                if (FIX && spread) {  // private copies: both features as one packed 64-bit add
                    const int q = (int)rintf(v * fs);
                    const int q1 = __shfl_down(q, 16, 64);  // the f = 1 lane of this (sample, corner)
                    const long long pq = (long long)((uint64_t)(uint32_t)q1 << 32) + (long long)q;
                    if (f == 0 && head && valid && pq != 0)
                        __hip_atomic_fetch_add(reinterpret_cast<long long*>(gt) + idx, pq, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                } else if (FIX) {
                    const int q = (int)rintf(v * fs);
                    if (head && valid && q != 0)
                        __hip_atomic_fetch_add(reinterpret_cast<int*>(gt) + 2 * idx + f, q, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                } else if (head && valid && v != 0.0f) {
                    __hip_atomic_fetch_add(gt + 2 * idx + f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

template <int MAXL, bool FIX>
__global__ __launch_bounds__(ENC_BLOCK) void grid_bw_kernel(const float* __restrict__ X, int64_t n,
                                                             const int32_t* __restrict__ n_dev, float x_min,
                                                             float x_range, const mfnerf_grid_desc D,
                                                             const float* __restrict__ dy, float* __restrict__ grad,
                                                             float* __restrict__ priv, int64_t dense_entries,
                                                             const float* __restrict__ level_l1, int l_end,
                                                             int32_t* __restrict__ zero_flag) {
    // zero_flag: a flag the NEXT launches on the stream start from zero (the binned scatter's slot
    // overflow), cleared here instead of by a memset launch of its own
    if (zero_flag && blockIdx.x == 0 && threadIdx.x == 0) *zero_flag = 0;
    grid_bw_body<MAXL, FIX>(blockIdx.x, gridDim.x, X, n, n_dev, x_min, x_range, D, dy, grad, priv,
                                    dense_entries, level_l1, l_end);
}

// Dense own-table levels [0, l_hi) into the private copies, one SAMPLE per lane.  grid_bw_body
// gives each sample 4 lanes (x-corner x feature) and merges runs with float segmented scans: it is
// VALU-bound (PMC: ~58 VALU wave-instructions per 16-sample row step; the same time with its
// atomics compiled out).  Here a lane holds its sample's whole cell (4 (y,z) rows x 2 x-corners x
// 2 features = 16 values) and a wave covers 64 consecutive samples (~ a ray):
//   * each value is rounded to the table's int32 fixed-point unit first (one rounding per sample
//     contribution); the run sums then come from an UNSEGMENTED integer prefix scan over the wave
//     (DPP row_shr 1/2/4/8 + row_bcast:15/:31 -- one v_add per step and value) as
//     P(tail) - P_excl(head): exact and order-free in two's complement;
//   * a run = consecutive samples in one cell (the 4 rows' keys change together), so one head/tail
//     structure serves all 16 values; heads and tails write their prefixes into a per-wave LDS
//     list, one entry per run;
//   * the list is issued 8 lanes per run -- (row, x-corner) -- each one 64-bit atomic carrying BOTH
//     features as the packed integer f1 * 2^32 + f0 (the fold decodes f0 = int32(low word),
//     f1 = int32(high word) + (f0 < 0); |sums| < 2^31 by the scale bound): a run costs 4 requests
//     (one 16-B span per row), 8 runs per instruction.
// Requires every level < l_hi to be a dense own table inside the private copies.

// a wave's window: consecutive chunks of 64 samples; the run open at a chunk's end is carried into
// the next chunk (per level, in LDS) instead of being issued twice.  Round 3 A/B (kbench, Lego step):
// 4 chunks 85 us; the smaller windows tried measured 95-101 us.  Round 6: the window is sized on the
// device from the live sample count so that ~DENSE_WAVES waves run, one window each -- the fixed
// 4-chunk window's optimum at the Lego step (~490 k samples: 1.9 k waves); at twice the samples
// (config 3's field, 16384 rays) 8 chunks ran 1.148 vs 1.184 ms/step, where the Lego step at 8
// chunks (960 waves) ran 0.526 vs 0.506 (r6o: profiles/r06_v7_ab_dense_window.txt).
constexpr int DENSE_WAVES = 2048;

struct DenseIn {
    float px, py, pz;
    bool valid;
};

template <int NG>  // float4 groups of dL/dy held per lane: levels < 2 NG
__global__ __launch_bounds__(ENC_BLOCK) void grid_bw_dense_kernel(const float* __restrict__ X, int64_t n,
                                                                  const int32_t* __restrict__ n_dev, float x_min,
                                                                  float x_range, const mfnerf_grid_desc D,
                                                                  const float* __restrict__ dy,
                                                                  float* __restrict__ priv, int64_t dense_entries,
                                                                  const float* __restrict__ level_l1, int l_hi,
                                                                  int32_t* __restrict__ zero_flag,
                                                                  int32_t* __restrict__ gate) {
    if (zero_flag && blockIdx.x == 0 && threadIdx.x == 0) *zero_flag = 0;
    // gate (gate.hip's {signals, waits, ticket}): opened as the table-gradient launches begin, so the
    // side stream's next march starts beside them with no one-thread signal kernel of its own on
    // the step's critical path
    if (gate && blockIdx.x == 0 && threadIdx.x == 0)  // relaxed: placement only (gate.hip)
        __hip_atomic_fetch_add(gate, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __shared__ float fs_s[MFN_MAX_LEVELS];
    // per wave, one entry per run: the 4 rows' (x0, x1) keys and the inclusive prefix at the run's
    // tail of the 16 values as 4 int4 (row r: x0f0, x0f1, x1f0, x1f1).  The runs tile the chunk's
    // valid lanes in order, so run r's exclusive prefix at its head is run r-1's tail prefix (0 for
    // r = 0): no head list (round 3: 45 -> 28 KB of LDS per block, 3 -> 4 blocks per CU)
    __shared__ int2 lkey[ENC_BLOCK / 64][64][4];
    __shared__ int4 ltail[ENC_BLOCK / 64][64][4];
    // per wave and level: the run left open at the previous chunk's end (sums, keys, on/off)
    __shared__ int4 csum[ENC_BLOCK / 64][2 * NG][4];
    __shared__ int2 ckey[ENC_BLOCK / 64][2 * NG][4];
    __shared__ int con[ENC_BLOCK / 64][2 * NG];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int)threadIdx.x < D.n_levels) fs_s[threadIdx.x] = table_fixed_scale(D, level_l1, threadIdx.x);
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int64_t n_waves = ((int64_t)gridDim.x * ENC_BLOCK) >> 6;
    const int row = 2 * D.n_levels;
    __syncthreads();  // fs_s
    auto load = [&](int64_t i, DenseIn& in, float4* gq) {
        in.valid = i < nn;
        in.px = in.valid ? (X[3 * i] - x_min) / x_range : 0.0f;
        in.py = in.valid ? (X[3 * i + 1] - x_min) / x_range : 0.0f;
        in.pz = in.valid ? (X[3 * i + 2] - x_min) / x_range : 0.0f;
        const float4* src = reinterpret_cast<const float4*>(dy + (in.valid ? i : 0) * row);
        const int ng = (2 * l_hi + 3) >> 2;
#pragma unroll
        for (int j = 0; j < NG; ++j) gq[j] = (in.valid && j < ng) ? src[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    const int64_t win = max<int64_t>(1, (nn + 64 * DENSE_WAVES - 1) / (64 * DENSE_WAVES));  // chunks (uniform)
    for (int64_t w = ((int64_t)blockIdx.x * ENC_BLOCK + threadIdx.x) >> 6; w * 64 * win < nn; w += n_waves) {
        const int64_t i0 = w * 64 * win;
        for (int l = lane; l < l_hi; l += 64) con[wv][l] = 0;
        DenseIn in, nx;
        float4 gq[NG], gn[NG];
        load(i0 + lane, in, gq);
        for (int k = 0; k < win && i0 + 64 * k < nn; ++k) {
            const bool more = k + 1 < win && i0 + 64 * (k + 1) < nn;
            if (more) load(i0 + 64 * (k + 1) + lane, nx, gn);  // in flight during this chunk's atomics
            const bool valid = in.valid;
            for (int l = 0; l < l_hi; ++l) {
                float g0 = 0.f, g1 = 0.f;
#pragma unroll
                for (int j = 0; j < NG; ++j) {  // uniform-index select of level l's pair
                    if (2 * j == l) { g0 = gq[j].x; g1 = gq[j].y; }
                    if (2 * j + 1 == l) { g0 = gq[j].z; g1 = gq[j].w; }
                }
                const float fs = fs_s[l];
                const LevelGeo Lg = level_geo(D.scale[l], in.px, in.py, in.pz);
                // dense index x + y res + z res^2 with corner_index's `% size`: corners of points in
                // [0,1]^3 stay below 2 size, where one conditional subtraction is that modulo
                const uint32_t res = D.res[l], size = D.size[l];
                int key[4], key1[4];
                bool far = false;
#pragma unroll
                for (int yz = 0; yz < 4; ++yz) {
                    const uint32_t gy = Lg.g[1] + (yz & 1), gz = Lg.g[2] + (yz >> 1);
                    const uint32_t k0 = Lg.g[0] + (gy + gz * res) * res, k1 = k0 + 1;
                    far |= valid && (k1 >= 2 * size || k1 < k0);
                    key[yz] = (int)(k0 >= size ? k0 - size : k0);
                    key1[yz] = (int)(k1 >= size ? k1 - size : k1);
                }
                if (__builtin_expect(__ballot(far) != 0, 0)) {  // points far outside the unit cube
#pragma unroll
                    for (int yz = 0; yz < 4; ++yz) {
                        const uint32_t gy = Lg.g[1] + (yz & 1), gz = Lg.g[2] + (yz >> 1);
                        key[yz] = (int)corner_index(D, l, Lg.g[0], gy, gz);
                        key1[yz] = (int)corner_index(D, l, Lg.g[0] + 1, gy, gz);
                    }
                }
                // the 16 contributions, each rounded once to the fixed-point unit
                int q[4][4];
                {
                    const float a0 = g0 * fs, a1 = g1 * fs;
                    const float w1 = Lg.w[0], w0 = 1.0f - Lg.w[0];
#pragma unroll
                    for (int yz = 0; yz < 4; ++yz) {
                        const float wy = (yz & 1) ? Lg.w[1] : 1.0f - Lg.w[1];
                        const float wz = (yz >> 1) ? Lg.w[2] : 1.0f - Lg.w[2];
                        const float wyz = wy * wz;
                        const float c0 = w0 * wyz, c1 = w1 * wyz;
                        q[yz][0] = valid ? (int)rintf(c0 * a0) : 0;
                        q[yz][1] = valid ? (int)rintf(c0 * a1) : 0;
                        q[yz][2] = valid ? (int)rintf(c1 * a0) : 0;
                        q[yz][3] = valid ? (int)rintf(c1 * a1) : 0;
                    }
                }
                // runs: consecutive samples in one cell (row 0's key identifies the cell)
                const int cell = valid ? key[0] : -1;
                // the run left open by the previous chunk: lane 0 continues it (its sums join lane
                // 0's values before the scan), or it is flushed as one more list entry
                const bool carried = con[wv][l] != 0;
                const bool cont = carried && lane == 0 && cell == ckey[wv][l][0].x;
                if (cont) {
#pragma unroll
                    for (int yz = 0; yz < 4; ++yz) {
                        const int4 c = csum[wv][l][yz];
                        q[yz][0] += c.x; q[yz][1] += c.y; q[yz][2] += c.z; q[yz][3] += c.w;
                    }
                }
                const bool flush = carried && !__shfl(cont ? 1 : 0, 0, 64);
                const int cp = __builtin_amdgcn_update_dpp(-2, cell, 0x138, 0xF, 0xF, false);  // wave_shr:1
                const int cn = __builtin_amdgcn_update_dpp(-2, cell, 0x130, 0xF, 0xF, false);  // wave_shl:1
                const bool head = valid && (lane == 0 || cp != cell);
                const bool tail = valid && (lane == 63 || cn != cell);
                // inclusive prefix sums over the wave (wraparound int32: differences are exact)
                int P[4][4];
#pragma unroll
                for (int yz = 0; yz < 4; ++yz)
#pragma unroll
                    for (int c = 0; c < 4; ++c) P[yz][c] = q[yz][c];
#define MFN_PSTEP(CTRL, RM)                                                                   \
    _Pragma("unroll") for (int yz = 0; yz < 4; ++yz)                                          \
        _Pragma("unroll") for (int c = 0; c < 4; ++c) P[yz][c] += dppz_i<CTRL, RM>(P[yz][c]);
                MFN_PSTEP(0x111, 0xF) MFN_PSTEP(0x112, 0xF) MFN_PSTEP(0x114, 0xF) MFN_PSTEP(0x118, 0xF)
                MFN_PSTEP(0x142, 0xA) MFN_PSTEP(0x143, 0xC)
#undef MFN_PSTEP
                // run index of each lane = heads at or before it - 1; tails write the inclusive
                // prefix and the keys
                const uint64_t hb = __ballot(head);
                const int nruns = __popcll(hb);
                const int run = __builtin_amdgcn_mbcnt_hi((uint32_t)(hb >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)hb, 0u)) + (head ? 0 : -1);
                if (tail) {
#pragma unroll
                    for (int yz = 0; yz < 4; ++yz) {
                        ltail[wv][run][yz] = make_int4(P[yz][0], P[yz][1], P[yz][2], P[yz][3]);
                        lkey[wv][run][yz] = make_int2(key[yz], key1[yz]);
                    }
                }
                long long* gt = reinterpret_cast<long long*>(priv) +
                                ((w & (GRAD_COPIES - 1)) * dense_entries + (int64_t)D.offset[l]);
                // one run's 16 sums, 8 lanes = (row, x-corner), both features packed in one 64-bit add
                auto issue = [&](int4 t, int2 kp, int c) {
                    const int f0 = c ? t.z : t.x, f1 = c ? t.w : t.y;
                    const long long pq = (long long)((uint64_t)(uint32_t)f1 << 32) + (long long)f0;
                    if (pq != 0)
                        __hip_atomic_fetch_add(gt + (c ? kp.y : kp.x), pq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                };
                // the run carried from the previous chunk that lane 0 did not continue: issued on its own
                if (flush && lane < 8) issue(csum[wv][l][(lane >> 1) & 3], ckey[wv][l][(lane >> 1) & 3], lane & 1);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                int nl = nruns;
                // the run at lane 63 stays open when the window's next chunk follows: carried (its
                // sums = its tail prefix minus the previous run's), and left out of this list
                con[wv][l] = 0;
                if (more && nruns > 0 && __shfl(tail ? 1 : 0, 63, 64)) {
                    const int r = nruns - 1;
                    if (lane < 4) {
                        const int4 t = ltail[wv][r][lane];
                        const int4 h = r > 0 ? ltail[wv][r - 1][lane] : make_int4(0, 0, 0, 0);
                        csum[wv][l][lane] = make_int4(t.x - h.x, t.y - h.y, t.z - h.z, t.w - h.w);
                        ckey[wv][l][lane] = lkey[wv][r][lane];
                    }
                    con[wv][l] = 1;
                    nl -= 1;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                for (int b = 0; b < nl; b += 8) {
                    const int r = b + (lane >> 3), yz = (lane >> 1) & 3;
                    if (r < nl) {
                        const int4 t = ltail[wv][r][yz];
                        const int4 h = r > 0 ? ltail[wv][r - 1][yz] : make_int4(0, 0, 0, 0);
                        issue(make_int4(t.x - h.x, t.y - h.y, t.z - h.z, t.w - h.w), lkey[wv][r][yz], lane & 1);
                    }
                }
                __builtin_amdgcn_wave_barrier();  // the list is rewritten by the next level
            }
            if (more) {
                in = nx;
#pragma unroll
                for (int j = 0; j < NG; ++j) gq[j] = gn[j];
            }
        }
    }
}

// grad[p] += sum_k priv[k][p]; priv[k][p] = 0 (ready for the next backward)
__global__ __launch_bounds__(256) void fold_copies_kernel(float* __restrict__ priv, int64_t n, float* __restrict__ grad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
        float4 acc = reinterpret_cast<float4*>(grad)[i];
#pragma unroll
        for (int k = 0; k < GRAD_COPIES; ++k) {
            float4* q = reinterpret_cast<float4*>(priv + k * n) + i;
            const float4 v = *q;
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            *q = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        reinterpret_cast<float4*>(grad)[i] = acc;
    }
}

// grid_bw_kernel over levels [0, l_end) (level_l1 NULL: float atomics)
void launch_grid_bw(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                    const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table, float* priv,
                    int64_t dense_entries, const float* level_l1, int l_end, int32_t* zero_flag,
                    mfnerf_stream_t stream) {
    const int64_t want = div_up<int64_t>(div_up<int64_t>(n, 16), ENC_BLOCK / 64);
    const int64_t cap = grid_bw_block_cap();
    const int64_t blocks = want < cap ? want : cap;
    const bool big = desc->n_levels > 16;
    auto kern = level_l1 ? (big ? grid_bw_kernel<MFN_MAX_LEVELS, true> : grid_bw_kernel<16, true>)
                         : (big ? grid_bw_kernel<MFN_MAX_LEVELS, false> : grid_bw_kernel<16, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(ENC_BLOCK), 0, stream, x, n, n_dev, x_min, x_range, *desc,
                       dL_dout, grad_table, priv, dense_entries, level_l1, l_end, zero_flag);
}

}  // namespace

namespace mfn_grid {

bool launch_dense_levels(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                         const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table, float* priv,
                         const float* level_l1, int l_first, int32_t* zero_flag, int32_t* gate,
                         mfnerf_stream_t stream) {
    const int64_t de = dense_entries_of(desc);
    int n_dense_levels = 0;  // leading levels that are dense own tables inside the private copies
    while (n_dense_levels < desc->n_levels && desc->table_kind[n_dense_levels] == 0 &&
           (int64_t)desc->offset[n_dense_levels] + desc->size[n_dense_levels] <= de)
        ++n_dense_levels;
    if (l_first > n_dense_levels) {  // request-shaped atomics, private copies
        launch_grid_bw(x, n, n_dev, x_min, x_range, desc, dL_dout, grad_table, priv, de, level_l1, l_first, zero_flag,
                       stream);
        return false;
    }
    // levels [0, l_first) all dense: one sample per lane, packed 64-bit adds into the copies
    // DENSE_WAVES waves at most (the kernel's window spreads any sample count over them)
    const int64_t wb = std::min<int64_t>(div_up<int64_t>(n, (int64_t)64 * (ENC_BLOCK / 64)),
                                    div_up<int64_t>(DENSE_WAVES, ENC_BLOCK / 64));
    const int64_t cap = grid_bw_block_cap();
    auto dk = l_first <= 8 ? grid_bw_dense_kernel<4> : l_first <= 16 ? grid_bw_dense_kernel<8> : grid_bw_dense_kernel<16>;
    hipLaunchKernelGGL(dk, dim3((unsigned)(wb < cap ? wb : cap)), dim3(ENC_BLOCK), 0, stream, x, n, n_dev, x_min,
                       x_range, *desc, dL_dout, priv, de, level_l1, l_first, zero_flag, gate);
    return true;
}

}  // namespace mfn_grid

extern "C" {

int64_t mfnerf_grid_encode_bw_workspace(const mfnerf_grid_desc* desc) {
    if (check_desc(desc, "grid_encode_bw_workspace")) return -1;
    return (int64_t)GRAD_COPIES * dense_entries_of(desc) * 2 * (int64_t)sizeof(float);
}

int mfnerf_grid_encode_bw_scatter(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                  const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                  void* workspace, const float* level_l1, mfnerf_stream_t stream) {
    int st = check_desc(desc, "grid_encode_bw");
    if (st) return st;
    if (n < 0) { mfn_set_error("grid_encode_bw: bad size"); return MFN_ERR_INVALID; }
    if (n == 0) return MFN_OK;
    if (!x || !dL_dout || !grad_table) { mfn_set_error("grid_encode_bw: null pointer"); return MFN_ERR_INVALID; }
    launch_grid_bw(x, n, n_dev, x_min, x_range, desc, dL_dout, grad_table, (float*)workspace,
                   workspace ? dense_entries_of(desc) : 0, level_l1, desc->n_levels, nullptr, stream);
    return mfn_check_launch("grid_encode_bw_scatter");
}

int mfnerf_grid_encode_bw_finish(const mfnerf_grid_desc* desc, float* grad_table, void* workspace,
                                 const float* level_l1, mfnerf_stream_t stream) {
    int st = check_desc(desc, "grid_encode_bw_finish");
    if (st) return st;
    if (!grad_table) { mfn_set_error("grid_encode_bw_finish: null pointer"); return MFN_ERR_INVALID; }
    const int64_t dense = workspace ? dense_entries_of(desc) : 0;
    if (level_l1) {
        launch_fold_convert(grad_table, (int*)workspace, 2 * dense, table_values_of(desc), desc, level_l1, nullptr, 0,
                            0, 0, stream);
    } else if (dense > 0) {
        const int64_t nf = 2 * dense;  // multiple of 16 (level sizes are multiples of 8)
        const int64_t fb = div_up<int64_t>(nf / 4, 256);
        hipLaunchKernelGGL(fold_copies_kernel, dim3((unsigned)(fb < 2048 ? fb : 2048)), dim3(256), 0, stream,
                           (float*)workspace, nf, grad_table);
    }
    return mfn_check_launch("grid_encode_bw_finish");
}

int mfnerf_grid_encode_bw(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                          const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table, void* workspace,
                          const float* level_l1, mfnerf_stream_t stream) {
    if (n == 0) return MFN_OK;  // (n < 0: the scatter's error)
    int st = mfnerf_grid_encode_bw_scatter(x, n, n_dev, x_min, x_range, desc, dL_dout, grad_table, workspace,
                                           level_l1, stream);
    if (st) return st;
    return mfnerf_grid_encode_bw_finish(desc, grad_table, workspace, level_l1, stream);
}

// Per-level L1 norm of dL/dout (n, L*F) f32: out[l] += sum_i |dy[i][2l]| + |dy[i][2l+1]| (the bound
// the fixed-point backward sizes its scales with, when the producer does not supply it).
__global__ __launch_bounds__(256) void level_l1_kernel(const float* __restrict__ dy, int64_t n,
                                                       const int32_t* __restrict__ n_dev, int L,
                                                       float* __restrict__ out) {
    __shared__ float part[MFN_MAX_LEVELS];
    if (threadIdx.x < L) part[threadIdx.x] = 0.0f;
    __syncthreads();
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int row = 2 * L;
    // flat (row, level) pairs f = t + k*S over the grid's first S = floor(threads / L) * L threads:
    // S is a multiple of L, so thread t always sees level l = t % L (any L, not only divisors of 64)
    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t S = ((int64_t)gridDim.x * blockDim.x / L) * L;
    const int l = (int)(gt % L);
    float acc = 0.0f;
    if (gt < S)
        for (int64_t f = gt; f < nn * L; f += S) {
            const float2 v = *reinterpret_cast<const float2*>(dy + (f / L) * row + 2 * l);
            acc += fabsf(v.x) + fabsf(v.y);
        }
    if (64 % L == 0 && (blockDim.x % L) == 0) {
        // L divides the wave and the block: lanes l, l+L, ... of a wave share level l (block-local
        // lane index = global index mod L); reduce inside the wave first
        for (int off = 32; off >= L; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if ((threadIdx.x & 63) < L) atomicAdd(&part[l], acc);
    } else if (gt < S) {
        atomicAdd(&part[l], acc);
    }
    __syncthreads();
    if (threadIdx.x < L) atomicAdd(out + threadIdx.x, part[threadIdx.x]);
}

int mfnerf_grid_level_l1(const float* dL_dout, int64_t n, const int32_t* n_dev, int n_levels, float* out,
                         mfnerf_stream_t stream) {
    if (n < 0 || n_levels <= 0 || n_levels > MFN_MAX_LEVELS || !out || (n > 0 && !dL_dout)) {
        mfn_set_error("grid_level_l1: bad arguments"); return MFN_ERR_INVALID;
    }
    if (n == 0) return MFN_OK;
    // one workgroup per CU at most: the 16 per-level sums are atomics on 16 addresses, which
    // serialise at the memory side -- 2048 workgroups made this 36 us, most of it in that tail
    const int64_t want = div_up<int64_t>(n * n_levels, 256 * 16);
    hipLaunchKernelGGL(level_l1_kernel, dim3((unsigned)(want < 256 ? (want < 1 ? 1 : want) : 256)), dim3(256), 0,
                       stream, dL_dout, n, n_dev, n_levels, out);
    return mfn_check_launch("grid_level_l1");
}

}  // extern "C"
