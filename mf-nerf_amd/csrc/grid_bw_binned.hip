// grid_bw_binned.hip -- the partitioned ("binned") hash-grid table gradient: the plan of a layout's
// partitions, the scatter of 8-B records into them, the accumulate with its fused Adam update, and
// every mfnerf_grid_encode_bw_binned* and mfnerf_adam_step_fixed* entry point.  Two parts of this
// translation unit have files of their own: the record format (grid_records.hpp) and the convert /
// Adam kernels on the fixed-point sums (grid_adam_fixed.hpp).
#include <type_traits>
#include <utility>

#include "grid_internal.hpp"
#include "grid_adam_fixed.hpp"
#include "grid_records.hpp"

using namespace mfn;
using namespace mfn_grid;

namespace {

// Partitioned table-gradient scatter ("binned").  The hashed levels' tables are small (2^19 entries
// = 4 MB of int32 pairs per level at the Lego config) and uniformly hit: every 64-B line receives
// ~30 adds per step from unrelated rays, so no ordering of the samples lets memory-side atomics
// merge them (tools/sim_scatter_requests.py: >= 3 requests per sample per fine level in any window
// of a Morton-sorted batch, 0.13 distinct lines per sample over the whole batch).  Instead each
// table is cut into 2^shift-entry partitions, every (sample, level, (y,z) corner row) becomes an
// 8-B record (entry, x weight, both features' values in fp16: the algorithmic fp16 scatter's own
// payload) routed to its partition by a counting sort, and one workgroup per partition sums its
// records into an LDS image with integer LDS atomics (ds_add_u32: ~4 T adds/s chip-wide at random
// addresses, tools/lds_atomic_probe.hip -- 20x ds_add_f32), then stores the image once.  The image
// holds one 64-bit word per entry: both features' sums in the table's int32 fixed-point unit,
// packed f1 * 2^32 + f0 (exact in two's complement, order-free: bit-reproducible), each weighted
// contribution rounded once to the unit -- 2 LDS atomics per pair record (an int64 image per
// feature at 2^32 x the unit, 4 atomics and a float -> int64 conversion per record, measured 349 vs
// 316 us for the whole scatter in round 2).  Passes: scatter (records into fixed per-(partition,
// unit) slots) -> accumulate (one workgroup per partition).
// partitions of 2^shift entries, shift in [MIN_BIN_SHIFT, MAX_BIN_SHIFT] chosen per layout so that
// there are >= ~1024 partitions (4 workgroups per CU); 2^11 entries = 16 KB of packed int32 pairs
constexpr int MIN_BIN_SHIFT = 8, MAX_BIN_SHIFT = 11, MAX_BIN_ENTRIES = 1 << MAX_BIN_SHIFT;
// partitions over all binned tables: the first LDS_CURSOR keep the scatter unit's running counts in
// LDS, the rest (own tables of 2^20-2^21 entries: --T 20/21, opt.py:78) in the unit's column of the
// slot counts in global memory, read and written by the one scanning wave (LDS for all 5120 of the
// T 2^20 layout measured the same: 0.654 vs 0.654 ms/step, r05_v27)
constexpr int LDS_CURSOR = 4096, MAX_BINS = 16384;

// Records live in fixed slots: unit u's records of bin b at rec[(b * UNITS + u) * slot + k],
// k < scnt[b * UNITS + u] -- no counting pass, no scan.  slot = 3 x the mean records per slot at this
// step's live count + 96, so the buffer (sized for the largest live count) holds them; the records
// of a slot that still overflows (a sample distribution far from uniform) go into the table by
// atomics (overflow_add), and `ovf` tells the accumulate to add them to its image.
constexpr int UNITS = 256;       // scatter workgroups, each owning a contiguous sample range
constexpr int MAX_TBINS = 1024;  // bins of one table
constexpr int SC_STAGE = SC_THREADS * 8;  // staged records per tile (8 per thread)

// records per (partition, unit) slot at live count nn; non-decreasing in nn, so the workspace sized
// with slot_size(n_max) (binned_workspace_layout) holds every slot of any nn <= n_max
__host__ __device__ __forceinline__ int64_t slot_size(int64_t nn, const BinPlan& P) {
    const int64_t recs = nn * P.n_binned * (P.pair_ok ? 4 : 8);
    const int64_t s = 3 * ((recs + (int64_t)P.n_bins * UNITS - 1) / ((int64_t)P.n_bins * UNITS)) + 96;
    return (s + 15) / 16 * 16;  // 16 records = 128 B: every slot starts on a 128-B line
}

// A record past its slot's capacity (a sample distribution far from uniform over the partitions):
// added by 64-bit packed integer atomics (f1 * 2^32 + f0 per entry, each contribution rounded once
// to the table's int32 unit) into the workspace's overflow words (one per partitioned entry, zero
// between steps: the accumulate zeroes what it reads), and the accumulate adds the partition's words
// to its image (bin_scatter raises ovf).  Exact integer sums: the order of the two paths does not
// matter.  The words are not the gradient's own, so the gradient need not be zero before a scatter.
__device__ __forceinline__ void overflow_add(const BinPlan& P, int* __restrict__ ovw, int bin, uint2 r) {
    const int t = bin_table(P, bin);
    const int64_t base = (int64_t)(P.t_offset[t] - P.t_offset[0]) + ((int64_t)(bin - P.t_bin0[t]) << P.shift);
    const uint32_t w = r.x;
    const float a = rec_value(r.y, 0) * REC_UP, b = rec_value(r.y, 1) * REC_UP;
    const float fx = (float)(w >> 17) * (1.0f / 32768.0f);
    const int e0 = w & ((1 << P.shift) - 1);
    auto add = [&](int e, float wt) {
        const int q0 = (int)rintf(wt * a), q1 = (int)rintf(wt * b);
        const long long pq = (long long)((uint64_t)(uint32_t)q1 << 32) + (long long)q0;
        if (pq != 0)
            __hip_atomic_fetch_add(reinterpret_cast<long long*>(ovw) + base + e, pq, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    };
    if (w & (1u << 15)) {
        add(e0, (w & (1u << 16)) ? fx : 1.0f - fx);
    } else {
        add(e0, 1.0f - fx);
        add(e0 ^ (((2 << ((w >> 11) & 15)) - 1) << ((w >> 16) & 1)), fx);
    }
}

// pass 1: unit u (one 1024-thread workgroup) walks its samples, staged in registers, level by level
// in tiles of up to 2048 samples.  Per level, ONE pass computes the tile's records into registers
// (8 per thread: 2 samples x 4 pair rows, or 1 sample x 8 single records), each taking its rank in
// its bin from an LDS counter; one wave scans the bin counts; the records are placed sorted by bin
// into an LDS stage; the stage is stored as one contiguous run per bin into the unit's slot of the
// bin (~30 records per run at the Lego config: whole-line stores) while the NEXT level counts.
struct BinRec {
    uint2 r;
    uint32_t meta;  // bin in the table (bits 0-15) | rank in the bin's run (bits 16-31); ~0u: none
};

// f(integral_constant<int, 0>), ..., f(integral_constant<int, N - 1>)
template <typename F, int... J>
__device__ __forceinline__ void static_for_impl(F& f, std::integer_sequence<int, J...>) {
    (f(std::integral_constant<int, J>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

template <int MAXB, bool PAIR>
__global__ __launch_bounds__(SC_THREADS) void bin_scatter_kernel(const float* __restrict__ X, int64_t n,
                                                                 const int32_t* __restrict__ n_dev, float x_min,
                                                                 float x_range, const mfnerf_grid_desc D,
                                                                 const BinPlan P, const float* __restrict__ dy,
                                                                 const float* __restrict__ level_l1,
                                                                 uint2* __restrict__ rec, int32_t* __restrict__ scnt,
                                                                 uint32_t* __restrict__ smax,
                                                                 int32_t* __restrict__ ovf, int64_t n_slots,
                                                                 int* __restrict__ ovw) {
    constexpr int SPT = PAIR ? 2 : 1;  // samples per thread per tile
    constexpr int TH = SC_THREADS, STG = SC_STAGE, LCUR = LDS_CURSOR;
    const int u = blockIdx.x;
    __shared__ int cursor[LCUR];  // the unit's running count per bin
    // per-level bin counts, double-buffered by level parity (a level's counts are read by the scan
    // and cleared during its placement, while the next level counts into the other buffer)
    __shared__ int hist2[2][MAX_TBINS], toff[MAX_TBINS];
    // per bin of the staged level: {index of the stage's first record of the bin in rec[] minus its
    // stage offset, the stage index its slot ends at} (one 8-B LDS read per stored record)
    __shared__ int2 gdst[2][MAX_TBINS];
    __shared__ uint2 stage[STG];
    __shared__ uint16_t sbin[STG];
    __shared__ float fs_s[MFN_MAX_LEVELS];
    __shared__ int s_total[2];
    uint32_t rmax2 = 0u;  // largest |a| (low half), |b| (high half) of this thread's records, fp16 bits
    load_fixed_scales(D, level_l1, fs_s);
    for (int b = threadIdx.x; b < min(P.n_bins, LCUR); b += blockDim.x) cursor[b] = 0;
    // the running counts of the bins past LCUR live in scnt: zeroed by the scanning wave, the only
    // one that touches them (program order within the wave)
    if (threadIdx.x < 64)
        for (int b = LCUR + (int)threadIdx.x; b < P.n_bins; b += 64) scnt[(int64_t)b * UNITS + u] = 0;
    for (int b = threadIdx.x; b < 2 * MAX_TBINS; b += blockDim.x) hist2[b >> 10][b & (MAX_TBINS - 1)] = 0;
    if (threadIdx.x < 2) s_total[threadIdx.x] = 0;
    __syncthreads();
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    // slots sized for at most the workspace's count: beyond it a slot may overflow (-> atomics)
    const int64_t slot = slot_size(min(nn, n_slots), P);
    // unit u owns the 16-sample chunks u, u + UNITS, u + 2 UNITS, ...: a ray's samples (which repeat
    // the coarse levels' rows) spread over many units, so every slot fills close to the mean
    const int64_t n_chunks = (nn + 15) / 16;
    const int64_t m = n_chunks > u ? ((n_chunks - 1 - u) / UNITS + 1) * 16 : 0;  // this unit's sample slots
    // Round 5: two barriers per level instead of three.  Phase A places level j's ranked records into
    // the stage and then counts level j + 1 (the next tile's first level after the last); phase B
    // stores level j's stage into the slots and scans level j + 1's bin counts.  Each LDS buffer is
    // written and read in different phases: the stage (A: place, B: store), toff (B: scan, A: place),
    // hist2 / gdst / s_total by level parity (count and scan of j + 1 beside place and store of j).
    int par = 0;  // parity of the level whose records R holds (its hist2 / gdst / s_total buffers)
    BinRec R[8];
    StagedSample<MAXB> S[SPT];
    bool live[SPT];
    auto stage_tile = [&](int64_t base) {
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const int64_t k = base + (int64_t)q * TH + threadIdx.x;
            const int64_t i = ((k >> 4) * UNITS + u) * 16 + (k & 15);  // chunk k/16 of the unit
            live[q] = k < m && i < nn;
            if (live[q]) stage_sample(D, P, X, x_min, x_range, dy, i, S[q]);
        }
    };
    // count: level j's records computed once each, ranked in their bin by the LDS counter of parity cp;
    // G(q) = sample q's dL/dy pair at level j
    auto count = [&](int j, int cp, auto G) __attribute__((always_inline)) {
        const int b0 = P.t_bin0[P.table_of[P.level[j]]];
#pragma unroll
        for (int k = 0; k < 8; ++k) R[k].meta = ~0u;
#pragma unroll
        for (int q = 0; q < SPT; ++q) {
            const SampleLevel Q = G(q);
            // the record's |a|, |b| maxima as two packed u16 (fp16 bits order like the values)
            auto rank = [&](int k, int lb, uint2 r) {
                R[k].r = r;
                R[k].meta = (uint32_t)lb | ((uint32_t)atomicAdd(&hist2[cp][lb], 1) << 16);
                rmax2 = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(
                    __builtin_bit_cast(ushort2v, rmax2), __builtin_bit_cast(ushort2v, r.y & 0x7fff7fffu)));
            };
            if constexpr (!PAIR) {
                if (P.merge[P.level[j]]) {  // (uniform) every lane takes part: DPP over the row
                    merged_level_records(D, P, j, S[q].x, S[q].y, S[q].z, Q.g0, Q.g1, fs_s[P.level[j]],
                                         live[q] && Q.live, [&](int sl, int bin, uint2 r) { rank(sl, bin - b0, r); });
                    continue;
                }
            }
            if (!(live[q] && Q.live)) continue;
            if constexpr (PAIR) {
                const int l = P.level[j];
                const float fs = fs_s[l] * REC_DOWN;
                pair_level_records(D, P, l, S[q].x, S[q].y, S[q].z, Q.g0 * fs, Q.g1 * fs,
                                   [&](int yz, int lb, uint2 r) { rank(4 * q + yz, lb, r); });
            } else {
                level_records(D, P, j, S[q].x, S[q].y, S[q].z, Q.g0, Q.g1, fs_s[P.level[j]],
                              [&](int sl, int bin, uint2 r) {
                                  if (bin >= 0) rank(sl, bin - b0, r);
                              });
            }
        }
    };
    // scan: level j's bins -> sorted tile offsets (toff) and slot places (gdst[cp]); a run's k-th
    // record goes to slot position gdst + k.  Chunk q of 64 bins (consecutive lanes on consecutive LDS
    // words: no bank conflicts) is scanned by wave q % 16 with an integer DPP wave scan; its carry (the
    // bins of the chunks before it) is each lane's column sum over those chunks
    auto scan = [&](int j, int cp) {
        static_assert(MAX_TBINS == 1024, "hist2 indexing");
        const int t = P.table_of[P.level[j]];
        const int b0 = P.t_bin0[t], tb = P.t_bin0[t + 1] - b0;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int per = (tb + 63) >> 6;
        const int* hs = hist2[cp];
        constexpr int nw = SC_THREADS / 64;
        for (int q = wv; q < per; q += nw) {
            int col = 0;  // chunks before q are whole (q < per - 1 ... < tb)
            for (int q2 = 0; q2 < q; ++q2) col += hs[q2 * 64 + lane];
            col += dppz_i<0x111, 0xF>(col); col += dppz_i<0x112, 0xF>(col);
            col += dppz_i<0x114, 0xF>(col); col += dppz_i<0x118, 0xF>(col);
            col += dppz_i<0x142, 0xA>(col); col += dppz_i<0x143, 0xC>(col);
            const int carry = __builtin_amdgcn_readlane(col, 63);
            const int lb = q * 64 + lane;
            const int c = lb < tb ? hs[lb] : 0;
            int x = c;
            x += dppz_i<0x111, 0xF>(x); x += dppz_i<0x112, 0xF>(x);
            x += dppz_i<0x114, 0xF>(x); x += dppz_i<0x118, 0xF>(x);
            x += dppz_i<0x142, 0xA>(x); x += dppz_i<0x143, 0xC>(x);
            const int run = carry + x - c;
            if (lb < tb) {
                toff[lb] = run;
                const int gb = b0 + lb, cl = gb;
                int32_t* gc = scnt + (int64_t)gb * UNITS + u;  // (bins past LCUR)
                const int cu = cl < LCUR ? cursor[cl] : *gc;
                // record k of the sorted stage is position cu - run + k of the slot
                gdst[cp][lb] = make_int2((int)((uint32_t)(b0 + lb) * UNITS + u) * (int)slot + cu - run,
                                         run + (int)slot - cu);
                if (cl < LCUR) cursor[cl] = cu + c;
                else *gc = cu + c;
            }
            if (q == per - 1 && lane == 63) s_total[cp] = carry + x;
        }
    };
    // place: level j's records (R, parity par) sorted by bin into the stage; its counts cleared for the
    // level after next, which counts into the same buffer
    auto place = [&](int j) {
        const int t = P.table_of[P.level[j]];
        const int tb = P.t_bin0[t + 1] - P.t_bin0[t];
        for (int b = threadIdx.x; b < tb; b += TH) hist2[par][b] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (R[k].meta == ~0u) continue;
            const int lb = R[k].meta & 0xffff;
            const int p = toff[lb] + (int)(R[k].meta >> 16);
            stage[p] = R[k].r;
            sbin[p] = (uint16_t)lb;
        }
    };
    // store: level j's sorted stage as one contiguous run per bin into the unit's slot of the bin
    auto store = [&](int j) {
        const int b0 = P.t_bin0[P.table_of[P.level[j]]];
        const int total = s_total[par];
        const int2* gd = gdst[par];
        // SU records per thread in flight: their stage / bin reads, then their slot places, then the
        // stores -- two LDS round trips per SU records (round 6: one record per iteration waited three
        // times; the phase probe puts ~1/3 of the Lego scatter's time in this phase).  Measured
        // (r6ab / r6ac, profiles/r06_v9_scatter_phase_probe.txt): the Lego scatter alone 0.2425 ->
        // 0.238 ms at SU = 2, the step within noise (0.4881 vs 0.4892); SU = 4 made the Lego kernel
        // 124 VGPRs -- no room left beside it for the side stream's march -- and the step 4 us slower;
        // reading place()'s eight offsets before its writes gained nothing
        constexpr int SU = PAIR ? (MAXB <= 12 ? 2 : 1) : 4;
        for (int k0 = threadIdx.x; k0 < total; k0 += SU * TH) {
            int lb[SU];
            uint2 r[SU];
            int2 g[SU];
#pragma unroll
            for (int q = 0; q < SU; ++q) {
                const int k = k0 + q * TH, kc = k < total ? k : 0;
                lb[q] = sbin[kc];
                r[q] = stage[kc];
            }
#pragma unroll
            for (int q = 0; q < SU; ++q) g[q] = gd[lb[q]];
#pragma unroll
            for (int q = 0; q < SU; ++q) {
                const int k = k0 + q * TH;
                if (k >= total) break;
                if (k < g[q].y) {  // inside the unit's slot of the bin
                    // a plain store (round 5, r5c: the nontemporal store this was made the scatter 92 instead
                    // of 82.5 us and the step 3 us slower; the accumulate reads them the same either way)
                    rec[(uint32_t)(g[q].x + k)] = r[q];
                } else {
                    overflow_add(P, ovw, b0 + lb[q], r[q]);  // a full slot: into the overflow words
                }
            }
        }
    };
    // one level step: phase A (place j, count the next level), phase B (store j, scan the next level)
    auto step = [&](int j, int64_t base, auto count_next) __attribute__((always_inline)) {
        place(j);
        int jn = j + 1;
        bool next = true;
        if (jn == P.n_binned) {  // the next tile's first level
            jn = 0;
            next = base + (int64_t)SPT * TH < m;
            // (the single-record layout stages it below, a step earlier)
            if (next && (PAIR || P.n_binned < 2)) stage_tile(base + (int64_t)SPT * TH);
        }
        if (next) count_next(jn, par ^ 1);  // (`next`, jn: uniform -- count() must stay wave-uniform)
        __syncthreads();
        // single-record layout (MixedFeature): the next tile's samples, loaded as soon as this tile's
        // last level is counted (phase A above) and ahead of this phase's record stores -- on gfx9 a
        // load's wait counts the stores issued before it too, and staged right before its first
        // count the load waited for the previous phase's stores and then its own round trip
        // (profiles/r06_v9_scatter_phase_probe.txt: that count 3x the others; config 3's step 1.151
        // -> 1.138 ms, r6v).  The PAIR kernels keep the late staging: the Lego layout's units hold
        // one tile, and the early form's code alone made its scatter 7 us slower (r6v)
        if constexpr (!PAIR)
            if (j == P.n_binned - 2 && base + (int64_t)SPT * TH < m) stage_tile(base + (int64_t)SPT * TH);
        store(j);
        if (next) scan(jn, par ^ 1);
        __syncthreads();
        par ^= 1;
    };
    auto level_g = [&](int j) {  // runtime-level dL/dy pair (sample_level's register select)
        return [&, j](int q) { return sample_level(D, P, S[q], j); };
    };
    if (m > 0) {  // the first tile's first level: count, scan
        stage_tile(0);
        count(0, 0, level_g(0));  // under `m > 0`, uniform: count() must stay wave-uniform (run_row's DPP)
        __syncthreads();
        scan(0, 0);
        __syncthreads();
    }
    for (int64_t base = 0; base < m; base += (int64_t)SPT * TH) {
        if constexpr (PAIR && MAXB <= 10) {
            // the level loop written out: j a constant in every copy, so the staged pair is a plain
            // register (sample_level's select costs 2 MAXB v_cndmask per sample and level).  The
            // single-record layout (MixedFeature) written out the same way: 331 vs 325 us, code
            // 91 vs 24 KB (r05_v25)
            auto count_c = [&](int jn, int cp) __attribute__((always_inline)) {
                auto each = [&](auto jc) __attribute__((always_inline)) {
                    constexpr int jj = decltype(jc)::value;
                    if (jj == jn)  // (uniform: count() must stay wave-uniform)
                        count(jj, cp, [&](int q) {
                            SampleLevel r;
                            r.g0 = S[q].g[2 * jj];
                            r.g1 = S[q].g[2 * jj + 1];
                            r.live = !(r.g0 == 0.0f && r.g1 == 0.0f);
                            return r;
                        });
                };
                static_for<MAXB>(each);
            };
            for (int j = 0; j < P.n_binned; ++j) step(j, base, count_c);
        } else {
            for (int j = 0; j < P.n_binned; ++j)
                step(j, base, [&](int jn, int cp) { count(jn, cp, level_g(jn)); });  // (count(): wave-uniform)
        }
    }
    // the unit's largest contribution (one word per unit: the accumulate's per-partition bound is
    // sum over units of count x this max)
    {
        __shared__ uint32_t wmax[TH / 64];
        uint32_t rmax = max(rmax2 & 0xffffu, rmax2 >> 16);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) rmax = max(rmax, (uint32_t)__shfl_xor((int)rmax, off, 64));
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = rmax;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t mx = 0u;
            for (int k = 0; k < TH / 64; ++k) mx = max(mx, wmax[k]);
            smax[u] = __float_as_uint(rec_value(mx, 0) * REC_UP);  // as a float in table units
        }
    }
    // ovf[0]: this step's overflowed records (the accumulate adds the gradient words when non-zero;
    // zeroed by the next step's first scatter launch); ovf[1]: their running total (never reset by
    // the kernels: mfnerf_grid_encode_bw_binned_flag_offset + 4 bytes, read by the training tools)
    int over = 0;
    for (int b = threadIdx.x; b < min(P.n_bins, LCUR); b += blockDim.x) {
        const int c = cursor[b];
        over += c > slot ? (int)(c - slot) : 0;
        scnt[(int64_t)b * UNITS + u] = c;
    }
    if (threadIdx.x < 64)  // the counts past LCUR: already in scnt, read back by the wave that wrote them
        for (int b = LCUR + (int)threadIdx.x; b < P.n_bins; b += 64) {
            const int c = scnt[(int64_t)b * UNITS + u];
            over += c > slot ? (int)(c - slot) : 0;
        }
    if (over) {
        atomicAdd(ovf, over);
        atomicAdd(ovf + 1, over);
    }
}

// pass 2: one workgroup per partition sums the partition's records (every unit's slot) into an LDS
// image of its entries and stores it (or feeds it to the fused Adam update).
//
// The image holds one 64-bit word per entry: both features' int32 sums packed as f1 * 2^32 + f0
// (exact in two's complement; decoded f0 = lo, f1 = hi + (f0 < 0)), 2 LDS atomics per pair record.
// The sums run at the PARTITION's own finer unit 2^-k of the table's: k is the largest with
// (sum over units of the unit's record count in the partition x the unit's largest |a|, |b|) * 2^k
// <= 2^30 -- a bound on every entry's sum, from bin_scatter's counts and maxima -- so the int32
// fields cannot overflow, and the stored table-unit value is rounded once per entry.
// The partition's LDS image: both features' int32 sums of an entry as one packed 64-bit word
// (f1 * 2^32 + f0, one ds_add_u64 per entry; decoded f0 = lo, f1 = hi + (f0 < 0)).  Round 6 measured
// the two-plane form (one ds_add_u32 per feature, the review's suggestion): bank conflicts 49 -> 54 %
// of the LDS-active cycles (a 32-bit add's 32-lane group on 32 banks conflicts as randomly as a
// 64-bit add's 16-lane group on 16 bank pairs, and there are twice as many adds), LDS cycles per
// instruction 6.4 -> 5.4, the step unchanged (0.5017 / 0.5007 vs 0.5003 / 0.4995 ms,
// profiles/r06_v1_pmc_sq_grid_bw*.txt).
struct AccImage {
    unsigned long long w[MAX_BIN_ENTRIES];
    __device__ __forceinline__ void add(int e, int q0, int q1) {
        atomicAdd(&w[e], ((unsigned long long)(uint32_t)q1 << 32) + (unsigned long long)(long long)q0);
    }
    __device__ __forceinline__ int2 get(int i) const {
        const unsigned long long v = w[i];
        const int lo = (int)(uint32_t)v;
        return make_int2(lo, (int)(uint32_t)(v >> 32) + (lo < 0));
    }
    __device__ __forceinline__ void set(int i, int2 v) {
        w[i] = ((unsigned long long)(uint32_t)v.y << 32) + (unsigned long long)(long long)v.x;
    }
};
__device__ __forceinline__ void accum_record(AccImage& img, int mask, uint2 r, float k2) {
    const uint32_t w = r.x;
    const float a = rec_value(r.y, 0) * k2, b = rec_value(r.y, 1) * k2;  // exact: k2 a power of two
    if (a == 0.0f && b == 0.0f) return;
    const float fx = (float)(w >> 17) * (1.0f / 32768.0f);
    const int e0 = w & mask;
    if (w & (1u << 15)) {  // single entry, weight sel ? fx : 1 - fx
        const float wt = (w & (1u << 16)) ? fx : 1.0f - fx;
        img.add(e0, (int)rintf(wt * a), (int)rintf(wt * b));
    } else {
        const int e1 = e0 ^ (((2 << ((w >> 11) & 15)) - 1) << ((w >> 16) & 1));
        const float w0 = 1.0f - fx;
        img.add(e0, (int)rintf(w0 * a), (int)rintf(w0 * b));
        img.add(e1, (int)rintf(fx * a), (int)rintf(fx * b));
    }
}

constexpr int ACC_THREADS = 512;
static_assert(MAX_BIN_ENTRIES % ACC_THREADS == 0, "the fused Adam's per-thread entries");

struct AdamRest {
    float* g;            // the flat gradient (MLP floats, then the table's int32 sums)
    int* priv;           // the dense levels' private copies
    int64_t dense_vals, total_vals, end4;
    int n_blocks;        // 0: none
    int first;           // 1: the grid's first n_blocks workgroups (dispatched early), 0: its last
    int32_t* gate;       // opened as the dense-level launch starts (NULL: none)
};

// Round 5: the partition's records are routed through an LDS stage by LDS-DMA
// (global_load_lds_dword), so that a workgroup has ALL its record loads in flight at once:
// (1) the 256 slot counts (and the fused Adam's optimizer state of this thread's entries) are
// loaded; (2) an exclusive prefix of the counts gives every slot's place in a compacted stage; (3)
// wave w copies slots w, w + 8, ... into the stage, 32 records (64 lanes x 4 B) per DMA instruction,
// with no register destination -- one round trip for the whole partition; (4) the adds read the
// stage in a strided order (record 37 t mod 512 of each 512-record block for thread t) so one LDS
// instruction's lanes hold records ~37 apart -- different slots, i.e. different rays -- instead of a
// ray's run of consecutive samples in one cell (same-address atomics).  A partition holding more
// records than the stage is done in chunks of ACC_RB records.  Same records, same integer adds:
// bit-identical sums.  LDS: 16 KB image + 32 KB stage -> three workgroups per CU.
// records per stage chunk.  Round 5: 3840 (30 KB), three workgroups per CU (r05_v21: the unfused accumulate 91.2 -> 88.3 us,
// grid_bw by events 0.239 -> 0.2366 ms; with the Adam fused 142.9 vs 142.5 us; 2560 records: slower)
// Round 6 (r6ai, profiles/r06_v10_accum_probe.txt): 4096 records (32 KB, still three workgroups per
// CU) 0.4885 vs 0.4924 ms/step at Lego, whose partitions hold ~7.7 k records -- two chunks more often
// than at 3840; 4608 (36 KB) left room for only two workgroups per CU: 0.500
constexpr int ACC_RB = 4096;
struct AccumStage {
    AccImage img;
    uint2 recs[ACC_RB];
    int pre[UNITS + 1];  // exclusive prefix of the slots' record counts; pre[UNITS] = the partition's
    float wsum[ACC_THREADS / 64];
    int wtot[ACC_THREADS / 64];
};
union AccumShared {  // ONE __shared__ object (a second one beside an LDS-DMA stage can cost waits)
    AccumStage a;
    TableRegions tr;
};
static_assert(sizeof(AccumShared) <= 163840 / 3, "three accumulate workgroups per CU");

template <bool FUSED>  // FUSED: the Adam update from the finished sums (A.params != NULL)
__global__ __launch_bounds__(ACC_THREADS) void bin_accum_kernel(const BinPlan P, int64_t n,
                                                                const int32_t* __restrict__ n_dev,
                                                                const uint2* __restrict__ rec,
                                                                const int32_t* __restrict__ scnt,
                                                                const uint32_t* __restrict__ smax,
                                                                const int32_t* __restrict__ ovf,
                                                                int* __restrict__ ovw,
                                                                int* __restrict__ grad, int64_t n_slots,
                                                                const mfnerf_grid_desc D,
                                                                const float* __restrict__ level_l1,
                                                                const mfnerf_adam_fused A, const AdamRest X,
                                                                int float_out) {
    __shared__ AccumShared S;
    const int rest_b = X.first ? (int)blockIdx.x : (int)blockIdx.x - P.n_bins;
    if (rest_b >= 0 && rest_b < X.n_blocks) {
        // independent of the slot-overflow flag: these values never go through the partitions
        TableRegions& TR = S.tr;
        TR.build(D, level_l1, X.total_vals);
        const bool skipped = A.amp && A.amp->nonfinite;
        const int stp = *A.step_dev + 1;
        const float lr = A.lr_dev ? *A.lr_dev : A.lr;
        const float bc1 = 1.0f - powf(A.beta1, (float)stp);
        const float bc2 = 1.0f - powf(A.beta2, (float)stp);
        adam_fixed_body(A.params, X.g, A.m, A.v, reinterpret_cast<__half*>(A.p16), A.table_offset, X.priv,
                        X.dense_vals, X.total_vals, TR, lr, A.beta1, A.beta2, A.eps, bc1, bc2, skipped,
                        (int64_t)rest_b * blockDim.x + threadIdx.x, X.end4, (int64_t)X.n_blocks * blockDim.x);
        return;
    }
    const bool add_words = *ovf != 0;  // a slot overflowed: its records are in the gradient words
    AccImage& img = S.a.img;
    const int bin = (int)blockIdx.x - (X.first ? X.n_blocks : 0);
    const int n_ent = 1 << P.shift, mask = n_ent - 1;
    const int64_t nn = n_dev ? min<int64_t>(n, (int64_t)*n_dev) : n;
    const int64_t slot = slot_size(min(nn, n_slots), P);  // = bin_scatter_kernel's
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NW = ACC_THREADS / 64;
    const int32_t* cnt = scnt + (int64_t)bin * UNITS;
    const uint2* base = rec + (int64_t)bin * UNITS * slot;
    const int t = bin_table(P, bin);
    const int64_t e_lo = (int64_t)(bin - P.t_bin0[t]) << P.shift;
    const int n_e = (int)min<int64_t>(n_ent, (int64_t)P.t_size[t] - e_lo);
    // (1) the slot counts, each slot's largest contribution ...
    int c = 0;
    float term = 0.0f;
    bool full = false;  // a slot of this partition overflowed (its extra records: overflow_add)
    if (tid < UNITS) {
        const int c0 = cnt[tid];
        c = min(c0, (int32_t)slot);  // (slot is even: a 16-record multiple)
        full = c0 > slot;
        term = (float)c * __uint_as_float(smax[tid]);
    }
    // ... (fused) this thread's entries' optimizer state is loaded after the last chunk's records
    // (below): in flight through that chunk's adds
    constexpr int IT = MAX_BIN_ENTRIES / ACC_THREADS;
    float2 p[IT], m[IT], v[IT];
    const int64_t base_v = A.table_offset + 2 * ((int64_t)P.t_offset[t] + e_lo);
    float2* __restrict__ pp = reinterpret_cast<float2*>(A.params + base_v);
    float2* __restrict__ mm = reinterpret_cast<float2*>(A.m + base_v);
    float2* __restrict__ vv = reinterpret_cast<float2*>(A.v + base_v);
    for (int i = tid; i < n_ent; i += ACC_THREADS) img.set(i, make_int2(0, 0));
    // (2) exclusive prefix of the counts rounded up to even (waves 0-3 hold them): every slot's run
    // starts on a 16-B record pair in the stage; and the partition's bound (sum over units of count x
    // max, summed in a fixed order) -> its unit 2^-k
    const int c2 = (c + 1) & ~1;
    int x = c2;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) term += __shfl_xor(term, off, 64);
    if (lane == 63) S.a.wtot[wv] = x;
    if (lane == 0) S.a.wsum[wv] = term;
    full = __syncthreads_or(full);
    {
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int s = S.a.wtot[k];
            before += k < wv ? s : 0;
            total += s;
        }
        if (tid < UNITS) S.a.pre[tid] = before + x - c2;
        if (tid == 0) S.a.pre[UNITS] = total;
    }
    float bound = 0.0f;
#pragma unroll
    for (int k = 0; k < NW; ++k) bound += S.a.wsum[k];
    int kbits = 0;
    // a partition with an overflowed slot sums at the table's own unit: every contribution, in the
    // image or added by overflow_add, is then rounded alike, so the sum does not depend on which of
    // them (an LDS-atomic arrival order) went past the slot -- bit-reproducible
    if (bound > 0.0f && !full) {
        int e;
        frexpf(bound * 1.0001f, &e);  // bound (with margin for its own rounding) < 2^e
        kbits = max(0, min(30, 30 - e));
    }
    const float k2 = ldexpf(1.0f, kbits + 15);  // the records' values are 2^-15 x table units
    __syncthreads();
    const int T = S.a.pre[UNITS];
    // lane j < 32 of wave wv: the run bounds of slot wv + NW j (read by the wave one slot at a time)
    const int my_u = wv + NW * (lane & 31);
    const int my_lo = my_u < UNITS ? S.a.pre[my_u] : T, my_hi = my_u < UNITS ? S.a.pre[my_u + 1] : T;
    static_assert(ACC_RB % 2 == 0, "chunks of whole record pairs");
    auto copy_chunk = [&](int c0, int c1) __attribute__((always_inline)) {
        // (3) wave wv copies the part of its slots' runs inside [c0, c1): 16 B (a record pair) per lane,
        // 128 records per instruction (4-B lanes measured TA-bound: 48 us of the accumulate's 92).
        // (A gather -- instruction i of the chunk on wave i mod 8, each lane's pair found in its slot
        // by a binary search of the prefix: ~4x fewer instructions, all lanes busy -- measured 96.5
        // vs 94.3 us: the instruction count is not what bounds the copy, profiles/r05_v6_*.)
        // only the wave's slots with records inside the chunk (a ballot of its 32 slot lanes): the
        // chunks cover the slots in order, so most of a wave's slots lie in other chunks.  (Round 6
        // again measured the gather -- a pair -> slot byte map per chunk, every lane busy: Lego
        // within noise, config 3's field 1.143 vs 1.113 ms, its 8 chunks per partition each paying
        // the map; profiles/r06_v10_accum_probe.txt)
        uint64_t todo = __ballot((lane < 32) & (my_lo < c1) & (my_hi > c0) & (my_lo < my_hi));
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int lo = max(__builtin_amdgcn_readlane(my_lo, j), c0);
            const int hi = min(__builtin_amdgcn_readlane(my_hi, j), c1);
            const int r0 = __builtin_amdgcn_readlane(my_lo, j);  // the slot's first record's place
            const uint4* src = reinterpret_cast<const uint4*>(base + (uint32_t)(NW * j + wv) * (uint32_t)slot);
            for (int q = lo; q < hi; q += 128) {
                const int k = q + 2 * lane;  // records k, k + 1 of the compacted partition (k even)
                if (k < hi)
                    __builtin_amdgcn_global_load_lds(src + ((k - r0) >> 1), &S.a.recs[q - c0], 16, 0, 2);  // nt: read once
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // an odd slot's pad record (the slot's next, stale record) becomes a zero record (no adds)
        if (tid < UNITS && (c & 1)) {
            const int k = S.a.pre[tid] + c;
            if (k >= c0 && k < c1) S.a.recs[k - c0] = make_uint2(0u, 0u);
        }
        __syncthreads();
    };
    auto add_chunk = [&](int c0, int c1) __attribute__((always_inline)) {
        // (4) the adds, in a strided order over the stage
        const int len = c1 - c0;
        const int perm = (tid * 37) & (ACC_THREADS - 1);
        constexpr int UR = 4;  // stage reads in flight per thread before the first add
        for (int i0 = 0; i0 < len; i0 += UR * ACC_THREADS) {
            uint2 r[UR];
#pragma unroll
            for (int q = 0; q < UR; ++q) r[q] = S.a.recs[min(i0 + q * ACC_THREADS + perm, ACC_RB - 1)];
#pragma unroll
            for (int q = 0; q < UR; ++q)
                if (i0 + q * ACC_THREADS + perm < len) accum_record(img, mask, r[q], k2);
        }
    };
    int c0 = 0;
    for (; T - c0 > ACC_RB; c0 += ACC_RB) {
        if (c0 > 0) __syncthreads();  // the previous chunk's adds are done with the stage
        copy_chunk(c0, c0 + ACC_RB);
        add_chunk(c0, c0 + ACC_RB);
    }
    if (c0 > 0) __syncthreads();
    copy_chunk(c0, T);  // the last chunk (T == 0: no records, its barriers only)
    if constexpr (FUSED) {
        // the optimizer state, loaded now: its loads then overlap the last chunk's adds instead of
        // delaying the partition's start.  Round 6: loaded first and guarded by `i < n_e`, each
        // entry's three loads were waited for inside their branch (a register copy out of the
        // loaded pair), four round trips in a row before the record copies began -- 27 % of a
        // partition workgroup's cycles (the phase probe, profiles/r06_v10_accum_probe.txt).
        // Unconditional here (a clamped index: the values past n_e are never used), no branch
        // and no copy; issued after the copy's wait, so the stage reads below need no vmcnt wait.
        // The clamp is in bounds because every partition has n_e >= 1: check_desc rejects empty
        // levels, and bin_plan refuses an empty table and ceil-divides each table into partitions.
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = min(tid + k * ACC_THREADS, n_e - 1);  // (streamed once per step: non-temporal)
            const float2v a = __builtin_nontemporal_load(reinterpret_cast<const float2v*>(pp + i));
            const float2v b = __builtin_nontemporal_load(reinterpret_cast<const float2v*>(mm + i));
            const float2v c3 = __builtin_nontemporal_load(reinterpret_cast<const float2v*>(vv + i));
            p[k] = make_float2(a.x, a.y);
            m[k] = make_float2(b.x, b.y);
            v[k] = make_float2(c3.x, c3.y);
        }
    }
    add_chunk(c0, T);
    __syncthreads();
    int* dst = grad + 2 * ((int64_t)P.t_offset[t] + e_lo);
    int2* ow = reinterpret_cast<int2*>(ovw) + ((int64_t)(P.t_offset[t] - P.t_offset[0]) + e_lo);  // overflow words
    const int rnd = kbits > 0 ? 1 << (kbits - 1) : 0;
    if constexpr (FUSED) {
        // fused optimizer (mfnerf_adam_step_fixed_partial): the entry's finished int32 sums, converted
        // with the table's scale exactly as adam_fixed_kernel converts them, feed the same Adam update;
        // the gradient words are left alone (zero)
        const float sc = table_fixed_scale(D, level_l1, P.t_level[t]);
        const float is = sc > 0.0f ? 1.0f / sc : 0.0f;
        if (add_words) {  // the overflowed records' sums join the image; the words are zeroed
            for (int i = threadIdx.x; i < n_e; i += blockDim.x) {
                const int2 g = ow[i];  // overflow_add's packed word
                const int2 v = img.get(i);
                const int o0 = ((v.x + rnd) >> kbits) + g.x, o1 = ((v.y + rnd) >> kbits) + g.y + (g.x < 0);
                img.set(i, make_int2(o0, o1));
                ow[i] = make_int2(0, 0);
            }
            __syncthreads();
        }
        if (A.amp && A.amp->nonfinite) return;  // GradScaler skip: no update (gradient words stay zero)
        const int kb = add_words ? 0 : kbits, rd = add_words ? 0 : rnd;  // (image now in table units)
        const int stp = *A.step_dev + 1;
        const float lr = A.lr_dev ? *A.lr_dev : A.lr;
        const float bc1 = 1.0f - powf(A.beta1, (float)stp);
        const float bc2 = 1.0f - powf(A.beta2, (float)stp);
        __half2* __restrict__ hh = reinterpret_cast<__half2*>(reinterpret_cast<__half*>(A.p16) + base_v);
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int i = tid + k * ACC_THREADS;
            if (i >= n_e) break;
            const int2 vv2 = img.get(i);
            const float g0 = (float)((vv2.x + rd) >> kb) * is, g1 = (float)((vv2.y + rd) >> kb) * is;
            mfn::adam_elem(p[k].x, m[k].x, v[k].x, g0, A.beta1, A.beta2, A.eps, lr, bc1, bc2);
            mfn::adam_elem(p[k].y, m[k].y, v[k].y, g1, A.beta1, A.beta2, A.eps, lr, bc1, bc2);
            __builtin_nontemporal_store(float2v{p[k].x, p[k].y}, reinterpret_cast<float2v*>(pp + i));
            __builtin_nontemporal_store(float2v{m[k].x, m[k].y}, reinterpret_cast<float2v*>(mm + i));
            __builtin_nontemporal_store(float2v{v[k].x, v[k].y}, reinterpret_cast<float2v*>(vv + i));
            if (A.p16) hh[i] = __floats2half2_rn(p[k].x, p[k].y);
        }
        return;
    }
    // float_out: the finished sums as float gradients (the int32 value times 1 / the table's scale,
    // exactly what fold_convert_kernel computes), else the int32 sums for the finish pass
    const float sc = float_out ? table_fixed_scale(D, level_l1, P.t_level[t]) : 0.0f;
    const float is = sc > 0.0f ? 1.0f / sc : 0.0f;
    for (int i = threadIdx.x; i < n_e; i += blockDim.x) {
        const int2 v = img.get(i);
        // back to the table's unit, rounded once (|fields| <= 2^30: no overflow adding rnd)
        int2 o = make_int2((v.x + rnd) >> kbits, (v.y + rnd) >> kbits);
        if (add_words) {
            const int2 g = ow[i];  // overflow_add's packed f1 * 2^32 + f0
            o.x += g.x;
            o.y += g.y + (g.x < 0);
            ow[i] = make_int2(0, 0);
        }
        if (float_out) reinterpret_cast<float2*>(dst)[i] = make_float2((float)o.x * is, (float)o.y * is);
        else reinterpret_cast<int2*>(dst)[i] = o;
    }
}

// first level routed through the bins (the dense levels before it use grid_bw_dense_kernel): every
// hashed level (binning only the last 6 measured 392 vs 365 us for the scatter in round 2) --
// extended down to every level that shares a table with them (MixedFeature), since a partition is
// stored whole.
int first_binned_level(const mfnerf_grid_desc* d) {
    int first_hashed = d->n_levels;
    for (int l = 0; l < d->n_levels; ++l) {
        const uint64_t r = d->res[l];
        if (!(d->table_kind[l] == 0 && r * r * r <= d->size[l])) { first_hashed = l; break; }
    }
    int l0 = first_hashed;
    for (bool moved = true; moved;) {
        moved = false;
        for (int a = first_hashed; a < l0 && !moved; ++a)
            for (int b = l0; b < d->n_levels; ++b)
                if (d->offset[a] == d->offset[b]) { l0 = a; moved = true; break; }
    }
    // (round 6: also partitioning a MixedFeature layout's finest dense levels -- res >= 60 or >= 80,
    // as merged single records instead of run-merged atomics -- measured the same: mf128 1.197-1.200
    // vs 1.199-1.202 ms/step, r6e)
    return l0;
}

// The plan for a desc: binned levels = every level that is not a dense own table; tables in address
// order.  Returns the number of bins (0: nothing to bin), or -1 for a layout the kernels do not take.
int bin_plan(const mfnerf_grid_desc* d, BinPlan* P) {
    *P = BinPlan{};
    const int l_first = first_binned_level(d);
    P->pair_ok = 1;
    uint64_t entries = 0, max_x = 0;
    for (int l = l_first; l < d->n_levels; ++l) {  // (the levels before: dense, atomics)
        int t = 0;
        while (t < P->n_tables && P->t_offset[t] != d->offset[l]) ++t;
        if (t == P->n_tables) {
            P->t_offset[t] = d->offset[l];
            P->t_size[t] = d->size[l];
            P->t_level[t] = l;
            P->n_tables++;
            entries += d->size[l];
        }
        P->table_of[l] = t;
        P->pairable[l] = d->table_kind[l] == 0 && (d->size[l] & (d->size[l] - 1)) == 0;
        // never a pair record: a shared table whose canonical x-step floor(canon_res / res) >= 3, or an
        // own table without the power-of-two hash -> runs merged (merged_level_records)
        P->merge[l] = d->table_kind[l] == 1 ? (uint64_t)d->canon_res >= 3 * (uint64_t)d->res[l] : !P->pairable[l];
        P->level[P->n_binned++] = l;
        max_x = max(max_x, (uint64_t)(d->table_kind[l] == 1 ? (uint32_t)d->canon_res : d->res[l]));
    }
    // every partition holds >= 1 entry (bin_accum_kernel clamps its state loads to n_e - 1): no empty
    // table (check_desc lets none through), and the ceil-division below adds no empty partition
    for (int t = 0; t < P->n_tables; ++t)
        if (P->t_size[t] == 0) return -1;
    // the largest partition (fewest records to route, least LDS per entry) leaving >= 1024 of them
    // (round 6, config 3's field -- 2^20 binned entries, 1024 partitions of 2^10 here: at least 512 /
    // 2048 / 4096 partitions ran 1.158 / 1.167 / 1.211 vs 1.149 ms/step, and the Lego step at 5120
    // partitions of 2^10 0.624 vs 0.506; profiles/r06_v8_ab_partition_count.txt)
    P->shift = MAX_BIN_SHIFT;
    while (P->shift > MIN_BIN_SHIFT && (entries >> P->shift) < 1024) --P->shift;
    int nb = 0;
    for (int t = 0; t < P->n_tables; ++t) {
        P->t_bin0[t] = nb;
        nb += (int)((P->t_size[t] + (1u << P->shift) - 1) >> P->shift);
        // x-corner indices differ below the top bit of x ^ (x+1), x + 1 <= max_x, in an own power-of-two
        // hash table: one record per row; otherwise up to two
        if ((P->t_size[t] & (P->t_size[t] - 1)) || max_x >= (1ull << P->shift)) P->pair_ok = 0;
    }
    for (int j = 0; j < P->n_binned; ++j) {
        if (!P->pairable[P->level[j]]) P->pair_ok = 0;
    }
    P->t_bin0[P->n_tables] = nb;
    P->n_bins = nb;
    if (P->n_binned > MAX_BINNED) return -1;
    for (int j = 1; j < P->n_binned; ++j)  // the binned levels are contiguous (staged dL/dy rows)
        if (P->level[j] != P->level[0] + j) return -1;
    for (int t = 0; t < P->n_tables; ++t)
        if (P->t_bin0[t + 1] - P->t_bin0[t] > MAX_TBINS) return -1;
    return nb > MAX_BINS ? -1 : nb;
}

struct BinWorkspace {
    float* priv;
    int32_t *scnt, *ovf;
    int* ovw;  // overflow words: one packed int64 per partitioned entry (zero between steps)
    uint32_t* smax;
    uint2* rec;
};

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// workspace = [private copies of the dense levels | overflow words | slot counts | overflow flag |
// record slots]
int64_t binned_workspace_layout(const mfnerf_grid_desc* d, int64_t n_max, char* base, BinWorkspace* W) {
    BinPlan P;
    if (bin_plan(d, &P) < 0) return -1;
    int64_t off = align256((int64_t)GRAD_COPIES * dense_entries_of(d) * 2 * (int64_t)sizeof(float));
    if (W) W->priv = reinterpret_cast<float*>(base);
    int64_t part_entries = 0;
    for (int t = 0; t < P.n_tables; ++t) part_entries += P.t_size[t];
    if (W) W->ovw = reinterpret_cast<int*>(base + off);
    off += align256(part_entries * 8);
    const int64_t nb = P.n_bins > 0 ? P.n_bins : 1;
    if (W) W->scnt = reinterpret_cast<int32_t*>(base + off);
    off += align256(nb * UNITS * 4);
    if (W) W->smax = reinterpret_cast<uint32_t*>(base + off);
    off += align256(UNITS * 4);
    if (W) W->ovf = reinterpret_cast<int32_t*>(base + off);
    off += 256;
    if (W) W->rec = reinterpret_cast<uint2*>(base + off);
    // every slot at the largest live count (the same function the kernels size them with); the
    // scatter addresses records with 32-bit indices
    if (nb * UNITS * slot_size(n_max, P) >= (int64_t)1 << 31) return -1;
    off += align256(nb * UNITS * slot_size(n_max, P) * (int64_t)sizeof(uint2));
    return off;
}

// mfnerf_grid_encode_bw_binned's `parts` mask
constexpr int PART_DENSE = 1;   // the levels before the partitioned ones, into the private copies
constexpr int PART_BINNED = 2;  // the partitioned tables: scatter -> accumulate
constexpr int PART_FLOAT = 4;   // the accumulate stores float gradients, not int32 sums (no fused Adam)

// The fused-Adam arguments of the entry points that take them: non-null vectors aligned to
// align_mask + 1 bytes (grads too where given), table_offset a multiple of offset_mult.
int validate_adam_fused(const mfnerf_adam_fused* adam, const float* grads, uintptr_t align_mask, int offset_mult,
                        const char* what) {
    if (adam && adam->params && adam->m && adam->v && adam->step_dev && adam->table_offset % offset_mult == 0 &&
        !(((uintptr_t)adam->params | (uintptr_t)adam->m | (uintptr_t)adam->v | (uintptr_t)grads) & align_mask))
        return MFN_OK;
    mfn_set_error("%s: bad Adam arguments (null or misaligned vectors, table_offset not a multiple of %d)", what,
                  offset_mult);
    return MFN_ERR_INVALID;
}

int binned_impl(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table, void* workspace,
                int64_t n_slots, const float* level_l1, int parts, const mfnerf_adam_fused* adam,
                mfnerf_stream_t stream, const AdamRest* rest = nullptr) {
    int st = check_desc(desc, "grid_encode_bw_binned");
    if (st) return st;
    if (n_slots <= 0 || n_slots > n) n_slots = n;
    if (n < 0 || parts < 1 || parts > (PART_DENSE | PART_BINNED | PART_FLOAT) || ((parts & PART_FLOAT) && adam)) {
        mfn_set_error("grid_encode_bw_binned: bad size or parts");
        return MFN_ERR_INVALID;
    }
    if (n == 0) return MFN_OK;
    if (!x || !dL_dout || !grad_table || !workspace || !level_l1) {
        mfn_set_error("grid_encode_bw_binned: null pointer (workspace and level_l1 are required)");
        return MFN_ERR_INVALID;
    }
    BinPlan P;
    if (bin_plan(desc, &P) < 0) {
        mfn_set_error("grid_encode_bw_binned: unsupported layout (> %d partitions, > %d bins per table, or binned "
                      "levels not the contiguous last %d)", MAX_BINS, MAX_TBINS, MAX_BINNED);
        return MFN_ERR_INVALID;
    }
    BinWorkspace W;
    if (binned_workspace_layout(desc, n_slots, (char*)workspace, &W) < 0) {
        mfn_set_error("grid_encode_bw_binned: %lld record slots per partition and unit overflow 32-bit record "
                      "indices (size the slots for fewer samples, n_slots)", (long long)n_slots);
        return MFN_ERR_INVALID;
    }
    int32_t* const gate = rest ? rest->gate : nullptr;
    // levels [0, l_first): their launch also clears the slot-overflow flag the scatter starts from
    const int l_first = first_binned_level(desc);
    const bool dense_launch = (parts & PART_DENSE) && l_first > 0;
    const bool gate_opened = dense_launch && launch_dense_levels(x, n, n_dev, x_min, x_range, desc, dL_dout,
                                                                 grad_table, W.priv, level_l1, l_first,
                                                                 (parts & PART_BINNED) ? W.ovf : nullptr, gate, stream);
    // the gate opens here whichever dense path ran (only grid_bw_dense_kernel opens it itself)
    if (gate && !gate_opened) mfnerf_gate_signal(gate, stream);  // (after the request-shaped atomics, or first)
    if ((parts & PART_BINNED) && P.n_bins > 0) {
        if (!dense_launch) mfn_zero_async(W.ovf, sizeof(int32_t), stream);
        // the staged dL/dy rows sized for the binned levels (10 at the Lego layout; MixedFeature's
        // shared tables bin more): the smallest staging that holds them leaves room on each CU for
        // the side stream's march kernels
        auto sk = P.pair_ok ? (P.n_binned <= 8    ? bin_scatter_kernel<8, true>
                               : P.n_binned <= 10 ? bin_scatter_kernel<10, true>
                               : P.n_binned <= 12 ? bin_scatter_kernel<12, true>
                                                  : bin_scatter_kernel<MAX_BINNED, true>)
                            : (P.n_binned <= 8    ? bin_scatter_kernel<8, false>
                               : P.n_binned <= 12 ? bin_scatter_kernel<12, false>
                                                  : bin_scatter_kernel<MAX_BINNED, false>);
        hipLaunchKernelGGL(sk, dim3(UNITS), dim3(SC_THREADS), 0, stream, x, n, n_dev, x_min, x_range,
                           *desc, P, dL_dout, level_l1, W.rec, W.scnt, W.smax, W.ovf, n_slots, W.ovw);

        mfnerf_adam_fused A{};
        if (adam) A = *adam;
        AdamRest X{};
        if (rest) X = *rest;
        hipLaunchKernelGGL(A.params ? bin_accum_kernel<true> : bin_accum_kernel<false>, dim3(P.n_bins + X.n_blocks),
                           dim3(ACC_THREADS), 0, stream, P, n, n_dev,
                           W.rec, W.scnt, W.smax, W.ovf, W.ovw, (int*)grad_table, n_slots, *desc, level_l1, A, X,
                           (parts & PART_FLOAT) ? 1 : 0);
    }
    return mfn_check_launch("grid_encode_bw_binned");
}

}  // namespace

void mfn_grid::launch_fold_convert(float* grad, int* priv, int64_t dense_vals, int64_t total_vals,
                                   const mfnerf_grid_desc* desc, const float* level_l1, const int32_t* flag,
                                   int64_t flag_world, int64_t flag_shard_len, int64_t table_off,
                                   mfnerf_stream_t stream) {
    const int64_t fb = div_up<int64_t>(total_vals / 4, 256);
    hipLaunchKernelGGL(fold_convert_kernel, dim3((unsigned)(fb < 4096 ? fb : 4096)), dim3(256), 0, stream, grad, priv,
                       dense_vals, total_vals, *desc, level_l1, ShardFlag{flag, flag_world, flag_shard_len, table_off});
}

extern "C" {

int mfnerf_adam_step_fixed(float* params, float* grads, float* m, float* v, void* p_f16, int64_t n,
                           int64_t table_offset, const mfnerf_grid_desc* desc, void* workspace,
                           float* level_l1, float lr, float beta1, float beta2, float eps,
                           int32_t* step_dev, const float* lr_dev, mfnerf_amp_state* amp, mfnerf_stream_t stream) {
    return mfnerf_adam_step_fixed_partial(params, grads, m, v, p_f16, n, table_offset, desc, workspace, level_l1, lr,
                                          beta1, beta2, eps, step_dev, lr_dev, amp, n, nullptr, stream);
}

int mfnerf_adam_step_fixed_partial(float* params, float* grads, float* m, float* v, void* p_f16, int64_t n,
                                   int64_t table_offset, const mfnerf_grid_desc* desc, void* workspace,
                                   float* level_l1, float lr, float beta1, float beta2, float eps,
                                   int32_t* step_dev, const float* lr_dev, mfnerf_amp_state* amp, int64_t fused_from,
                                   const int32_t* fused_ovf, mfnerf_stream_t stream) {
    int st = check_desc(desc, "adam_step_fixed");
    if (st) return st;
    if (!params || !grads || !m || !v || !step_dev || !level_l1) {
        mfn_set_error("adam_step_fixed: null pointer"); return MFN_ERR_INVALID;
    }
    if ((((uintptr_t)params) | ((uintptr_t)grads) | ((uintptr_t)m) | ((uintptr_t)v)) & 15 ||
        (p_f16 && (((uintptr_t)p_f16) & 7))) {
        mfn_set_error("adam_step_fixed: misaligned buffer"); return MFN_ERR_INVALID;
    }
    const int64_t total = table_values_of(desc);
    const int64_t dense = workspace ? dense_entries_of(desc) : 0;
    if (fused_from < 0 || fused_from > n || fused_from % 4) {
        mfn_set_error("adam_step_fixed_partial: fused_from (%lld) must be a multiple of 4 in [0, n]",
                      (long long)fused_from);
        return MFN_ERR_INVALID;
    }
    if (n % 4 || table_offset % 4 || table_offset < 0 || table_offset + total > n) {
        mfn_set_error("adam_step_fixed: n (%lld) and table_offset (%lld) must be multiples of 4 holding the table",
                      (long long)n, (long long)table_offset);
        return MFN_ERR_INVALID;
    }
    // sized for the range normally updated: every workgroup takes the last-workgroup ticket (one
    // memory-side atomic on ONE address each, serialised: ~13 ns apiece), so an idle workgroup is
    // not free (4096 of them cost ~55 us in the fused_from case); grid-stride covers the rest
    const int64_t want = div_up<int64_t>((fused_ovf ? fused_from : n) / 4, 256);
    // measured: 4096 -> 1024 workgroups 88 -> 78 us (fewer tickets, same bandwidth)
    constexpr int64_t ADAM_BLOCKS = 1024;
    hipLaunchKernelGGL(adam_fixed_kernel,
                       dim3((unsigned)(want < ADAM_BLOCKS ? (want < 1 ? 1 : want) : ADAM_BLOCKS)), dim3(256), 0,
                       stream, params, grads, m, v, (__half*)p_f16, n, table_offset, (int*)workspace, 2 * dense,
                       total, *desc, level_l1, lr, beta1, beta2, eps, step_dev, lr_dev, amp, desc->n_levels,
                       fused_from, fused_ovf, 0, PackArgs{nullptr, nullptr, nullptr, 0});
    if (!amp)  // else the kernel's last workgroup did it
        hipLaunchKernelGGL(mfn_bump_step_kernel, dim3(1), dim3(1), 0, stream, step_dev, amp, level_l1, desc->n_levels);
    return mfn_check_launch("adam_step_fixed");
}

// Partitioned (binned) fixed-point table-gradient scatter: the dense levels through grid_bw_body's
// private copies (parts & 1), the hashed / shared tables through scatter -> LDS accumulate (parts & 2).
int64_t mfnerf_grid_encode_bw_binned_workspace(const mfnerf_grid_desc* desc, int64_t n_max) {
    if (check_desc(desc, "grid_encode_bw_binned_workspace") || n_max < 0) return -1;
    return binned_workspace_layout(desc, n_max, nullptr, nullptr);
}

int mfnerf_grid_encode_bw_binned(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                 const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                 void* workspace, int64_t n_slots, const float* level_l1, int parts,
                                 mfnerf_stream_t stream) {
    return binned_impl(x, n, n_dev, x_min, x_range, desc, dL_dout, grad_table, workspace, n_slots, level_l1, parts,
                       nullptr, stream);
}

int mfnerf_grid_encode_bw_binned_float(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                       const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                       void* workspace, int64_t n_slots, const float* level_l1, int32_t* gate,
                                       const int32_t* flag, int64_t flag_world, int64_t flag_shard_len,
                                       int64_t table_offset, mfnerf_stream_t stream) {
    if (flag && (flag_world < 1 || flag_world > 256 || flag_shard_len < 1 || table_offset < 0)) {
        mfn_set_error("grid_encode_bw_binned_float: bad shard-flag arguments");
        return MFN_ERR_INVALID;
    }
    BinPlan P;
    if (check_desc(desc, "grid_encode_bw_binned_float") || bin_plan(desc, &P) <= 0) {
        mfn_set_error("grid_encode_bw_binned_float: bad desc or nothing partitioned");
        return MFN_ERR_INVALID;
    }
    AdamRest X{};  // no optimizer blocks; only the gate (opened as the dense-level launch starts)
    X.gate = gate;
    int st = binned_impl(x, n, n_dev, x_min, x_range, desc, dL_dout, grad_table, workspace, n_slots, level_l1,
                         PART_DENSE | PART_BINNED | PART_FLOAT, nullptr, stream, gate ? &X : nullptr);
    if (st || n == 0) return st;
    // the values before the partitioned tables: the dense levels' copies folded, any other level's
    // int32 sums converted (the accumulate wrote the partitioned tables' floats)
    const int64_t head = 2 * (int64_t)P.t_offset[0];
    if (head > 0) {
        launch_fold_convert(grad_table, (int*)workspace, 2 * dense_entries_of(desc), head, desc, level_l1, flag,
                            flag_world, flag_shard_len, table_offset, stream);
    } else if (flag) {
        mfn_set_error("grid_encode_bw_binned_float: a shard flag needs a table prefix to ride");
        return MFN_ERR_INVALID;
    }
    return mfn_check_launch("grid_encode_bw_binned_float");
}

int mfnerf_grid_encode_bw_binned_adam(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                      const mfnerf_grid_desc* desc, const float* dL_dout, float* grad_table,
                                      void* workspace, int64_t n_slots, const float* level_l1,
                                      const mfnerf_adam_fused* adam, mfnerf_stream_t stream) {
    if (int st = validate_adam_fused(adam, nullptr, 7, 2, "grid_encode_bw_binned_adam")) return st;
    return binned_impl(x, n, n_dev, x_min, x_range, desc, dL_dout, grad_table, workspace, n_slots, level_l1,
                       PART_DENSE | PART_BINNED, adam, stream);
}

int mfnerf_grid_encode_bw_binned_adam_all(const float* x, int64_t n, const int32_t* n_dev, float x_min, float x_range,
                                          const mfnerf_grid_desc* desc, const float* dL_dout, float* grads,
                                          int64_t n_params, void* workspace, int64_t n_slots, float* level_l1,
                                          const mfnerf_adam_fused* adam, int32_t* step_dev, mfnerf_amp_state* amp,
                                          void* packed, int rgb_width, int32_t* gate, mfnerf_stream_t stream) {
    const char* what = "grid_encode_bw_binned_adam_all";
    if (packed && ((rgb_width != 64 && rgb_width != 128) || !adam || !adam->p16)) {
        mfn_set_error("%s: the repack needs rgb_width 64 or 128 and adam->p16", what);
        return MFN_ERR_INVALID;
    }
    int st = validate_adam_fused(adam, grads, 15, 4, what);
    if (st) return st;
    if (!grads || adam->step_dev != step_dev || adam->amp != amp || (adam->p16 && ((uintptr_t)adam->p16 & 7)) ||
        n_params % 4 || adam->table_offset < 0) {
        mfn_set_error("%s: bad Adam arguments (null grads, misaligned p16, n_params not a multiple of 4, negative "
                      "table_offset, step_dev / amp differing from adam's)", what);
        return MFN_ERR_INVALID;
    }
    st = check_desc(desc, what);
    if (st) return st;
    const int64_t total = table_values_of(desc);
    BinPlan P;
    if (bin_plan(desc, &P) <= 0 || adam->table_offset + total > n_params) {
        mfn_set_error("%s: nothing partitioned, or the table outside [table_offset, n_params)", what);
        return MFN_ERR_INVALID;
    }
    const int64_t fused_from = adam->table_offset + 2 * (int64_t)P.t_offset[0];  // the partitioned tables' first value
    if (fused_from % 4) { mfn_set_error("%s: partitions not float4-aligned", what); return MFN_ERR_INVALID; }
    BinWorkspace W;
    if (binned_workspace_layout(desc, n_slots <= 0 || n_slots > n ? n : n_slots, (char*)workspace, &W) < 0) {
        mfn_set_error("%s: the record slots overflow 32-bit record indices", what);
        return MFN_ERR_INVALID;
    }
    // [0, fused_from) by the accumulate launch's leading workgroups (one float4 per thread, <= 256 of
    // them)
    AdamRest X{grads, (int*)workspace, 2 * dense_entries_of(desc), total, fused_from / 4, 0, 1, gate};
    // <= 256 workgroups, the grid's first (256 vs 64 of them 0.655 vs 0.657 ms/step; first vs last
    // in the grid within noise)
    const int64_t want = div_up<int64_t>(fused_from / 4, ACC_THREADS);
    X.n_blocks = (int)(want < 1 ? 1 : (want < 256 ? want : 256));
    st = binned_impl(x, n, n_dev, x_min, x_range, desc, dL_dout, grads + adam->table_offset, workspace, n_slots,
                     level_l1, PART_DENSE | PART_BINNED, adam, stream, &X);
    if (st) return st;
    // the MLP repack and the step's bookkeeping (step count, loss scale, level_l1 zeroed) by the last
    // workgroup -- after every workgroup of the accumulate has read them
    hipLaunchKernelGGL(adam_fixed_kernel, dim3(64), dim3(256), 0, stream, adam->params, grads, adam->m, adam->v,
                       (__half*)adam->p16, n_params, adam->table_offset, (int*)workspace, 2 * dense_entries_of(desc),
                       total, *desc, level_l1, adam->lr, adam->beta1, adam->beta2, adam->eps, step_dev, adam->lr_dev,
                       amp, desc->n_levels, fused_from, (const int32_t*)W.ovf, 1,
                       PackArgs{(const _Float16*)adam->p16, (const _Float16*)adam->p16 + mfn_field::N_XYZ_PARAMS,
                                (_Float16*)packed, rgb_width});
    if (!amp)
        hipLaunchKernelGGL(mfn_bump_step_kernel, dim3(1), dim3(1), 0, stream, step_dev, amp, level_l1, desc->n_levels);
    return mfn_check_launch(what);
}

int64_t mfnerf_grid_binned_first_value(const mfnerf_grid_desc* desc) {
    if (check_desc(desc, "grid_binned_first_value")) return -1;
    BinPlan P;
    if (bin_plan(desc, &P) <= 0) return -1;
    return 2 * (int64_t)P.t_offset[0];
}

int64_t mfnerf_grid_dense_values(const mfnerf_grid_desc* desc) {
    if (check_desc(desc, "grid_dense_values")) return -1;
    return 2 * dense_entries_of(desc);
}

int64_t mfnerf_grid_encode_bw_binned_flag_offset(const mfnerf_grid_desc* desc, int64_t n_slots) {
    if (check_desc(desc, "grid_encode_bw_binned_flag_offset") || n_slots <= 0) return -1;
    BinWorkspace W;
    if (binned_workspace_layout(desc, n_slots, nullptr, &W) < 0) return -1;
    return (int64_t)reinterpret_cast<uintptr_t>(W.ovf);
}

}  // extern "C"
