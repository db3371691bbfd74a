// mesh_clean.hip -- floaters out of an extracted mesh, on the device (the reference's test.ipynb
// "mesh" cell leaves them to the user: "tune these parameters until the whole object lies tightly in
// range with little noise").  Three things, all specified by tests/mesh_clean_ref.py:
//
//   connected components  labels[v] = the smallest vertex index of v's component (two vertices are
//                         connected when a face holds both), face_counts[r] = faces of the component
//                         labelled r.  A pure function of (V, faces): integer atomics only, the same
//                         bits on every run whatever order the hardware unites in.
//   selection, compaction keep flags from the counts (thresholds computed here, no host read), then a
//                         stable copy of the kept vertices and faces, indices remapped.
//   occupancy cull        lattice values cleared where the renderer never samples.
//
// The labelling is a lock-free union-find over parent[] (= labels, in place), three launches after
// the initialisation: hook (one thread per face, unite (a,b) and (b,c)), flatten (one thread per
// vertex), count (ITEMS faces per thread).  No host read, no host-driven iteration.
//
// Why the hook kernel is safe:
//   (1) parent[v] <= v at all times.  init writes parent[v] = v; after that parent[] changes only in
//       unite (a compare-and-swap parent[hi]: hi -> lo with lo < hi, so it installs a smaller
//       root under a larger one) and in find_root (atomicMin(parent[x], g) with g an ancestor of x,
//       g < x).  Both only lower.  Every walk x -> parent[x] therefore strictly descends until it
//       meets parent[x] == x and ends within V steps, whatever other threads do meanwhile.
//   (2) Nobody waits.  There is no flag, no lock and no spin on another thread's write: a failed
//       compare-and-swap returns the current value of parent[hi], which is smaller than hi, and the
//       thread goes on from there; max(ra, rb) strictly falls with every failure.
//   (3) Staleness.  Every load of parent[] is a relaxed agent-scope atomic load (L1 is bypassed).
//       Should one still return an old value, that is harmless by construction: only roots are
//       hooked and shortcuts go to ancestors, so a tree's vertex set only ever grows by merging and
//       every value parent[x] ever held is a vertex of x's tree, <= x.  A walk over old values still
//       descends inside the right tree; the only step that decides anything is the compare-and-swap
//       on the presumed root, which acts on the true current value.  Final labels are read by the
//       next launch only.
//   (4) Bounds.  A face with an index outside [0, V) is skipped by every kernel here (face_ok), so
//       bad input never indexes parent[], the counts or the flags out of range.
// At the end every face's vertices share a tree (unite returns only then, and trees never split),
// parents are strictly smaller than children, so each root is its component's minimum.
#include "common.hpp"

namespace {

constexpr int CLEAN_BLOCK = 256;

__device__ __forceinline__ int32_t load_parent(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x's tree as far as this thread can see; on the way every vertex of the path is
// pointed at its grandparent (path splitting), by atomicMin so that parent[] only falls.
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
    int32_t p = load_parent(parent, x);
    while (p != x) {  // p < x: (1)
        const int32_t g = load_parent(parent, p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
    int32_t ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const int32_t hi = max(ra, rb), lo = min(ra, rb);
        const int32_t old = atomicCAS(parent + hi, hi, lo);  // the linearisation point
        if (old == hi) return;        // hi was a root and now hangs under lo
        ra = find_root(parent, old);  // old < hi: somebody hooked hi first; go on from there
        rb = lo;                      // need not be a root any more: then the next CAS fails too
    }
}

__device__ __forceinline__ bool face_ok(int32_t a, int32_t b, int32_t c, int32_t V) {
    return (uint32_t)a < (uint32_t)V && (uint32_t)b < (uint32_t)V && (uint32_t)c < (uint32_t)V;
}

__global__ __launch_bounds__(CLEAN_BLOCK) void components_init_kernel(int32_t V, int32_t* __restrict__ parent,
                                                                     int32_t* __restrict__ face_counts) {
    const int64_t v = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
    if (v >= V) return;
    parent[v] = (int32_t)v;
    face_counts[v] = 0;
}

__global__ __launch_bounds__(CLEAN_BLOCK) void components_hook_kernel(const int32_t* __restrict__ faces, int32_t V,
                                                                     int32_t F, int32_t* parent) {
    const int64_t f = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!face_ok(a, b, c, V)) return;
    unite(parent, a, b);
    unite(parent, b, c);
}

// After the hook launch the forest is final; each vertex walks to its root and stores it.  A
// concurrent store only replaces a parent by the root of the same tree, so walks still end there.
__global__ __launch_bounds__(CLEAN_BLOCK) void components_flatten_kernel(int32_t V, int32_t* parent) {
    const int64_t v = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
    if (v >= V) return;
    int32_t x = (int32_t)v, p = load_parent(parent, x);
    while (p != x) {
        x = p;
        p = load_parent(parent, x);
    }
    __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Atomics on one address are served one after another (about 7 ns each on the MI355X: one per wave
// of faces made the count 6.4 ms of a 55 M-face mesh with nearly all faces in a few components), so
// the kernels below that add into few addresses take ITEMS elements per thread, a workgroup
// covering CLEAN_BLOCK * ITEMS consecutive ones, and combine on chip first.
constexpr int ITEMS = 16;
constexpr int64_t BLOCK_ITEMS = (int64_t)CLEAN_BLOCK * ITEMS;

// The lanes of a wave that share the leader's label are counted by a ballot, then the next unserved
// lane leads.  The wave carries one (label, count) run from item to item -- the larger one when two
// labels meet -- and adds the other: one integer atomic per wave for faces of one component, one
// per distinct label of a wave at worst.
__global__ __launch_bounds__(CLEAN_BLOCK) void components_count_kernel(const int32_t* __restrict__ faces, int32_t V,
                                                                      int32_t F,
                                                                      const int32_t* __restrict__ labels,
                                                                      int32_t* __restrict__ face_counts) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t first = (int64_t)blockIdx.x * BLOCK_ITEMS + threadIdx.x;
    int32_t run_label = -1, run_count = 0;  // the same in every lane
    for (int i = 0; i < ITEMS; ++i) {
        const int64_t f = first + (int64_t)i * CLEAN_BLOCK;
        if (f - lane >= F) break;  // the whole wave is past the end
        int32_t label = -1;
        if (f < F) {
            const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
            if (face_ok(a, b, c, V)) label = labels[a];
        }
        uint64_t todo = __ballot(label >= 0);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int32_t l = __shfl(label, leader);
            const uint64_t same = __ballot(label == l);
            int32_t add_label = l, add_count = (int32_t)__popcll(same);
            if (l == run_label) {
                run_count += add_count;
                add_count = 0;
            } else if (add_count > run_count) {
                const int32_t tl = run_label, tc = run_count;
                run_label = add_label;
                run_count = add_count;
                add_label = tl;
                add_count = tc;
            }
            if (add_count > 0 && lane == 0) atomicAdd(face_counts + add_label, add_count);
            todo &= ~same;
        }
    }
    if (run_count > 0 && lane == 0) atomicAdd(face_counts + run_label, run_count);
}

// (count << 32 | INT32_MAX - label): its maximum is the largest count and, among equals, the
// smallest label
__global__ __launch_bounds__(CLEAN_BLOCK) void select_best_kernel(int32_t V, const int32_t* __restrict__ face_counts,
                                                                 unsigned long long* best) {
    __shared__ unsigned long long part[CLEAN_BLOCK / 64];
    const int64_t first = (int64_t)blockIdx.x * BLOCK_ITEMS + threadIdx.x;
    unsigned long long key = 0;
#pragma unroll 4
    for (int i = 0; i < ITEMS; ++i) {
        const int64_t v = first + (int64_t)i * CLEAN_BLOCK;
        if (v < V) {
            const unsigned long long k =
                (unsigned long long)(uint32_t)face_counts[v] << 32 | (uint32_t)(INT32_MAX - (int32_t)v);
            key = k > key ? k : key;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < CLEAN_BLOCK / 64; ++w) key = part[w] > key ? part[w] : key;
        if (key >> 32) atomicMax(best, key);  // a block of empty components has nothing to offer
    }
}

struct Selection {
    int32_t min_faces;
    float min_fraction;
    int largest_only;
};

__device__ __forceinline__ bool component_kept(int32_t label, int32_t count, unsigned long long best,
                                               const Selection& s) {
    const int32_t max_count = (int32_t)(best >> 32);
    const int32_t best_label = INT32_MAX - (int32_t)(uint32_t)best;
    if (count <= 0 || count < s.min_faces) return false;
    if (!((double)count >= (double)s.min_fraction * (double)max_count)) return false;
    return !s.largest_only || label == best_label;
}

// stats[0] += components, stats[1] += kept components: integer adds, one per workgroup and counter
__global__ __launch_bounds__(CLEAN_BLOCK) void select_vertices_kernel(int32_t V, const int32_t* __restrict__ labels,
                                                                     const int32_t* __restrict__ face_counts,
                                                                     const unsigned long long* __restrict__ best,
                                                                     Selection s, uint8_t* __restrict__ vkeep,
                                                                     long long* stats) {
    __shared__ int part[CLEAN_BLOCK / 64][2];
    const int64_t first = (int64_t)blockIdx.x * BLOCK_ITEMS + threadIdx.x;
    const unsigned long long b = *best;
    int roots = 0, kept_roots = 0;  // of the wave, the same in every lane
    for (int i = 0; i < ITEMS; ++i) {
        const int64_t v = first + (int64_t)i * CLEAN_BLOCK;
        bool root = false, kept = false;
        if (v < V) {
            const int32_t l = labels[v];
            root = l == (int32_t)v;
            kept = component_kept(l, face_counts[l], b, s);
            vkeep[v] = (uint8_t)kept;
        }
        roots += (int)__popcll(__ballot(root));
        kept_roots += (int)__popcll(__ballot(root && kept));
    }
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6][0] = roots;
        part[threadIdx.x >> 6][1] = kept_roots;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < CLEAN_BLOCK / 64; ++w) {
            roots += part[w][0];
            kept_roots += part[w][1];
        }
        if (roots) atomicAdd((unsigned long long*)stats, (unsigned long long)roots);
        if (kept_roots) atomicAdd((unsigned long long*)stats + 1, (unsigned long long)kept_roots);
    }
}

__global__ __launch_bounds__(CLEAN_BLOCK) void select_faces_kernel(const int32_t* __restrict__ faces, int32_t V,
                                                                  int32_t F, const int32_t* __restrict__ labels,
                                                                  const int32_t* __restrict__ face_counts,
                                                                  const unsigned long long* __restrict__ best,
                                                                  Selection s, uint8_t* __restrict__ fkeep) {
    const int64_t f = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    bool kept = false;
    if (face_ok(a, b, c, V)) {
        const int32_t l = labels[a];
        kept = component_kept(l, face_counts[l], *best, s);
    }
    fkeep[f] = (uint8_t)kept;
}

// rows of 3 words copied bit for bit to their place in the kept order
__global__ __launch_bounds__(CLEAN_BLOCK) void compact_vertices_kernel(
    int32_t V, const uint8_t* __restrict__ vkeep, const int32_t* __restrict__ voff,
    const uint32_t* __restrict__ vertices, const uint32_t* __restrict__ normals, const uint32_t* __restrict__ colors,
    uint32_t* __restrict__ out_vertices, uint32_t* __restrict__ out_normals, uint32_t* __restrict__ out_colors) {
    const int64_t v = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
    if (v >= V || !vkeep[v]) return;
    const int64_t o = voff[v];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_vertices[3 * o + k] = vertices[3 * v + k];
        out_normals[3 * o + k] = normals[3 * v + k];
        if (colors) out_colors[3 * o + k] = colors[3 * v + k];
    }
}

// a kept face passed face_ok and its three vertices share its component: they are kept too
__global__ __launch_bounds__(CLEAN_BLOCK) void compact_faces_kernel(const int32_t* __restrict__ faces, int32_t F,
                                                                   const uint8_t* __restrict__ fkeep,
                                                                   const int32_t* __restrict__ foff,
                                                                   const int32_t* __restrict__ voff,
                                                                   int32_t* __restrict__ out_faces) {
    const int64_t f = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
    if (f >= F || !fkeep[f]) return;
    const int64_t o = foff[f];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * o + k] = voff[faces[3 * f + k]];
}

struct MaskLattice {
    int nx, ny;
    float lo[3], step[3];
};

// One thread per lattice point, x fastest (as lattice_points_kernel of mesh.hip, whose fp32
// position expression this repeats).  The cell is lookup_cell's (ray_march.hpp) with the position's
// mip alone: there is no ray here, hence no dt term.
__global__ __launch_bounds__(CLEAN_BLOCK) void occupancy_mask_kernel(float* __restrict__ sigma, MaskLattice L,
                                                                    int64_t n,
                                                                    const uint8_t* __restrict__ bitfield,
                                                                    int cascades, int grid_size, float scale) {
    const int64_t p = (int64_t)blockIdx.x * CLEAN_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t pu = (uint32_t)p;  // n < 2^31
    const uint32_t r = pu / (uint32_t)L.nx;
    const uint32_t ix = pu - r * (uint32_t)L.nx, iz = r / (uint32_t)L.ny, iy = r - iz * (uint32_t)L.ny;
    const float x = L.lo[0] + (float)ix * L.step[0];
    const float y = L.lo[1] + (float)iy * L.step[1];
    const float z = L.lo[2] + (float)iz * L.step[2];
    bool occ = false;
    if (fabsf(x) <= scale && fabsf(y) <= scale && fabsf(z) <= scale) {  // a NaN position is outside
        const int mip = mfn::mip_from_pos(x, y, z, cascades);
        const float mip_bound = fminf(scalbnf(1.0f, mip - 1), scale);
        const float inv = 1 / mip_bound;
        const float gs = (float)grid_size, gm1 = (float)grid_size - 1.0f;
        const int cx = (int)mfn::clampf(0.5f * fmaf(x, inv, 1.0f) * gs, 0.0f, gm1);
        const int cy = (int)mfn::clampf(0.5f * fmaf(y, inv, 1.0f) * gs, 0.0f, gm1);
        const int cz = (int)mfn::clampf(0.5f * fmaf(z, inv, 1.0f) * gs, 0.0f, gm1);
        const uint32_t g3 = (uint32_t)grid_size * grid_size * grid_size;
        const uint32_t idx = (uint32_t)mip * g3 + mfn::morton3((uint32_t)cx, (uint32_t)cy, (uint32_t)cz);
        occ = (bitfield[idx >> 3] >> (idx & 7)) & 1u;
    }
    if (!occ) sigma[p] = 0.0f;
}

// 0 <= V, F < 2^31
bool mesh_sizes_ok(const char* what, int64_t V, int64_t F) {
    constexpr int64_t LIM = (int64_t)1 << 31;
    if (V < 0 || F < 0) {
        mfn_set_error("%s: negative size (V %lld, F %lld)", what, (long long)V, (long long)F);
        return false;
    }
    if (V >= LIM || F >= LIM) {
        mfn_set_error("%s: the mesh must have fewer than 2^31 vertices and faces (V %lld, F %lld)", what,
                      (long long)V, (long long)F);
        return false;
    }
    return true;
}

unsigned blocks_for(int64_t n) { return (unsigned)mfn::div_up<int64_t>(n, CLEAN_BLOCK); }
unsigned item_blocks_for(int64_t n) { return (unsigned)mfn::div_up<int64_t>(n, BLOCK_ITEMS); }  // ITEMS per thread

}  // namespace

extern "C" {

int mfnerf_mesh_components(const int32_t* faces, int64_t V, int64_t F, int32_t* labels, int32_t* face_counts,
                           mfnerf_stream_t stream) {
    if (!mesh_sizes_ok("mesh_components", V, F)) return MFN_ERR_INVALID;
    if (!faces || !labels || !face_counts) {
        mfn_set_error("mesh_components: null pointer");
        return MFN_ERR_INVALID;
    }
    if (V == 0 || F == 0) return MFN_OK;
    hipLaunchKernelGGL(components_init_kernel, dim3(blocks_for(V)), dim3(CLEAN_BLOCK), 0, stream, (int32_t)V, labels,
                       face_counts);
    hipLaunchKernelGGL(components_hook_kernel, dim3(blocks_for(F)), dim3(CLEAN_BLOCK), 0, stream, faces, (int32_t)V,
                       (int32_t)F, labels);
    hipLaunchKernelGGL(components_flatten_kernel, dim3(blocks_for(V)), dim3(CLEAN_BLOCK), 0, stream, (int32_t)V,
                       labels);
    hipLaunchKernelGGL(components_count_kernel, dim3(item_blocks_for(F)), dim3(CLEAN_BLOCK), 0, stream, faces, (int32_t)V,
                       (int32_t)F, labels, face_counts);
    return mfn_check_launch("mesh_components");
}

int mfnerf_mesh_select(const int32_t* faces, int64_t V, int64_t F, const int32_t* labels, const int32_t* face_counts,
                       int64_t min_faces, float min_fraction, int64_t largest_only, uint8_t* vkeep, uint8_t* fkeep,
                       int64_t* stats, mfnerf_stream_t stream) {
    if (!mesh_sizes_ok("mesh_select", V, F)) return MFN_ERR_INVALID;
    if (min_faces < 0 || !(min_fraction >= 0.0f && min_fraction <= 1.0f)) {
        mfn_set_error("mesh_select: min_faces must be >= 0 and min_fraction in [0, 1] (got %lld and %g)",
                      (long long)min_faces, (double)min_fraction);
        return MFN_ERR_INVALID;
    }
    if (!faces || !labels || !face_counts || !vkeep || !fkeep || !stats) {
        mfn_set_error("mesh_select: null pointer");
        return MFN_ERR_INVALID;
    }
    if (V == 0 || F == 0) return MFN_OK;
    Selection s;
    s.min_faces = (int32_t)(min_faces < INT32_MAX ? min_faces : INT32_MAX);  // no count exceeds F < 2^31
    s.min_fraction = min_fraction;
    s.largest_only = largest_only != 0;
    unsigned long long* best = reinterpret_cast<unsigned long long*>(stats + 2);
    mfn_zero_async(stats, 3 * sizeof(int64_t), stream);
    hipLaunchKernelGGL(select_best_kernel, dim3(item_blocks_for(V)), dim3(CLEAN_BLOCK), 0, stream, (int32_t)V, face_counts,
                       best);
    hipLaunchKernelGGL(select_vertices_kernel, dim3(item_blocks_for(V)), dim3(CLEAN_BLOCK), 0, stream, (int32_t)V, labels,
                       face_counts, best, s, vkeep, reinterpret_cast<long long*>(stats));
    hipLaunchKernelGGL(select_faces_kernel, dim3(blocks_for(F)), dim3(CLEAN_BLOCK), 0, stream, faces, (int32_t)V,
                       (int32_t)F, labels, face_counts, best, s, fkeep);
    return mfn_check_launch("mesh_select");
}

int mfnerf_mesh_compact(const float* vertices, const float* normals, const float* colors, const int32_t* faces,
                        int64_t V, int64_t F, const uint8_t* vkeep, const int32_t* voff, const uint8_t* fkeep,
                        const int32_t* foff, float* out_vertices, float* out_normals, float* out_colors,
                        int32_t* out_faces, mfnerf_stream_t stream) {
    if (!mesh_sizes_ok("mesh_compact", V, F)) return MFN_ERR_INVALID;
    if (!vertices || !normals || !faces || !vkeep || !voff || !fkeep || !foff || !out_vertices || !out_normals ||
        !out_faces || (colors && !out_colors)) {
        mfn_set_error("mesh_compact: null pointer");
        return MFN_ERR_INVALID;
    }
    if (V == 0 || F == 0) return MFN_OK;
    auto words = [](const float* p) { return reinterpret_cast<const uint32_t*>(p); };
    hipLaunchKernelGGL(compact_vertices_kernel, dim3(blocks_for(V)), dim3(CLEAN_BLOCK), 0, stream, (int32_t)V, vkeep,
                       voff, words(vertices), words(normals), words(colors),
                       reinterpret_cast<uint32_t*>(out_vertices), reinterpret_cast<uint32_t*>(out_normals),
                       reinterpret_cast<uint32_t*>(out_colors));
    hipLaunchKernelGGL(compact_faces_kernel, dim3(blocks_for(F)), dim3(CLEAN_BLOCK), 0, stream, faces, (int32_t)F,
                       fkeep, foff, voff, out_faces);
    return mfn_check_launch("mesh_compact");
}

int mfnerf_mesh_occupancy_mask(float* sigma, const float* lo, const float* hi, int64_t nx, int64_t ny, int64_t nz,
                               const uint8_t* bitfield, int64_t bitfield_bytes, int64_t cascades, int64_t grid_size,
                               float scale, mfnerf_stream_t stream) {
    constexpr int64_t LIM = (int64_t)1 << 31;
    if (nx < 2 || ny < 2 || nz < 2) {
        mfn_set_error("mesh_occupancy_mask: every resolution must be >= 1 (lattice %lld x %lld x %lld points)",
                      (long long)nx, (long long)ny, (long long)nz);
        return MFN_ERR_INVALID;
    }
    if (nx >= LIM || ny >= LIM || nz >= LIM || nx * ny >= LIM || nx * ny * nz >= LIM) {
        mfn_set_error("mesh_occupancy_mask: the lattice must have fewer than 2^31 points (%lld x %lld x %lld)",
                      (long long)nx, (long long)ny, (long long)nz);
        return MFN_ERR_INVALID;
    }
    // Morton codes of cells < G fill [0, G^3) only for a power of two; 10 bits per axis
    if (cascades < 1 || cascades > 32 || grid_size < 1 || grid_size > 1024 || (grid_size & (grid_size - 1)) ||
        cascades * grid_size * grid_size * grid_size >= LIM) {
        mfn_set_error("mesh_occupancy_mask: cascades must be in [1, 32] and grid_size a power of two <= 1024 with "
                      "cascades * grid_size^3 < 2^31 (got %lld and %lld)", (long long)cascades, (long long)grid_size);
        return MFN_ERR_INVALID;
    }
    const int64_t need = (cascades * grid_size * grid_size * grid_size + 7) / 8;
    if (bitfield_bytes < need) {
        mfn_set_error("mesh_occupancy_mask: the bitfield has %lld bytes, %lld cascades of %lld^3 cells need %lld",
                      (long long)bitfield_bytes, (long long)cascades, (long long)grid_size, (long long)need);
        return MFN_ERR_INVALID;
    }
    if (!(scale > 0.0f)) {
        mfn_set_error("mesh_occupancy_mask: scale must be positive (got %g)", (double)scale);
        return MFN_ERR_INVALID;
    }
    if (!sigma || !lo || !hi || !bitfield) {
        mfn_set_error("mesh_occupancy_mask: null pointer");
        return MFN_ERR_INVALID;
    }
    MaskLattice L;
    L.nx = (int)nx;
    L.ny = (int)ny;
    const int64_t r[3] = {nx - 1, ny - 1, nz - 1};
    for (int a = 0; a < 3; ++a) {
        L.lo[a] = lo[a];
        L.step[a] = (hi[a] - lo[a]) / (float)r[a];
    }
    const int64_t n = nx * ny * nz;
    hipLaunchKernelGGL(occupancy_mask_kernel, dim3(blocks_for(n)), dim3(CLEAN_BLOCK), 0, stream, sigma, L, n, bitfield,
                       (int)cascades, (int)grid_size, scale);
    return mfn_check_launch("mesh_occupancy_mask");
}

}  // extern "C"
