// mesh.hip -- a triangle mesh of the density field's iso-surface, extracted on the device (the
// reference's test.ipynb "mesh" cell: model.density on an N^3 lattice, copied to the host, then
// mcubes.marching_cubes(sigma, sigma_threshold)).  Here the lattice never leaves HBM.
//
// Marching tetrahedra on the Kuhn split (mesh_table.hpp; the specification is tests/mesh_ref.py):
// six tetrahedra around each cell's body diagonal, the same split in every cell, so neighbouring
// cells agree on their shared face diagonals and no case is ambiguous.  Every tetrahedron edge
// runs from a lattice point p, its owner, to p + d, d in {0,1}^3 \ {0}: 7 edge types named by
// the bit code of d (x = 1, y = 2, z = 4).  A crossing edge carries one vertex, numbered
// voff[owner] + (crossing edges of the owner of a lower type); the owner's crossing mask is
// recomputed from sigma wherever it is needed, never stored.
//
// Two stencil passes, one thread per lattice point in x-fastest order.  The thread of point p needs
// the eight corners p + d of the cell at p: they are both the far ends of p's seven owned edges
// and the cell's corners.  It loads the four with dx = 0 and takes the four with dx = 1 from the
// next lane, so a wave covers 63 consecutive points and its last lane only supplies values.  Each
// sigma value is fetched from HBM once; the other three reads of it (rows y+1, planes z+1) hit L2.
// Indexing is int64 wherever a product of extents appears.
#include "common.hpp"
#include "mesh_table.hpp"

namespace {

using namespace mfn_mesh;

constexpr int MESH_BLOCK = 256;
constexpr int WAVE_POINTS = 63;                               // lane 63 is the halo of lane 62
constexpr int BLOCK_POINTS = (MESH_BLOCK / 64) * WAVE_POINTS; // lattice points per workgroup

// triangles of a tetrahedron case from its population count; checked against the generated table
__host__ __device__ constexpr int tri_count(unsigned c) {
    const int pc = (int)((c & 1) + (c >> 1 & 1) + (c >> 2 & 1) + (c >> 3 & 1));
    return pc == 2 ? 2 : (pc == 0 || pc == 4) ? 0 : 1;
}
constexpr bool tri_count_matches_table() {
    for (unsigned c = 0; c < 16; ++c)
        if (tri_count(c) != TRI_COUNT[c]) return false;
    return true;
}
static_assert(tri_count_matches_table(), "TRI_COUNT is 0/1/2 by the number of inside corners");
static_assert(N_TETS == 6, "the Kuhn split has six tetrahedra");

struct Lattice {
    int nx, ny, nz;
    float lo[3], step[3];
};

struct Point {
    int x, y, z;
    int64_t p;
};

__device__ __forceinline__ Point point_of(int64_t p, int nx, int ny) {
    // p < 2^31 + a workgroup (the entry points check the lattice): 32-bit divisions
    const uint32_t pu = (uint32_t)p;
    const uint32_t r = pu / (uint32_t)nx;
    Point q;
    q.x = (int)(pu - r * (uint32_t)nx);
    q.z = (int)(r / (uint32_t)ny);
    q.y = (int)(r - (uint32_t)q.z * (uint32_t)ny);
    q.p = p;
    return q;
}

// NaN is outside, +inf inside
__device__ __forceinline__ bool is_inside(float s, float thr) { return s > thr; }

// The corners p + d (d = 0..7) of the cell at p that lie on the lattice: their values, `have` (bit d:
// the corner exists) and `in` (bit d: it exists and is inside).
struct Corners {
    float s[8];
    unsigned have, in;
};

// the lattice point of this thread in a stencil pass (it may lie beyond the lattice)
__device__ __forceinline__ int64_t stencil_point() {
    return (int64_t)blockIdx.x * BLOCK_POINTS + (threadIdx.x >> 6) * WAVE_POINTS + (threadIdx.x & 63);
}
// ... and whether the thread has work there; EVERY thread of a wave calls load_corners first
__device__ __forceinline__ bool stencil_active(int64_t p, int64_t n) {
    return (threadIdx.x & 63) < WAVE_POINTS && p < n;
}

// Wave-collective.  Lane l + 1 holds point p + 1: where p's x + 1 is on the lattice, that is the
// point (x + 1, y, z) of the same row, whose own (dy, dz) corners exist exactly when p's do.
__device__ __forceinline__ Corners load_corners(const float* __restrict__ sigma, const Point& q, bool on_lattice,
                                                int nx, int ny, int nz, float thr) {
    const int64_t sy = nx, sz = (int64_t)nx * ny;
    const bool hx = q.x + 1 < nx, hy = q.y + 1 < ny, hz = q.z + 1 < nz;
    Corners c;
    c.have = 0;
    c.in = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // k = dy | dz << 1
        const bool ok = on_lattice && (!(k & 1) || hy) && (!(k & 2) || hz);
        const float own = ok ? sigma[q.p + (k & 1) * sy + (k >> 1) * sz] : 0.0f;
        const float next = __shfl_down(own, 1);
        c.s[2 * k] = own;
        c.s[2 * k + 1] = next;
        c.have |= (unsigned)ok << (2 * k) | (unsigned)(ok && hx) << (2 * k + 1);
        c.in |= (unsigned)(ok && is_inside(own, thr)) << (2 * k) |
                (unsigned)(ok && hx && is_inside(next, thr)) << (2 * k + 1);
    }
    return c;
}

// bit d (1..7): p's edge of type d exists and exactly one of its ends is inside
__device__ __forceinline__ unsigned crossing_mask(const Corners& c) {
    return ((c.in & 1u) ? ~c.in : c.in) & c.have & 0xFEu;
}

__device__ __forceinline__ unsigned tet_case(unsigned in, int t) {
    return (in >> TET_CORNER[t][0] & 1u) | (in >> TET_CORNER[t][1] & 1u) << 1 | (in >> TET_CORNER[t][2] & 1u) << 2 |
           (in >> TET_CORNER[t][3] & 1u) << 3;
}

__global__ __launch_bounds__(MESH_BLOCK) void lattice_points_kernel(Lattice L, int64_t first, int64_t count,
                                                                    float* __restrict__ xyz) {
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= count) return;
    const Point q = point_of(first + i, L.nx, L.ny);
    xyz[3 * i] = L.lo[0] + (float)q.x * L.step[0];
    xyz[3 * i + 1] = L.lo[1] + (float)q.y * L.step[1];
    xyz[3 * i + 2] = L.lo[2] + (float)q.z * L.step[2];
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_count_kernel(const float* __restrict__ sigma, int nx, int ny,
                                                                int nz, float thr, uint8_t* __restrict__ vcount,
                                                                uint8_t* __restrict__ tcount) {
    const int64_t n = (int64_t)nx * ny * nz;
    const int64_t p = stencil_point();
    const Point q = point_of(p, nx, ny);
    const Corners c = load_corners(sigma, q, p < n, nx, ny, nz, thr);
    if (!stencil_active(p, n)) return;
    vcount[p] = (uint8_t)__popc(crossing_mask(c));
    if (c.have != 0xFFu) return;  // no cell at p
    int nt = 0;
    if (c.in != 0u && c.in != 0xFFu) {
#pragma unroll
        for (int t = 0; t < N_TETS; ++t) nt += tri_count(tet_case(c.in, t));
    }
    tcount[((int64_t)q.z * (ny - 1) + q.y) * (nx - 1) + q.x] = (uint8_t)nt;
}

// d sigma / d axis at lattice coordinate i of an axis with n points (stride st in sigma): central,
// one-sided on the boundary, per world step
__device__ __forceinline__ float axis_gradient(const float* __restrict__ sigma, int64_t p, int i, int n, int64_t st,
                                               float step) {
    if (i == 0) return (sigma[p + st] - sigma[p]) / step;
    if (i == n - 1) return (sigma[p] - sigma[p - st]) / step;
    return (sigma[p + st] - sigma[p - st]) / (2.0f * step);
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_emit_kernel(const float* __restrict__ sigma, Lattice L, float thr,
                                                               const int32_t* __restrict__ voff,
                                                               const int32_t* __restrict__ toff,
                                                               float* __restrict__ vertices,
                                                               float* __restrict__ normals,
                                                               int32_t* __restrict__ faces) {
    const int nx = L.nx, ny = L.ny, nz = L.nz;
    const int64_t sy = nx, sz = (int64_t)nx * ny;
    const int64_t n = sz * nz;
    const int64_t p = stencil_point();
    const Point q = point_of(p, nx, ny);
    const Corners c = load_corners(sigma, q, p < n, nx, ny, nz, thr);
    if (!stencil_active(p, n)) return;
    const unsigned cross = crossing_mask(c);

    // ---- the vertices of p's crossing edges, in type order
    if (cross) {
        int64_t v = voff[p];
        const float g0x = axis_gradient(sigma, p, q.x, nx, 1, L.step[0]);
        const float g0y = axis_gradient(sigma, p, q.y, ny, sy, L.step[1]);
        const float g0z = axis_gradient(sigma, p, q.z, nz, sz, L.step[2]);
        const float px = L.lo[0] + (float)q.x * L.step[0];
        const float py = L.lo[1] + (float)q.y * L.step[1];
        const float pz = L.lo[2] + (float)q.z * L.step[2];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!(cross >> d & 1u)) continue;
            float t = (thr - c.s[0]) / (c.s[d] - c.s[0]);
            if (!isfinite(t)) t = 0.5f;
            t = mfn::clampf(t, 0.0f, 1.0f);
            const int dx = d & 1, dy = d >> 1 & 1, dz = d >> 2 & 1;
            vertices[3 * v] = dx ? px + t * L.step[0] : px;
            vertices[3 * v + 1] = dy ? py + t * L.step[1] : py;
            vertices[3 * v + 2] = dz ? pz + t * L.step[2] : pz;
            const int64_t p1 = p + dx + dy * sy + dz * sz;
            const float g1x = axis_gradient(sigma, p1, q.x + dx, nx, 1, L.step[0]);
            const float g1y = axis_gradient(sigma, p1, q.y + dy, ny, sy, L.step[1]);
            const float g1z = axis_gradient(sigma, p1, q.z + dz, nz, sz, L.step[2]);
            const float gx = g0x + t * (g1x - g0x), gy = g0y + t * (g1y - g0y), gz = g0z + t * (g1z - g0z);
            const float len = sqrtf(gx * gx + gy * gy + gz * gz);
            const bool ok = isfinite(len) && len > 0.0f;  // a non-finite component makes len non-finite
            normals[3 * v] = ok ? -gx / len : 0.0f;
            normals[3 * v + 1] = ok ? -gy / len : 0.0f;
            normals[3 * v + 2] = ok ? -gz / len : 0.0f;
            ++v;
        }
    }

    // ---- the triangles of the cell at p
    if (c.have != 0xFFu || c.in == 0u || c.in == 0xFFu) return;
    // The crossing masks (bit d-1: type d) of the seven corners that can own an edge of this cell,
    // 7 bits each.  Far ends inside the cell are known from c.in; the others are loaded.
    uint64_t masks = 0;
#pragma unroll
    for (int u = 0; u < 7; ++u) {
        const int ox = q.x + (u & 1), oy = q.y + (u >> 1 & 1), oz = q.z + (u >> 2 & 1);
        const int64_t o = p + (u & 1) + (u >> 1 & 1) * sy + (u >> 2 & 1) * sz;
        const bool hx = ox + 1 < nx, hy = oy + 1 < ny, hz = oz + 1 < nz;
        const unsigned in_u = c.in >> u & 1u;
        unsigned m = 0;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            unsigned far_in;
            bool ok = true;
            if ((u & d) == 0) {
                far_in = c.in >> (u | d) & 1u;
            } else {
                ok = (!(d & 1) || hx) && (!(d & 2) || hy) && (!(d & 4) || hz);
                far_in = ok ? (unsigned)is_inside(sigma[o + (d & 1) + (d >> 1 & 1) * sy + (d >> 2 & 1) * sz], thr) : 0u;
            }
            m |= (unsigned)(ok && far_in != in_u) << (d - 1);
        }
        masks |= (uint64_t)m << (7 * u);
    }
    int64_t f = toff[((int64_t)q.z * (ny - 1) + q.y) * (nx - 1) + q.x];
#pragma unroll
    for (int t = 0; t < N_TETS; ++t) {
        const unsigned cs = tet_case(c.in, t);
        const int nt = tri_count(cs);
        for (int k = 0; k < nt; ++k) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned e = TRI_EDGE[t][cs][3 * k + j];
                const unsigned u = e & 7u, d = e >> 3;
                const unsigned m = (unsigned)(masks >> (7 * u)) & 0x7Fu;
                const int64_t o = p + (u & 1u) + (u >> 1 & 1u) * sy + (u >> 2 & 1u) * sz;
                faces[3 * f + j] = voff[o] + __popc(m & ((1u << (d - 1)) - 1u));
            }
            ++f;
        }
    }
}

// nx, ny, nz >= 2 and nx*ny*nz < 2^31, without overflowing on absurd sizes
bool lattice_ok(const char* what, int64_t nx, int64_t ny, int64_t nz) {
    constexpr int64_t LIM = (int64_t)1 << 31;
    if (nx < 2 || ny < 2 || nz < 2) {
        mfn_set_error("%s: every resolution must be >= 1 (lattice %lld x %lld x %lld points)", what, (long long)nx,
                      (long long)ny, (long long)nz);
        return false;
    }
    if (nx >= LIM || ny >= LIM || nz >= LIM || nx * ny >= LIM || nx * ny * nz >= LIM) {
        mfn_set_error("%s: the lattice must have fewer than 2^31 points (%lld x %lld x %lld)", what, (long long)nx,
                      (long long)ny, (long long)nz);
        return false;
    }
    return true;
}

bool make_lattice(const char* what, const float* lo, const float* hi, int64_t nx, int64_t ny, int64_t nz,
                  Lattice* L) {
    if (!lattice_ok(what, nx, ny, nz)) return false;
    if (!lo || !hi) {
        mfn_set_error("%s: null pointer", what);
        return false;
    }
    L->nx = (int)nx;
    L->ny = (int)ny;
    L->nz = (int)nz;
    const int64_t r[3] = {nx - 1, ny - 1, nz - 1};
    for (int a = 0; a < 3; ++a) {
        L->lo[a] = lo[a];
        L->step[a] = (hi[a] - lo[a]) / (float)r[a];
    }
    return true;
}

}  // namespace

extern "C" {

int mfnerf_mesh_lattice_points(const float* lo, const float* hi, int64_t nx, int64_t ny, int64_t nz, int64_t first,
                               int64_t count, float* xyz, mfnerf_stream_t stream) {
    Lattice L;
    if (!make_lattice("mesh_lattice_points", lo, hi, nx, ny, nz, &L)) return MFN_ERR_INVALID;
    const int64_t n = nx * ny * nz;
    if (first < 0 || count < 0 || first > n || count > n - first) {
        mfn_set_error("mesh_lattice_points: points %lld .. %lld + %lld lie outside the lattice's %lld",
                      (long long)first, (long long)first, (long long)count, (long long)n);
        return MFN_ERR_INVALID;
    }
    if (!xyz) {
        mfn_set_error("mesh_lattice_points: null pointer");
        return MFN_ERR_INVALID;
    }
    if (count == 0) return MFN_OK;
    hipLaunchKernelGGL(lattice_points_kernel, dim3((unsigned)mfn::div_up<int64_t>(count, MESH_BLOCK)),
                       dim3(MESH_BLOCK), 0, stream, L, first, count, xyz);
    return mfn_check_launch("mesh_lattice_points");
}

int mfnerf_mesh_count(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float threshold, uint8_t* vcount,
                      uint8_t* tcount, mfnerf_stream_t stream) {
    if (!lattice_ok("mesh_count", nx, ny, nz)) return MFN_ERR_INVALID;
    if (!sigma || !vcount || !tcount) {
        mfn_set_error("mesh_count: null pointer");
        return MFN_ERR_INVALID;
    }
    const int64_t n = nx * ny * nz;
    hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)mfn::div_up<int64_t>(n, BLOCK_POINTS)), dim3(MESH_BLOCK), 0,
                       stream, sigma, (int)nx, (int)ny, (int)nz, threshold, vcount, tcount);
    return mfn_check_launch("mesh_count");
}

int mfnerf_mesh_emit(const float* sigma, int64_t nx, int64_t ny, int64_t nz, float threshold, const int32_t* voff,
                     const int32_t* toff, const float* lo, const float* hi, float* vertices, float* normals,
                     int32_t* faces, mfnerf_stream_t stream) {
    Lattice L;
    if (!make_lattice("mesh_emit", lo, hi, nx, ny, nz, &L)) return MFN_ERR_INVALID;
    if (!sigma || !voff || !toff || !vertices || !normals || !faces) {
        mfn_set_error("mesh_emit: null pointer");
        return MFN_ERR_INVALID;
    }
    const int64_t n = nx * ny * nz;
    hipLaunchKernelGGL(mesh_emit_kernel, dim3((unsigned)mfn::div_up<int64_t>(n, BLOCK_POINTS)), dim3(MESH_BLOCK), 0,
                       stream, sigma, L, threshold, voff, toff, vertices, normals, faces);
    return mfn_check_launch("mesh_emit");
}

}  // extern "C"
