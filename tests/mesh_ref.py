"""numpy restatement of the density-lattice mesh extraction (csrc/mesh.hip, mfnerf/mesh.py): marching
tetrahedra on the Kuhn split of every lattice cell.  This file is the specification; the kernels
match it (faces as integers, vertices to fp32 rounding).

Lattice: (nx, ny, nz) = (Rx+1, Ry+1, Rz+1) points, sigma[z, y, x], linear index (z*ny + y)*nx + x,
world position lo + i * ((hi - lo) / R) per axis in fp32 (one division, one multiply, one add).
Cube corners are bit codes x = 1, y = 2, z = 4; for each permutation (a, b, c) of (1, 2, 4), in
itertools.permutations order, one tetrahedron (0, a, a|b, 7): six of them around the body diagonal,
the same split in every cell, so neighbouring cells agree on the diagonal of their shared face.
A tetrahedron's corners are nested as bit sets, so each of its edges runs from a lattice point p
(the "owner", the end with the smaller linear index) to p + d, d in {0,1}^3 \\ {0}: 7 edge types,
named by the bit code of d.

inside = sigma > threshold (NaN outside, +inf inside).  An edge crosses when exactly one end is
inside; its vertex is p0 + t*d (in lattice steps), t = (thr - s0) / (s1 - s0) in fp32, a non-finite
t replaced by 0.5, then clamped to [0, 1].  Vertices are ordered by owner index, then edge type;
faces by cell index ((z*Ry + y)*Rx + x), tetrahedron, triangle of the case.  Triangle normals point
from inside to outside.  Vertex normals are -grad sigma: central differences at the edge's two ends
(one-sided on the lattice boundary, each axis divided by its world step), interpolated with t and
normalised; a zero or non-finite gradient gives (0, 0, 0).  Here the normals are fp64.
"""
import itertools

import numpy as np

TETS = tuple((0, a, a | b, 7) for a, b, c in itertools.permutations((1, 2, 4)))


def _corner(code):
    return np.array([code & 1, (code >> 1) & 1, (code >> 2) & 1], dtype=np.float64)


def build_table():
    """table[t][case] = list of triangles of tetrahedron t when the corners in `case` (bit i = corner
    i in tetrahedron order) are inside; a triangle is three edges, an edge (u, d): from cube corner u
    to cube corner u | d.  One or three corners inside: one triangle; two inside corners a < b with
    outside corners c < d: the quad q = (a-c, a-d, b-d, b-c) as (q0, q1, q2), (q0, q2, q3).  Each
    triangle is wound, with its vertices at the edge midpoints of the unit cube, so that
    (v1 - v0) x (v2 - v0) points from the inside corners' centroid to the outside corners'."""
    table = []
    for tet in TETS:
        per_case = []
        for case in range(16):
            ins = [i for i in range(4) if case >> i & 1]
            outs = [i for i in range(4) if not case >> i & 1]
            if len(ins) in (0, 4):
                tris = []
            elif len(ins) == 1:
                tris = [[(ins[0], o) for o in outs]]
            elif len(ins) == 3:
                tris = [[(i, outs[0]) for i in ins]]
            else:
                (a, b), (c, d) = ins, outs
                q = [(a, c), (a, d), (b, d), (b, c)]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            out = []
            for tri in tris:
                mid = [(_corner(tet[i]) + _corner(tet[j])) / 2 for i, j in tri]
                towards = np.mean([_corner(tet[i]) for i in outs], 0) - np.mean([_corner(tet[i]) for i in ins], 0)
                w = float(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), towards))
                assert abs(w) > 1e-9, (tet, case)
                if w < 0:
                    tri = [tri[0], tri[2], tri[1]]
                edges = []
                for i, j in tri:
                    u, v = min(tet[i], tet[j]), max(tet[i], tet[j])
                    assert u & v == u  # nested: the owner is the smaller code
                    edges.append((u, v ^ u))
                out.append(edges)
            per_case.append(out)
        table.append(per_case)
    return table


TABLE = build_table()
TRI_COUNT = [len(TABLE[0][c]) for c in range(16)]
assert all([len(TABLE[t][c]) for c in range(16)] == TRI_COUNT for t in range(6))


def lattice_axis(lo, hi, R, n=None):
    """World coordinates of one axis' lattice points, in fp32."""
    lo, hi = np.float32(lo), np.float32(hi)
    step = np.float32((hi - lo) / np.float32(R))
    return (lo + np.arange(R + 1 if n is None else n, dtype=np.float32) * step).astype(np.float32), step


def _as3(v):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    return np.repeat(a, 3) if a.size == 1 else a


def _gradient(s64, steps):
    """(gx, gy, gz) of sigma[z, y, x] at every lattice point, fp64."""
    out = []
    for axis, step in ((2, steps[0]), (1, steps[1]), (0, steps[2])):
        s = np.moveaxis(s64, axis, 0)
        g = np.empty_like(s)
        g[1:-1] = (s[2:] - s[:-2]) / (2.0 * step)
        g[0] = (s[1] - s[0]) / step
        g[-1] = (s[-1] - s[-2]) / step
        out.append(np.moveaxis(g, 0, axis))
    return out


def extract(sigma, threshold, lo=-0.5, hi=0.5):
    """sigma (nz, ny, nx) float32 -> {"vertices" (V,3) f32, "normals" (V,3) f64, "faces" (F,3) i32,
    "cases" (6,16) histogram of tetrahedron cases over all cells, "vcount" (n,) u8, "tcount" (cells,) u8}."""
    sigma = np.ascontiguousarray(sigma, dtype=np.float32)
    nz, ny, nx = sigma.shape
    assert min(nx, ny, nz) >= 2
    thr = np.float32(threshold)
    lo3, hi3 = _as3(lo), _as3(hi)
    n = nx * ny * nz
    inside = sigma > thr

    # crossing[p, d-1]: the edge of type d owned by p exists and crosses
    crossing = np.zeros((nz, ny, nx, 7), dtype=bool)
    for d in range(1, 8):
        dx, dy, dz = d & 1, d >> 1 & 1, d >> 2 & 1
        a = inside[:nz - dz, :ny - dy, :nx - dx]
        b = inside[dz:, dy:, dx:]
        crossing[:nz - dz, :ny - dy, :nx - dx, d - 1] = a != b
    crossing = crossing.reshape(n, 7)
    vcount = crossing.sum(1)
    voff = np.cumsum(vcount) - vcount
    rank = np.cumsum(crossing, 1) - crossing  # crossing edges of the owner below this type
    owner, dm1 = np.nonzero(crossing)          # row-major: by owner, then by type
    d = dm1 + 1
    V = owner.size

    # vertices
    x0, y0, z0 = owner % nx, owner // nx % ny, owner // (nx * ny)
    dxyz = np.stack([d & 1, d >> 1 & 1, d >> 2 & 1], 1)
    p1 = owner + dxyz[:, 0] + dxyz[:, 1] * nx + dxyz[:, 2] * nx * ny
    flat = sigma.reshape(-1)
    s0, s1 = flat[owner], flat[p1]
    with np.errstate(all="ignore"):
        t = ((thr - s0) / (s1 - s0)).astype(np.float32)
    t = np.where(np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
    t = np.clip(t, np.float32(0), np.float32(1))
    vertices = np.empty((V, 3), dtype=np.float32)
    steps = []
    for k, (i0, R) in enumerate(((x0, nx - 1), (y0, ny - 1), (z0, nz - 1))):
        _, step = lattice_axis(lo3[k], hi3[k], R)
        steps.append(step)
        pos0 = (lo3[k] + i0.astype(np.float32) * step).astype(np.float32)
        vertices[:, k] = pos0 + (t * dxyz[:, k].astype(np.float32)) * step

    # normals, fp64
    with np.errstate(all="ignore"):
        g = _gradient(sigma.astype(np.float64), [float(s) for s in steps])
        g = np.stack([c.reshape(-1) for c in g], 1)
        gi = g[owner] + t.astype(np.float64)[:, None] * (g[p1] - g[owner])
        length = np.sqrt((gi * gi).sum(1))
        ok = np.isfinite(length) & (length > 0)
        normals = np.where(ok[:, None], -gi / np.where(ok, length, 1.0)[:, None], 0.0)

    # faces
    Rx, Ry, Rz = nx - 1, ny - 1, nz - 1
    cells = Rx * Ry * Rz
    corner_in = [inside[(c >> 2 & 1):(c >> 2 & 1) + Rz, (c >> 1 & 1):(c >> 1 & 1) + Ry, (c & 1):(c & 1) + Rx]
                 .reshape(-1).astype(np.int64) for c in range(8)]
    case = np.stack([sum(corner_in[tet[i]] << i for i in range(4)) for tet in TETS], 1)  # (cells, 6)
    ntri = np.asarray(TRI_COUNT)[case]
    tcount = ntri.sum(1)
    cases = np.stack([np.bincount(case[:, t], minlength=16) for t in range(6)])
    valid = np.stack([ntri > 0, ntri > 1], 2)          # (cells, 6, 2)
    cell, tet_i, k = np.nonzero(valid)                 # by cell, tetrahedron, triangle
    tab_u = np.zeros((6, 16, 2, 3), dtype=np.int64)
    tab_d = np.ones((6, 16, 2, 3), dtype=np.int64)
    for t_ in range(6):
        for c in range(16):
            for kk, tri in enumerate(TABLE[t_][c]):
                for j, (u, dd) in enumerate(tri):
                    tab_u[t_, c, kk, j], tab_d[t_, c, kk, j] = u, dd
    cs = case[cell, tet_i]
    u = tab_u[tet_i, cs, k]                            # (F, 3)
    dd = tab_d[tet_i, cs, k]
    cx, cy, cz = cell % Rx, cell // Rx % Ry, cell // (Rx * Ry)
    own = ((cz[:, None] + (u >> 2 & 1)) * ny + cy[:, None] + (u >> 1 & 1)) * nx + cx[:, None] + (u & 1)
    assert crossing[own, dd - 1].all()
    faces = (voff[own] + rank[own, dd - 1]).astype(np.int32)
    return {"vertices": vertices, "normals": normals, "faces": faces.reshape(-1, 3), "cases": cases,
            "vcount": vcount.astype(np.uint8), "tcount": tcount.astype(np.uint8), "t": t}


# ------------------------------------------------------------------------------- mesh measures
def edge_table(faces):
    """Undirected edges of a face list: (edges (E,2) sorted pairs, uses (E,), balance (E,)): how
    many faces hold each edge, and the number of times it runs low->high minus high->low."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    key = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)
    sign = np.where(a < b, 1, -1)
    if key.shape[0] == 0:
        return key, np.zeros(0, np.int64), np.zeros(0, np.int64)
    edges, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    uses = np.bincount(inv, minlength=edges.shape[0])
    balance = np.bincount(inv, weights=sign, minlength=edges.shape[0]).astype(np.int64)
    return edges, uses, balance


def euler_characteristic(n_vertices, faces):
    edges, _, _ = edge_table(faces)
    return int(n_vertices) - edges.shape[0] + np.asarray(faces).reshape(-1, 3).shape[0]


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ------------------------------------------------------------------------------- test fields
def lattice_xyz(R, lo=-0.5, hi=0.5):
    """(X, Y, Z) fp64 coordinate arrays of shape (nz, ny, nx) for R = int or (Rx, Ry, Rz)."""
    Rx, Ry, Rz = (R, R, R) if np.isscalar(R) else R
    lo3, hi3 = _as3(lo), _as3(hi)
    ax = [lattice_axis(lo3[k], hi3[k], r)[0].astype(np.float64) for k, r in enumerate((Rx, Ry, Rz))]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return X, Y, Z


SPHERE_C, SPHERE_THR, SPHERE_R = (0.013, -0.021, 0.007), -0.3, 0.3
TORUS_C, TORUS_THR, TORUS_MAJOR, TORUS_MINOR = (0.01, -0.02, -0.013), -0.1, 0.25, 0.1


def sphere_field(X, Y, Z, c=SPHERE_C):
    return -np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)


def torus_field(X, Y, Z, c=TORUS_C):
    return -np.sqrt((np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2) - TORUS_MAJOR) ** 2 + (Z - c[2]) ** 2)


def two_spheres_field(X, Y, Z):
    return np.maximum(sphere_field(X, Y, Z, (0.22, 0.0, 0.0)), sphere_field(X, Y, Z, (-0.22, 0.0, 0.0)))


def sphere_outward(v, c=SPHERE_C):
    return np.asarray(v, dtype=np.float64) - np.asarray(c)


def torus_outward(v, c=TORUS_C):
    """Direction from the nearest point of the torus' centre circle."""
    p = np.asarray(v, dtype=np.float64) - np.asarray(c)
    rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
    ring = np.stack([p[:, 0] / rho, p[:, 1] / rho, np.zeros_like(rho)], 1) * TORUS_MAJOR
    return p - ring
