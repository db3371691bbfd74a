"""numpy restatement of the mesh cleaning (csrc/mesh_clean.hip, mfnerf/mesh.py: components,
clean_mesh, occupancy_mask).  This file is the specification; the kernels match it exactly -- labels,
counts, flags and the cleaned arrays are compared with ==.

Components.  Two vertices are connected when a face holds both; a component is a class of the
transitive closure.  A vertex's label is the smallest vertex index of its component; a component's
face count is the number of faces whose first vertex carries its label (all three do); face_counts[r]
holds it at r = the label and 0 elsewhere.  A vertex in no face is a component of its own with count
0.  A face with an index outside [0, V) connects nothing, counts nowhere and is never kept.  The
definition is stated twice: by union-find (`components`) and by breadth-first search over a vertex
adjacency list (`components_bfs`).

Selection.  max_count = the largest face count.  A component is kept when count > 0,
count >= min_faces and float64(count) >= float64(float32(min_fraction)) * float64(max_count); with
largest_only only the component with the largest count, the smallest label among equals.

Compaction.  Stable: kept vertices and faces keep their relative order, per-vertex rows are copied
bit for bit, face indices go through the exclusive scan of the vertex keep flags.

Occupancy mask.  Lattice positions in fp32 (mesh_ref.lattice_axis, the expression of
mfnerf_mesh_lattice_points).  A point with any |coordinate| > scale is cleared.  Otherwise
mip = clip(frexp(max |coordinate|).exponent + 1, 0, cascades - 1), mip_bound = min(2^(mip-1), scale),
cell = floor(clip(0.5 * (x / mip_bound + 1) * G, 0, G - 1)) per axis (here in fp64), m = its Morton
index, and the point is cleared when bit (mip*G^3 + m) & 7 of byte (mip*G^3 + m) >> 3 is clear."""
import numpy as np

import mesh_ref as M


def _valid(V, faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return f, ((f >= 0) & (f < V)).all(1)


def _face_counts(V, f, ok, labels):
    counts = np.zeros(V, dtype=np.int32)
    np.add.at(counts, labels[f[ok, 0]], 1)
    return counts


def components(V, faces):
    """(labels (V,) i32, face_counts (V,) i32) by union-find, the smaller root on top."""
    f, ok = _valid(V, faces)
    parent = list(range(V))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b, c in f[ok].tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    labels = np.asarray([find(v) for v in range(V)], dtype=np.int32).reshape(V)
    return labels, _face_counts(V, f, ok, labels)


def components_bfs(V, faces):
    """The same by breadth-first search: vertices in increasing order, each unlabelled one floods
    its component with its own index over the adjacency list of all three edges of every face."""
    f, ok = _valid(V, faces)
    g = f[ok]
    a = np.concatenate([g[:, 0], g[:, 1], g[:, 2], g[:, 1], g[:, 2], g[:, 0]])
    b = np.concatenate([g[:, 1], g[:, 2], g[:, 0], g[:, 0], g[:, 1], g[:, 2]])
    order = np.argsort(a, kind="stable")
    nbr = b[order]
    start = np.searchsorted(a[order], np.arange(V + 1))
    labels = np.full(V, -1, dtype=np.int32)
    for s in range(V):
        if labels[s] >= 0:
            continue
        labels[s] = s
        frontier = [s]
        while frontier:
            nxt = []
            for u in frontier:
                for w in nbr[start[u]:start[u + 1]].tolist():
                    if labels[w] < 0:
                        labels[w] = s
                        nxt.append(w)
            frontier = nxt
    return labels, _face_counts(V, f, ok, labels)


def select(labels, face_counts, min_faces=0, min_fraction=0.0, largest_only=False):
    """keep (V,) bool by LABEL: keep[r] for the component labelled r (False at non-labels)."""
    V = labels.shape[0]
    keep = np.zeros(V, dtype=bool)
    if V == 0:
        return keep
    counts = face_counts.astype(np.int64)
    max_count = int(counts.max())
    bound = np.float64(np.float32(min_fraction)) * np.float64(max_count)
    roots = np.flatnonzero(labels == np.arange(V))
    ok = (counts[roots] > 0) & (counts[roots] >= int(min_faces)) & (counts[roots].astype(np.float64) >= bound)
    if largest_only:
        best = roots[counts[roots] == max_count].min()  # roots is increasing: the smallest label
        ok &= roots == best
    keep[roots[ok]] = True
    return keep


def clean(mesh, min_faces=0, min_fraction=0.0, largest_only=False):
    """mesh: {"vertices" (V,3), "normals" (V,3), "faces" (F,3), optionally "colors" (V,3)} arrays ->
    the cleaned mesh with "components": (total, kept)."""
    V = mesh["vertices"].shape[0]
    labels, counts = components(V, mesh["faces"])
    keep = select(labels, counts, min_faces, min_fraction, largest_only)
    f, ok = _valid(V, mesh["faces"])
    vkeep = keep[labels] if V else np.zeros(0, dtype=bool)
    fkeep = ok.copy()
    fkeep[ok] = vkeep[f[ok, 0]]
    voff = np.cumsum(vkeep) - vkeep
    out = {k: mesh[k][vkeep].copy() for k in ("vertices", "normals", "colors") if mesh.get(k) is not None}
    out["faces"] = voff[f[fkeep]].astype(np.int32).reshape(-1, 3)
    out["components"] = (int((labels == np.arange(V)).sum()), int(keep.sum()))
    return out


def component_table(V, faces):
    """[(label, faces, vertices, euler characteristic)] of the components with a face, by label."""
    labels, counts = components(V, faces)
    f, ok = _valid(V, faces)
    rows = []
    for r in np.flatnonzero(counts > 0):
        nv = int((labels == r).sum())
        rows.append((int(r), int(counts[r]), nv, M.euler_characteristic(nv, f[ok][labels[f[ok, 0]] == r])))
    return rows


def permuted(mesh, seed):
    """The same mesh with its vertex indices renamed by a random permutation: vertex v becomes
    perm[v], the per-vertex rows move with it, the faces keep their order.  Returns (mesh, perm)."""
    V = mesh["vertices"].shape[0]
    perm = np.random.default_rng(seed).permutation(V)
    return renamed(mesh, perm), perm


def renamed(mesh, perm):
    inv = np.argsort(perm)
    out = {k: np.ascontiguousarray(mesh[k][inv]) for k in ("vertices", "normals", "colors") if mesh.get(k) is not None}
    out["faces"] = perm[np.asarray(mesh["faces"], dtype=np.int64)].astype(np.int32).reshape(-1, 3)
    return out


# ------------------------------------------------------------------------------- test inputs
SPECKS = ((2, 2, 2), (17, 3, 9), (4, 16, 15), (10, 18, 2), (18, 17, 17))  # (x, y, z), no two adjacent
R_INPUT = 20


def speck_field():
    """sphere_field at R = 20 with the isolated lattice points SPECKS, all farther than 0.42 from the
    sphere's centre, raised to 0.0: each is a closed component of 24 faces around one point."""
    X, Y, Z = M.lattice_xyz(R_INPUT)
    s = M.sphere_field(X, Y, Z)
    for x, y, z in SPECKS:
        assert s[z, y, x] < -0.42
        s[z, y, x] = 0.0
    return s.astype(np.float32)


def input_lattices():
    """name -> (sigma (nz, ny, nx) f32, threshold): the lattices of the cleaning tests."""
    X, Y, Z = M.lattice_xyz(R_INPUT)
    rng = np.random.default_rng(0)
    noise_a, noise_b = rng.random((11, 11, 11)), rng.random((11, 11, 11))
    return {"two_spheres": (M.two_spheres_field(X, Y, Z).astype(np.float32), -0.15),
            "torus": (M.torus_field(X, Y, Z).astype(np.float32), M.TORUS_THR),
            "shell": ((-np.abs(-M.sphere_field(X, Y, Z) - 0.3)).astype(np.float32), -0.08),
            "noise": (noise_a.astype(np.float32), 0.5),
            "sparse_noise": (noise_b.astype(np.float32), 0.85),
            "specks": (speck_field(), M.SPHERE_THR)}


CLOSED_INPUTS = ("two_spheres", "torus", "shell", "specks")
_INPUTS = {}


def input_meshes():
    """name -> {"vertices", "normals" (f32), "colors" (random f32), "faces"} of input_lattices(),
    extracted by mesh_ref.extract: computed once, shared, read-only."""
    if not _INPUTS:
        rng = np.random.default_rng(7)
        for name, (sigma, thr) in input_lattices().items():
            e = M.extract(sigma, thr)
            m = {"vertices": e["vertices"], "normals": e["normals"].astype(np.float32),
                 "colors": rng.random(e["vertices"].shape, dtype=np.float32), "faces": e["faces"]}
            for a in m.values():
                a.setflags(write=False)
            _INPUTS[name] = m
    return _INPUTS


# ------------------------------------------------------------------------------- occupancy
def lattice_positions(lo, hi, R):
    """fp32 world coordinates (x, y, z), each of shape (nz, ny, nx), R = int or (Rx, Ry, Rz)."""
    Rx, Ry, Rz = (R, R, R) if np.isscalar(R) else R
    lo3, hi3 = M._as3(lo), M._as3(hi)
    ax = [M.lattice_axis(lo3[k], hi3[k], r)[0] for k, r in enumerate((Rx, Ry, Rz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x, y, z


def _cells(lo, hi, R, cascades, scale, G):
    """(inside the box (nz,ny,nx) bool, mip (nz,ny,nx), u (3,nz,ny,nx) fp64 continuous cell
    coordinates 0.5 * (x / mip_bound + 1) * G, largest |coordinate| fp64)."""
    x, y, z = lattice_positions(lo, hi, R)
    s32 = np.float32(scale)
    inside = (np.abs(x) <= s32) & (np.abs(y) <= s32) & (np.abs(z) <= s32)
    mx = np.maximum(np.abs(x), np.maximum(np.abs(y), np.abs(z)))
    mip = np.clip(np.frexp(mx)[1] + 1, 0, cascades - 1).astype(np.int64)
    bound = np.minimum(np.ldexp(1.0, mip - 1), np.float64(s32))
    u = np.stack([0.5 * (c.astype(np.float64) / bound + 1.0) * G for c in (x, y, z)])
    return inside, mip, u, mx.astype(np.float64)


def occupancy_mask(lo, hi, R, bitfield, cascades, scale, G):
    """(nz, ny, nx) bool: True where the lattice value stays, False where it is cleared."""
    import torch

    from oracle import vren_oracle
    inside, mip, u, _ = _cells(lo, hi, R, cascades, scale, G)
    cell = np.floor(np.clip(u, 0.0, G - 1.0)).astype(np.int32).reshape(3, -1).T
    m = vren_oracle.morton3D(torch.from_numpy(np.ascontiguousarray(cell))).numpy().astype(np.int64)
    idx = mip.reshape(-1) * G ** 3 + m
    bits = np.asarray(bitfield, dtype=np.uint8).reshape(-1)
    idx = np.where(inside.reshape(-1), idx, 0)  # points outside the box are cleared whatever they index
    occ = (bits[idx >> 3] >> (idx & 7).astype(np.uint8)) & 1
    return (inside.reshape(-1) & (occ == 1)).reshape(inside.shape)


def rounding_margins(lo, hi, R, cascades, scale, G):
    """How far the lattice is from a decision that fp32 and fp64 arithmetic could take differently:
    (smallest distance, in cells, of an in-box point from a cell boundary of its cascade;
     smallest distance of any point's largest |coordinate| from a power of two or from scale)."""
    inside, _, u, mx = _cells(lo, hi, R, cascades, scale, G)
    cell_margin = float(np.abs(u - np.rint(u))[:, inside].min()) if inside.any() else np.inf
    marks = np.concatenate([np.ldexp(1.0, np.arange(-40, 12)), [np.float64(np.float32(scale))]])
    mip_margin = float(np.abs(mx.reshape(-1, 1) - marks.reshape(1, -1)).min())
    return cell_margin, mip_margin
